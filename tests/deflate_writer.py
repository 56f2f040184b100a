"""Test infrastructure: a DEFLATE (RFC 1951) writer at the level of bits, for the streams zlib's deflate never makes but
every inflater must take -- run-length-coded code lengths that run from the literal/length array into the distance array
(libdeflate writes them), a single distance code or none, codes of any depth up to 15, distances up to 32 768, length 258
spelt 284 + 31, stored / fixed / dynamic blocks in any order starting at any bit -- and, through Stream.broken_dynamic /
broken_fixed and the field overrides, headers and blocks that are not DEFLATE at all.  The writer keeps what it wrote (blocks, their
start bits, code lengths, the code-length symbols, tokens), so a corpus can assert its constructs from the record.

A token is an int (a literal byte) or a pair (length, distance)."""
import bisect
import heapq

from bgzf_cases import _FixedBits

LEN_BASE, LEN_EXTRA = _FixedBits.LEN_BASE, _FixedBits.LEN_EXTRA
DIST_BASE, DIST_EXTRA = _FixedBits.DIST_BASE, _FixedBits.DIST_EXTRA
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STORED, FIXED, DYNAMIC = 0, 1, 2
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32

_LEN_SYM = [0] * 259                     # length -> index of its code (258 -> 28)
for _k in range(29):
    for _n in range(LEN_BASE[_k], min(259, LEN_BASE[_k] + (1 << LEN_EXTRA[_k]))):
        _LEN_SYM[_n] = _k
_LEN_SYM[258] = 28


def dist_sym(d):
    return bisect.bisect_right(DIST_BASE, d) - 1


def kraft(lens):
    """sum of 2^-l over the codes, in units of 2^-15: 32 768 = complete"""
    return sum(1 << (15 - l) for l in lens if l)


def canonical(lens):
    """code lengths -> {symbol: (code with its bits reversed, ready for an LSB-first writer, length)}.  An
    over-subscribed set still gets codes (cut to their lengths): the invalid streams need them."""
    mx = max(lens) if lens else 0
    count = [0] * (mx + 2)
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (mx + 2)
    for l in range(1, mx + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            c = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
            out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)
    return out


def limited_lengths(freq, limit):
    """symbol frequencies -> the lengths of a COMPLETE prefix code of at most `limit` bits (7..15) over the symbols with
    a non-zero frequency (at least two of them): Huffman's lengths, cut at the limit, then the cheapest symbols
    lengthened until the code fits and the dearest shortened until it is complete"""
    used = [s for s, f in enumerate(freq) if f]
    assert len(used) >= 2 and len(used) <= (1 << limit) and 1 <= limit <= 15
    heap = [(freq[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    depth = dict((s, 0) for s in used)
    tie = len(freq)
    while len(heap) > 1:
        fa, _a, sa = heapq.heappop(heap)
        fb, _b, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, tie, sa + sb))
        tie += 1
    lens = dict((s, min(d, limit)) for s, d in depth.items())
    unit = lambda l: 1 << (limit - l)
    total = sum(unit(l) for l in lens.values())
    by_cost = sorted(used, key=lambda s: (freq[s], s))
    while total > 1 << limit:                                # over-subscribed by the cut: lengthen rare symbols
        for s in by_cost:
            if lens[s] < limit:
                total -= unit(lens[s]) - unit(lens[s] + 1)
                lens[s] += 1
                break
    while total < 1 << limit:                                # room left: shorten, the longest codes of frequent symbols first
        room = (1 << limit) - total
        fits = [s for s in used if lens[s] > 1 and unit(lens[s]) <= room]
        assert fits, "no code can be shortened"
        s = max(fits, key=lambda s: (lens[s], freq[s], -s))
        total += unit(lens[s])
        lens[s] -= 1
    out = [0] * len(freq)
    for s, l in lens.items():
        out[s] = l
    assert kraft(out) == 1 << 15 and max(out) <= limit
    return out


def completed(lens):
    """further lengths that make the code complete: one code for every set bit of what is missing"""
    room = (1 << 15) - kraft(lens)
    assert room >= 0
    return [l for l in range(1, 16) if room & (1 << (15 - l))]


def expand(tokens, out):
    """the bytes the tokens stand for, appended to the bytearray `out`"""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            n, d = t
            assert 3 <= n <= 258 and 1 <= d <= 32768 and d <= len(out), (t, len(out))
            for _ in range(n):
                out.append(out[-d])
    return out


def tokenize(data, chain=12):
    """LZ77 with a 32 768-byte window (zlib stops at 32 506): at every position the longest match among the last `chain`
    places with the same three bytes and the oldest one in the window, the FARTHEST of equal ones; deterministic"""
    data = bytes(data)
    n, at, toks, seen = len(data), 0, [], {}

    def note(p):
        if p + 3 <= n:
            seen.setdefault(data[p:p + 3], []).append(p)

    while at < n:
        best, best_d = 0, 0
        places = seen.get(data[at:at + 3], [])
        near = places[-chain:][::-1]
        far = bisect.bisect_left(places, at - 32768)         # ... and the oldest place still inside the window
        if far < len(places) - chain:
            near.append(places[far])
        for c in near:
            if at - c > 32768:
                break
            lim = min(258, n - at)
            lo, hi = 3, lim                                  # data[c:c + lo] matches; find the first difference by halving
            if data[c:c + lim] == data[at:at + lim]:
                lo = lim
            else:
                while lo < hi:
                    mid = (lo + hi + 1) // 2
                    if data[c:c + mid] == data[at:at + mid]:
                        lo = mid
                    else:
                        hi = mid - 1
            if lo >= best and lo >= 3:
                best, best_d = lo, at - c
        if best >= 3:
            toks.append((best, best_d))
            for p in range(at, at + best):
                note(p)
            at += best
        else:
            toks.append(data[at])
            note(at)
            at += 1
    return toks


def rle(lens, zeros_only_17=False):
    """code lengths -> [(symbol 0..18, extra value, first index, lengths covered)] with repeats 16 / 17 / 18 where a
    run allows them"""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = lens[i], i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            r = min(run, 138)
            if r >= 11 and not zeros_only_17:
                out.append((18, r - 11, i, r))
            else:
                r = min(r, 10)
                out.append((17, r - 3, i, r))
            i += r
            continue
        out.append((v, 0, i, 1)); i += 1; run -= 1
        while run >= 3:
            r = min(run, 6)
            out.append((16, r - 3, i, r)); i += r; run -= r
    return out


class Block(object):
    """what Stream wrote for one block"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class Stream(object):
    """one DEFLATE stream, block after block into one run of bits"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.text = bytearray()                              # the bytes the stream inflates to, as far as the tokens say
        self.blocks = []

    # ---- bits
    def bits(self, v, k):
        assert 0 <= v < (1 << k) or k == 0
        self.acc |= v << self.n; self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xff); self.acc >>= 8; self.n -= 8

    def tell(self):
        return len(self.out) * 8 + self.n

    def done(self):
        """-> the stream's bytes (the last one padded with zero bits)"""
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)

    def _note(self, kind, final, start, **kw):
        b = Block(kind=kind, final=bool(final), bit=start, out_at=kw.pop("out_at"), **kw)
        self.blocks.append(b)
        return b

    # ---- blocks
    def stored(self, data, final=False):
        data = bytes(data)
        assert len(data) <= 65535
        start, at = self.tell(), len(self.text)
        self.bits(1 if final else 0, 1); self.bits(STORED, 2)
        if self.n:
            self.bits(0, 8 - self.n)
        self.bits(len(data), 16); self.bits(len(data) ^ 0xffff, 16)
        self.out += data
        self.text += data
        return self._note(STORED, final, start, out_at=at, aligned=(start + 3) % 8 == 0, size=len(data))

    def _tokens(self, tokens, lc, dc, len258_as_284, check):
        for t in tokens:
            if isinstance(t, int):
                self.bits(*lc[t])
                if check:
                    self.text.append(t)
                continue
            n, d = t[0], t[1]
            k = 27 if (n == 258 and len258_as_284) else _LEN_SYM[n]
            self.bits(*lc[257 + k]); self.bits(n - LEN_BASE[k], LEN_EXTRA[k])
            if len(t) == 3:                                  # (length, distance, what to write for the distance): for
                if isinstance(t[2], tuple):                  # invalid streams, a symbol (nothing if it has no code) or
                    self.bits(*t[2])                         # (value, bits)
                elif t[2] in dc:
                    self.bits(*dc[t[2]])
            else:
                q = dist_sym(d)
                self.bits(*dc[q]); self.bits(d - DIST_BASE[q], DIST_EXTRA[q])
            if check:
                expand([(n, d)], self.text)

    def fixed(self, tokens, final=False, check=True):
        start, at = self.tell(), len(self.text)
        self.bits(1 if final else 0, 1); self.bits(FIXED, 2)
        lc, dc = canonical(FIXED_LL), canonical(FIXED_DL)
        self._tokens(tokens, lc, dc, False, check)
        self.bits(*lc[256])
        return self._note(FIXED, final, start, out_at=at, tokens=list(tokens))

    def dynamic(self, tokens, ll, dl, final=False, joint=True, cl=None, trim_hclen=True, len258_as_284=False, check=True,
                hlit_field=None, hdist_field=None, ops=None, end=True):
        """a dynamic block from the literal/length lengths `ll` (257..286 of them) and the distance lengths `dl` (1..30).
        joint: the code lengths are run-length coded as ONE array of HLIT + HDIST (a repeat may cross from one into the
        other), else each array for itself, zlib's way.  cl: the 19 lengths of the code-length code (default: a code of
        at most 7 bits from the symbols' frequencies).  trim_hclen: leave out the trailing zero lengths of the
        permuted code-length code.  check=False writes what it is told: codes that are not prefix codes, wrong counts
        (hlit_field / hdist_field: the raw 5-bit fields), `ops` = the code-length symbols [(symbol, extra value)] as
        given, end=False: no end-of-block code."""
        ll, dl = list(ll), list(dl)
        if check:
            assert 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30 and ll[256]
            kl, kd = kraft(ll), kraft(dl)
            assert kl == 1 << 15 or [l for l in ll if l] == [1], "the literal/length code is neither complete nor a single bit"
            assert kd == 1 << 15 or [l for l in dl if l] in ([1], []), "the distance code is neither complete, a single bit nor empty"
        start, at = self.tell(), len(self.text)
        if ops is None:
            runs = rle(ll + dl) if joint else rle(ll) + [(s, e, i + len(ll), r) for s, e, i, r in rle(dl)]
        else:
            runs = [(s, e, -1, 0) for s, e in ops]
        if cl is None:
            freq = [0] * 19
            for r in runs:
                freq[r[0]] += 1
            if sum(1 for f in freq if f) < 2:
                freq[0 if freq[0] == 0 else 1] += 1
            cl = limited_lengths(freq, 7)
        cl = list(cl)
        assert len(cl) == 19 and max(cl) <= 7
        hclen = 19
        if trim_hclen:
            while hclen > 4 and cl[ORDER[hclen - 1]] == 0:
                hclen -= 1
        self.bits(1 if final else 0, 1); self.bits(DYNAMIC, 2)
        self.bits(len(ll) - 257 if hlit_field is None else hlit_field, 5)
        self.bits(len(dl) - 1 if hdist_field is None else hdist_field, 5)
        self.bits(hclen - 4, 4)
        for i in range(hclen):
            self.bits(cl[ORDER[i]], 3)
        cc = canonical(cl)
        for s, e, _i, _r in runs:
            self.bits(*cc[s])
            if s >= 16:
                self.bits(e, {16: 2, 17: 3, 18: 7}[s])
        lc, dc = canonical(ll), canonical(dl)
        self._tokens(tokens, lc, dc, len258_as_284, check)
        if end:
            self.bits(*lc[256])
        complete = len(ll) <= 286 and len(dl) <= 30 and kraft(ll) == 1 << 15 and kraft(dl) == 1 << 15
        return self._note(DYNAMIC, final, start, out_at=at, ll=ll, dl=dl, cl=cl, hclen=hclen, runs=runs, joint=joint,
                          tokens=list(tokens), complete=complete, len258_as_284=len258_as_284)


    def broken_dynamic(self, tokens, ll, dl, **kw):
        """the entry point for headers and blocks that are NOT DEFLATE: dynamic() without its checks"""
        return self.dynamic(tokens, ll, dl, check=False, **kw)

    def broken_fixed(self, tokens, **kw):
        return self.fixed(tokens, check=False, **kw)


def code_for(tokens, ll_limit, dl_limit=None, len258_as_284=False, ll_size=None, dl_size=None):
    """tokens -> (ll, dl): complete codes of at most ll_limit / dl_limit bits from the tokens' own frequencies (trailing
    unused symbols left out unless ll_size / dl_size say otherwise; an unused array gets the spare symbols a complete
    code needs)"""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[257 + (27 if t[0] == 258 and len258_as_284 else _LEN_SYM[t[0]])] += 1
            df[dist_sym(t[1])] += 1
    if sum(1 for f in lf if f) < 2:
        lf[0 if lf[0] == 0 else 1] += 1
    ll = limited_lengths(lf, ll_limit)
    nd = sum(1 for f in df if f)
    if nd == 0:
        dl = [0]
    else:
        if nd == 1:
            df[0 if df[0] == 0 else 1] += 1
        dl = limited_lengths(df, dl_limit or min(ll_limit, 15))
    while ll_size is None and len(ll) > 257 and ll[-1] == 0:
        ll.pop()
    while dl_size is None and len(dl) > 1 and dl[-1] == 0:
        dl.pop()
    return ll[:ll_size] if ll_size else ll, dl[:dl_size] if dl_size else dl


def blocks_for(tokens, limit, per_block=4000):
    """cut the tokens into runs that a code of `limit` bits can carry (at most 3/4 of its 2^limit codes used)"""
    out, cur, syms = [], [], set([256])
    for t in tokens:
        s = t if isinstance(t, int) else 257 + _LEN_SYM[t[0]]
        if len(cur) >= per_block or (s not in syms and len(syms) + 1 > (3 << limit) // 4):
            out.append(cur); cur, syms = [], set([256])
        cur.append(t); syms.add(s)
    out.append(cur)
    return out


def compress(data, limit=15, per_block=4000, joint=True):
    """bytes -> raw DEFLATE through tokenize(): dynamic blocks of at most per_block tokens, code depth at most `limit`"""
    w = Stream()
    parts = blocks_for(tokenize(data), limit, per_block)
    for k, toks in enumerate(parts):
        ll, dl = code_for(toks, limit, min(limit, 15))
        w.dynamic(toks, ll, dl, final=k == len(parts) - 1, joint=joint)
    assert bytes(w.text) == bytes(data)
    return w.done()
