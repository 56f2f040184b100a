"""Inputs shared by the BGZF tests (test_bgzf_host.py, test_bgzf_sanitized.py, test_gpu_bgzf.py): raw-DEFLATE members
made with zlib at test time (and two written bit by bit, for what zlib never emits), seeded damage to them, BGZF files in
and out of the format, and a stand-in for the device side of utils_v2.GetTensorDevice that inflates with zlib."""
import functools
import struct
import zlib

import numpy as np

import textparse_cases as T

OK, HOST = 1, 2                       # CV_BGZF_* of include/clairvoyante_amd.h


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    """raw DEFLATE of `data`; flush_at: byte offsets at which a Z_FULL_FLUSH ends the block"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = [], 0
    for cut in list(flush_at) + [len(data)]:
        out.append(c.compress(data[at:cut]))
        if cut < len(data):
            out.append(c.flush(zlib.Z_FULL_FLUSH))
        at = cut
    return b"".join(out) + c.flush()


class _FixedBits(object):
    """a block in the fixed Huffman code, written bit by bit (RFC 1951 3.2.6): what zlib never emits"""
    LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
    DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                 8193, 12289, 16385, 24577]
    DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.bits(1, 1); self.bits(1, 2)                     # BFINAL, BTYPE = 01

    def bits(self, v, k):                                    # k bits, least significant first
        self.acc |= v << self.n; self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xff); self.acc >>= 8; self.n -= 8

    def code(self, v, k):                                    # a Huffman code: most significant bit first
        self.bits(int(format(v, "0%db" % k)[::-1], 2), k)

    def symbol(self, s):
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xc0 + s - 280, 8)

    def literals(self, data):
        for b in data:
            self.symbol(b)

    def match(self, length, dist):
        k = max(i for i in range(29) if self.LEN_BASE[i] <= length and (i < 28 or length == 258))
        if length == 258: k = 28
        self.symbol(257 + k); self.bits(length - self.LEN_BASE[k], self.LEN_EXTRA[k])
        d = max(i for i in range(30) if self.DIST_BASE[i] <= dist)
        self.code(d, 5); self.bits(dist - self.DIST_BASE[d], self.DIST_EXTRA[d])

    def end(self):
        self.symbol(256)
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def _far_matches():
    """matches at distance 32 768 (zlib itself stops at 32 506), one of them overlapping the member's first byte"""
    rng = np.random.RandomState(11)
    head = rng.randint(0, 256, 32768).astype(np.uint8).tobytes()
    w = _FixedBits()
    w.literals(head)
    w.match(258, 32768); w.match(3, 32768); w.literals(b"xyz"); w.match(100, 32768); w.match(258, 1); w.match(37, 2)
    return w.end()


@functools.lru_cache(maxsize=1)
def corpus():
    """-> [(name, DEFLATE data, the bytes it inflates to)]: every construct the issue lists.  No member of it may come
    back HOST."""
    text = T.volume_text(2000)
    rows = text[:65280]
    rng = np.random.RandomState(7)
    noise = rng.randint(0, 256, 60000).astype(np.uint8).tobytes()
    out = []
    for level in (0, 1, 6, 9):
        out.append(("rows_level%d" % level, deflate(rows if level else rows[:60000], level)))
    for name, strategy in (("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED)):
        out.append(("rows_" + name, deflate(rows, 6, strategy)))
    out.append(("noise_stored", deflate(noise, 6)))
    out.append(("noise_level0", deflate(noise, 0)))
    out.append(("full_flushes", deflate(rows, 6, flush_at=(1, 5000, 5000, 40000))))
    out.append(("mixed_blocks", deflate(rows[:20000] + noise[:20000] + b"\0" * 20000, 6, flush_at=(20000, 40000))))
    out.append(("empty", deflate(b"")))
    out.append(("empty_stored", deflate(b"", 0)))
    out.append(("one_byte", deflate(b"A")))
    out.append(("full_65536", deflate(text[1000:1000 + 65536], 6)))
    out.append(("full_65536_level1", deflate(text[70000:70000 + 65536], 1)))
    out.append(("run_of_one_byte", deflate(b"a" * 65536, 9)))
    out.append(("run_of_two_bytes", deflate(b"ab" * 30000, 9)))
    out.append(("short_periods", deflate(b"".join(bytes(range(65, 65 + p)) * (700 // p) for p in range(1, 70)), 9)))
    out.append(("far_matches", _far_matches()))
    out.append(("binary_ramp", deflate(bytes(range(256)) * 200, 6)))
    for k in range(6):                                       # short members, as a writer with small blocks makes them
        out.append(("rows_short_%d" % k, deflate(text[k * 3001:k * 3001 + 700 * (k + 1)], (1, 6, 9)[k % 3])))
    res = []
    for name, data in out:
        raw = zlib.decompress(data, -15)
        assert len(raw) <= 65536 and len(data) <= 65536, name
        res.append((name, data, raw))
    far = dict((n, r) for n, _d, r in res)["far_matches"]
    assert far[32768:32768 + 258] == far[:258] and len(far) == 32768 + 258 + 3 + 3 + 100 + 258 + 37
    return res


def small_corpus():
    """members of a few KB for the mutation runs: (name, data, raw)"""
    text = T.volume_text(2000)
    rng = np.random.RandomState(19)
    out = []
    for k, (level, strategy) in enumerate(((1, 0), (6, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE), (0, 0))):
        raw = text[k * 5000:k * 5000 + 2500 + 300 * k]
        out.append(("rows_%d_%d" % (level, strategy), deflate(raw, level, strategy), raw))
    raw = rng.randint(0, 256, 1500).astype(np.uint8).tobytes() + b"z" * 1000
    out.append(("noise_and_run", deflate(raw, 6, flush_at=(700,)), raw))
    w = _FixedBits(); w.literals(b"abcdefgh"); w.match(258, 8); w.match(20, 3); w.match(5, 1)
    data = w.end()
    out.append(("hand_written", data, zlib.decompress(data, -15)))
    return out


def zlib_verdict(data, isize, crc):
    """what zlib makes of a (possibly damaged) member: its bytes when the stream is valid, ends with the data, and gives
    `isize` bytes with CRC-32 `crc`; None otherwise"""
    d = zlib.decompressobj(-15)
    try:
        raw = d.decompress(data, 1 << 20) + d.flush()
    except zlib.error:
        return None
    if not d.eof or d.unused_data or d.unconsumed_tail or len(raw) != isize or zlib.crc32(raw) != crc:
        return None
    return raw


def mutations(count, seed):
    """-> generator of (data, isize, crc) of `count` damaged members: bit flips, truncations, appended bytes, swapped
    byte pairs (the LEN / NLEN words of stored blocks among them), wrong ISIZE in both directions, a wrong CRC"""
    base = small_corpus()
    rng = np.random.RandomState(seed)
    for i in range(count):
        _name, data, raw = base[i % len(base)]
        isize, crc = len(raw), zlib.crc32(raw)
        b = bytearray(data)
        kind = rng.randint(0, 8)
        if kind <= 2:                                        # one to three flipped bits; early bits (the block headers) favoured
            for _ in range(1 + rng.randint(0, 3)):
                at = rng.randint(0, min(len(b), 40) if rng.randint(0, 3) == 0 else len(b))
                b[at] ^= 1 << rng.randint(0, 8)
        elif kind == 3:
            del b[rng.randint(0, len(b)):]
        elif kind == 4:
            p, q = rng.randint(0, len(b), 2)
            b[p], b[q] = b[q], b[p]
            if rng.randint(0, 2):
                b[:4] = b[2:4] + b[:2]
        elif kind == 5:
            isize = max(0, isize + int(rng.choice([-1, 1])) * int(rng.choice([1, 2, 7, 64, 300, 5000])))
        elif kind == 6:
            b += bytes(rng.randint(0, 256, rng.randint(1, 9)).astype(np.uint8))
        else:
            crc ^= 1 << rng.randint(0, 32)
        yield bytes(b), min(isize, 65536), crc


def bgzf_member(body, raw_len, crc, extra=b""):
    """one BGZF member around the DEFLATE data `body`; `extra`: further subfields in front of BC"""
    xlen = 6 + len(extra)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\0" +
            struct.pack("<H", 12 + xlen + len(body) + 8 - 1) + body + struct.pack("<II", crc, raw_len))


def bgzf_file(text, block=65280, level=6, eof=True):
    """`text` as BGZF members of `block` input bytes"""
    out = [bgzf_member(deflate(text[at:at + block], level), len(text[at:at + block]), zlib.crc32(text[at:at + block]))
           for at in range(0, len(text), block)]
    return b"".join(out) + (bgzf_member(deflate(b""), 0, 0) if eof else b"")


def walk(data):
    """the members of a BGZF file, in Python: [(offset of the DEFLATE data, its length, ISIZE, CRC-32)]"""
    out, p = [], 0
    while p < len(data) and data[p] != 0:
        xlen = struct.unpack_from("<H", data, p + 10)[0]
        at, bsize = p + 12, None
        while at < p + 12 + xlen:
            sid, slen = data[at:at + 2], struct.unpack_from("<H", data, at + 2)[0]
            if sid == b"BC":
                bsize = struct.unpack_from("<H", data, at + 4)[0] + 1
            at += 4 + slen
        crc, isize = struct.unpack_from("<II", data, p + bsize - 8)
        out.append((p + 12 + xlen, bsize - 12 - xlen - 8, isize, crc))
        p += bsize
    return out


class ZlibSlabDevice(T.AllHostDevice):
    """T.AllHostDevice (every line HOST, nothing parsed) with the BGZF methods of utils_v2._TextSlabDevice: members are
    inflated with zlib into a numpy buffer, so the slab / tail logic of GetTensorDevice runs without a GPU"""

    def upload_bgzf(self, slab, head):
        parts = [np.zeros(head, dtype=np.uint8)]
        for off, clen, _at, _packed in slab.table:
            parts.append(np.frombuffer(zlib.decompress(bytes(slab.comp[off:off + clen]), -15), dtype=np.uint8))
        if slab.last:
            parts.append(np.array([10], dtype=np.uint8))
        text = np.concatenate(parts)
        assert len(text) == head + slab.n + (1 if slab.last else 0)
        return text, len(text)

    def settle(self, up, slab, head):
        pass

    def carry(self, frm, lo, hi, up, at):
        up[at:at + hi - lo] = frm[lo:hi]

    def grow(self, up, end, extra):
        return np.concatenate((np.zeros(extra, dtype=np.uint8), up[:end]))

    def host_text(self, up, lo, hi):
        return up[lo:hi]

    def tokens(self, job, keep, meta):
        raise AssertionError("every line is HOST here: the positions come from the host text")
