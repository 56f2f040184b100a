"""Inputs of the BGZF compressor's tests: three texts made by the project's own formatters and generators (tensor rows,
VCF records, a candidate list), the special texts of tests/native/bgzf_deflate_driver.cpp, and the judges every member
faces -- zlib, gzip and the project's own scan -- none of which is the code under test."""
import ctypes
import gzip
import struct
import zlib

import numpy as np

import vcf_merge_cases as vc

BLOCKS = (64, 1000, 4096, 65280)
HEAD = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"
_cache = {}


def tensor_rows():
    """about 130 KB of CreateTensor's rows (cv_format_tensor_row): mostly "0.0", counts where reads would lie"""
    from clairvoyante_amd import pileup
    rs = np.random.RandomState(23)
    k = 57
    ref = bytes(rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 4000).tolist())
    centers = np.sort(rs.choice(np.arange(100, 3900), k, replace=False)) + 1
    counts = np.zeros((k, 33, 4, 4), dtype=np.float32)
    depth = rs.randint(8, 60, (k, 33, 1))
    counts[:, :, :, 0] = np.where(rs.rand(k, 33, 4) < 0.3, depth, 0)
    counts[:, :, :, 1:] = np.where(rs.rand(k, 33, 4, 3) < 0.04, rs.randint(1, 9, (k, 33, 4, 3)), 0)
    rows = pileup.format_rows("chr20", centers, ref, 0, counts)
    return b"".join(r + b"\n" for r in rows)


def vcf_records():
    return b"".join(vc.expected_order(vc.records(2000)))


def candidate_list():
    from clairvoyante_amd import ExtractVariantCandidates as evc
    rs = np.random.RandomState(29)
    n = 3000
    pos0 = np.sort(rs.choice(np.arange(10, 5000000), n, replace=False)).astype(np.int64)
    depth = rs.randint(10, 80, n)
    alt = (depth * rs.uniform(0.1, 0.6, n)).astype(np.int64)
    counts = np.zeros((n, len(evc.SYMBOLS)), dtype=np.int64)
    major, minor = rs.randint(0, 4, n), rs.randint(0, 6, n)
    counts[np.arange(n), major] += depth - alt
    counts[np.arange(n), minor] += alt
    ref = bytes(rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 5000010).tolist())
    res = {"pos0": pos0, "counts": counts, "late": np.zeros(n, dtype=np.int64), "last_pos": 1 << 40}
    return ("\n".join(evc.candidate_rows("chr20", res, ref, 0)) + "\n").encode()


FIXTURES = {"tensor_rows": tensor_rows, "vcf_records": vcf_records, "candidate_list": candidate_list}


def fixture(name):
    if name not in _cache:
        _cache[name] = FIXTURES[name]()
    return _cache[name]


def special_texts():
    """(name, text): what the sanitizer driver builds, restated"""
    rs = np.random.RandomState(31)
    out = [("run %d" % n, b"z" * n) for n in (257, 258, 259, 260, 261, 516, 517)]
    out += [("period %d" % p, (b"abcd"[:p] * 300)[:1000 + p]) for p in (2, 3, 4)]
    out.append(("random", rs.randint(0, 256, 65280).astype(np.uint8).tobytes()))
    R = rs.randint(0, 200, 300).astype(np.uint8).tobytes()
    out += [("window %d" % far, R + b"\xee" * (far - 300) + R) for far in (32768, 32769)]
    seq = []                                     # every trigram over six symbols exactly once: nothing to match
    a = [0] * 19

    def db(t, p):
        if t > 3:
            if 3 % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, 6):
            a[t] = j
            db(t + 1, t)
    db(1, 1)
    s = bytes(b"ACGT\t\n"[i] for i in seq)
    out.append(("no match", s + s[:2]))
    return out


WORKGROUPS = 512                                 # csrc/cv_bgzf_deflate_dev.hip, MAX_GRID: bd_compress's workgroups
TWO_TRIPS = ((WORKGROUPS + 77, 4096), (WORKGROUPS + 3, 65280))      # (members, block): 16 and 255 tiles of 256 positions each


def two_trip_kind(m):
    """True: member m is text, False: random bytes -- members m and m + WORKGROUPS, which one workgroup takes, differ"""
    return (m // WORKGROUPS + m) % 2 == 0


def two_trip_text(members, block):
    """members of exactly `block` bytes.  A text member is a cut of the three fixtures laid end to end, half a block long,
    and the same cut again: its second half matches block / 2 bytes back, many tiles further than the 256 positions of
    one (at 65 280: 32 640 back, inside the window of 32 768).  The others are random bytes, which no block type but
    stored holds in fewer bytes"""
    rs = np.random.RandomState(37)
    pool = np.frombuffer(b"".join(fixture(n) for n in sorted(FIXTURES)), dtype=np.uint8)
    half = block // 2
    assert block % 2 == 0 and len(pool) > 2 * half
    out = rs.randint(0, 256, (members, block)).astype(np.uint8)
    for m in range(members):
        if two_trip_kind(m):
            at = (m * 7919) % (len(pool) - half)
            out[m, :half] = pool[at:at + half]
            out[m, half:] = out[m, :half]
    return out.tobytes()


def member_kinds(data, sizes):
    """the block type of every member (0 stored, 1 fixed, 2 dynamic), as judge reads it"""
    at = np.concatenate(([0], np.cumsum(sizes)))[:-1]
    return [(data[int(a) + 18] >> 1) & 3 for a in at]


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
              16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]


def match_distances(member):
    """the distances of the matches in one member's single final DEFLATE block (RFC 1951 read in plain Python, for the
    tests that claim something about them) -> list; a stored block has none"""
    bits = int.from_bytes(member[18:-8], "little")
    at = [0]

    def take(n):
        v = (bits >> at[0]) & ((1 << n) - 1)
        at[0] += n
        return v

    def table(lengths):
        code, out = 0, {}
        for ln in range(1, 16):
            for sym, l in enumerate(lengths):
                if l == ln:
                    out[(ln, code)] = sym
                    code += 1
            code <<= 1
        return out

    def symbol(t):
        code = 0
        for ln in range(1, 16):
            code = code << 1 | take(1)
            if (ln, code) in t:
                return t[(ln, code)]
        raise ValueError("no such code")

    assert take(1) == 1
    kind = take(2)
    if kind == 0:
        return []
    if kind == 1:
        lit, dist = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30)
    else:
        hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
        cl = [0] * 19
        for k in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[:hclen]:
            cl[k] = take(3)
        t, lens = table(cl), []
        while len(lens) < hlit + hdist:
            c = symbol(t)
            if c < 16:
                lens.append(c)
            elif c == 16:
                lens += [lens[-1]] * (3 + take(2))
            else:
                lens += [0] * (3 + take(3) if c == 17 else 11 + take(7))
        lit, dist = table(lens[:hlit]), table(lens[hlit:])
    found = []
    while True:
        c = symbol(lit)
        if c == 256:
            return found
        if c > 256:
            take(_LEN_EXTRA[c - 257])
            d = symbol(dist)
            found.append(_DIST_BASE[d] + take(_DIST_EXTRA[d]))


def host_form(text, block, out_cap=None, fill=0):
    """cv_bgzf_deflate_host_form -> (file bytes without the EOF marker, sizes, info); with out_cap, the room the call is
    told the output has: -> (the WHOLE output, `fill` where nothing was written, sizes, info)"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    members = max(1, -(-len(text) // block))
    src = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)
    out = np.full(members * (block + 31), fill, dtype=np.uint8)
    sizes, info = np.zeros(members, dtype=np.int32), np.zeros(8, dtype=np.int64)
    V = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(lib.cv_bgzf_deflate_host_form(V(src), len(text), block, V(out), len(out) if out_cap is None else out_cap, V(sizes), V(info)))
    return (out[:int(info[0])] if out_cap is None else out).tobytes(), sizes, info


def small_output_caps(sizes):
    """the caps of the too-small-output tests -> [(cap, members that fit)]: the exact total, one byte less, the first
    member's end, one byte less, nothing"""
    total, first = int(np.sum(sizes)), int(sizes[0])
    return [(total, len(sizes)), (total - 1, len(sizes) - 1), (first, 1), (first - 1, 0), (0, 0)]


def judge(data, sizes, text, block):
    """every member of `data` (members back to back, no EOF marker) against zlib: the input back with eof set and nothing
    left over, CRC-32, ISIZE and BSIZE; the whole through gzip; -> the block type of every member"""
    assert int(np.sum(sizes)) == len(data)
    at, kinds = 0, []
    for k, size in enumerate(int(s) for s in sizes):
        m = data[at:at + size]
        want = text[k * block:(k + 1) * block]
        assert m[:16] == HEAD and struct.unpack("<H", m[16:18])[0] == size - 1
        d = zlib.decompressobj(-15)
        got = d.decompress(m[18:-8])
        assert got == want and d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(want), len(want))
        assert size <= len(want) + 5 + 26                       # never larger than its stored form
        kinds.append((m[18] >> 1) & 3)
        at += size
    assert gzip.decompress(data) == text
    return kinds
