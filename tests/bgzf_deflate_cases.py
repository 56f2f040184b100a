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


def host_form(text, block):
    """cv_bgzf_deflate_host_form -> (file bytes without the EOF marker, sizes, info)"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    members = max(1, -(-len(text) // block))
    src = np.frombuffer(text, dtype=np.uint8) if len(text) else np.zeros(1, dtype=np.uint8)
    out = np.zeros(members * (block + 31), dtype=np.uint8)
    sizes, info = np.zeros(members, dtype=np.int32), np.zeros(8, dtype=np.int64)
    V = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(lib.cv_bgzf_deflate_host_form(V(src), len(text), block, V(out), len(out), V(sizes), V(info)))
    return out[:int(info[0])].tobytes(), sizes, info


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
