"""Inputs shared by tests/test_gpu_gzip.py and tests/test_gzip_core_host.py: ordinary (non-BGZF) gzip files of text tensor
rows in every shape the device reader meets, and the host restatement of the symbols' resolution."""
import functools
import gzip
import io
import struct
import zlib

import numpy as np

import textparse_cases as T

LANDED, FINAL, PASSED, BAD = 1, 2, 3, 4
MARK = 0x8000


def deflate(text, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    """one gzip member by zlib: memLevel 1..9 ends a block after 128..32 768 symbols, the window stays 32 KiB"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    return c.compress(text) + c.flush()


def raw_deflate(text, level=6, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem)
    return c.compress(text) + c.flush()


def member(raw, text, extra=None, name=None, comment=None, hcrc=False):
    """a gzip member around raw DEFLATE data with the optional header fields of RFC 1952"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff"
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + raw + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def header_end(data):
    """byte at which the DEFLATE data of the file's first member starts"""
    flg, p = data[3], 10
    if flg & 4:
        p += 2 + struct.unpack_from("<H", data, p)[0]
    for bit in (8, 16):
        if flg & bit:
            p = data.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return p


def python_gzip(text, name="tensor.txt"):
    """what Python's gzip module writes: an FNAME header"""
    buf = io.BytesIO()
    with gzip.GzipFile(filename=name, mode="wb", fileobj=buf, mtime=0) as fh:
        fh.write(text)
    data = buf.getvalue()
    assert data[3] & 8
    return data


def full_flush(text, pieces=7):
    """Z_FULL_FLUSH points: an empty stored block between the dynamic ones, and no match across it"""
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    out, step = [], len(text) // pieces + 1
    for at in range(0, len(text), step):
        out.append(c.compress(text[at:at + step]))
        out.append(c.flush(zlib.Z_FULL_FLUSH))
    out.append(c.flush())
    return b"".join(out)


def decoy(inner_text):
    """a gzip file of STORED blocks whose payload is the raw DEFLATE data of a tensor file: valid dynamic headers stand
    where no block starts.  -> (file, its text = that DEFLATE data)"""
    payload = raw_deflate(inner_text, 6, 8)
    return deflate(payload, 0), payload


@functools.lru_cache(maxsize=1)
def kernel_corpus():
    """-> {name: (gzip file, its text, may fall back to the host entirely)}"""
    text = T.volume_text(300)
    out = {}
    for level in (1, 6, 9):
        for mem in (1, 4, 8):
            out["level%d_mem%d" % (level, mem)] = (deflate(text, level, mem), text, False)
    out["python_gzip"] = (python_gzip(text), text, False)
    out["extra_comment_hcrc"] = (member(raw_deflate(text), text, extra=b"AB\x03\0xyz", comment=b"a comment", hcrc=True), text, False)
    out["all_header_fields"] = (member(raw_deflate(text, 6, 4), text, extra=b"", name=b"n", comment=b"", hcrc=True), text, False)
    out["full_flush"] = (full_flush(text), text, True)
    row = text[:text.index(b"\n") + 1]
    out["one_row_3000_times"] = (deflate(row * 3000), row * 3000, True)
    out["empty"] = (deflate(b""), b"", True)
    out["twenty_bytes"] = (deflate(b"chr1 1000 ACGT 1.0 \n"), b"chr1 1000 ACGT 1.0 \n", True)
    for name, (data, t, _f) in out.items():
        assert zlib.decompress(data, 31) == t, name
    return out


def unserved_corpus():
    """files without a dynamic block: nothing for the finder"""
    text = T.volume_text(300)
    return {"level0": (deflate(text, 0), text), "fixed": (deflate(text, 6, 8, zlib.Z_FIXED), text)}


def resolve(sym, window):
    """symbols (uint16) -> bytes with the 32 KiB `window` in front (shorter: what exists)"""
    sym = np.asarray(sym, dtype=np.uint16)
    w = np.zeros(32768, dtype=np.uint8)
    if len(window):
        w[32768 - len(window):] = np.frombuffer(bytes(window), dtype=np.uint8)
    marked = (sym & MARK) != 0
    return np.where(marked, w[sym & (MARK - 1)], (sym & 0xff).astype(np.uint8)).astype(np.uint8).tobytes()
