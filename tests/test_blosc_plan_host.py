"""cv_blosc_plan (the host half of the device's .bin block reader) and the second writer, without a GPU: the plan's
rows against an independent Python reading of the chunk header, its refusals, cv_blosc_compress_lz4_blocks through the
host decoder and through the real c-blosc, and the route rule where there is no device."""
import ctypes
import os
import pickle
import struct

import numpy as np
import pytest

import blosc_cases as B
from clairvoyante_amd import _lib, param, utils_v2

CBLOSC = "/opt/conda/lib/libblosc.so.1"


def plan(chunks, max_nbytes=B.NBYTES_CAP, max_streams=1 << 16):
    lib = _lib.load()
    n = len(chunks)
    hold = [np.frombuffer(c, dtype=np.uint8) for c in chunks]
    src = (ctypes.c_void_p * n)(*[h.ctypes.data for h in hold])
    clen = (ctypes.c_int64 * n)(*[len(c) for c in chunks])
    srows = np.full((max_streams, 5), -7, dtype=np.int64)
    crows = np.full((n, 10), -7, dtype=np.int64)
    ns, comp, scratch = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    refused = lib.cv_blosc_plan(src, clen, n, max_nbytes, max_streams, srows.ctypes.data_as(ctypes.c_void_p),
                                crows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ns), ctypes.byref(comp), ctypes.byref(scratch))
    return refused, srows[:ns.value], crows, comp.value, scratch.value


def read_header(c):
    """an independent reading of a c-blosc 1.x chunk -> (typesize, shuffle, nbytes, blocksize, [(offset in the chunk, cb,
    offset in the decompressed block layout, neblock, stored)])"""
    version, _vl, flags, ts = c[0], c[1], c[2], c[3] or 1
    nbytes, blocksize, _cbytes = struct.unpack_from("<iii", c, 4)
    assert version == 2
    streams = []
    if nbytes == 0:
        return ts, 0, nbytes, blocksize, streams
    if flags & 2:
        return ts, 0, nbytes, blocksize, [(16, nbytes, 0, nbytes, 1)]
    nblocks = -(-nbytes // blocksize)
    for b in range(nblocks):
        bsize = blocksize
        left = b == nblocks - 1 and nbytes % blocksize != 0
        if left:
            bsize = nbytes % blocksize
        splits = ts if (not flags & 0x10 and blocksize // ts >= 128 and not left) else 1
        ip = struct.unpack_from("<i", c, 16 + 4 * b)[0]
        for s in range(splits):
            cb = struct.unpack_from("<i", c, ip)[0]
            streams.append((ip + 4, cb, b * blocksize + s * (bsize // splits), bsize // splits, int(cb == bsize // splits)))
            ip += 4 + cb
    return ts, int(bool(flags & 1) and ts > 1), nbytes, blocksize, streams


def test_plan_rows_match_an_independent_reading_of_the_header():
    corpus = [(n, c) for n, c in B.corpus() if not B.unsupported(c)]
    refused, srows, crows, comp, scratch = plan([c for _n, c in corpus])
    assert refused == 0
    at = sc = s0 = 0
    kinds = set()
    for (name, c), row in zip(corpus, crows):
        ts, shuffle, nbytes, blocksize, streams = read_header(c)
        assert list(row) == [ts, shuffle, nbytes, blocksize, s0, len(streams), sc, 0, at, len(c)], name
        for k, (off, cb, oat, ne, stored) in enumerate(streams):
            assert list(srows[s0 + k]) == [at + off, cb, sc + oat, ne, stored], (name, k)
            kinds.add("stored" if stored else "lz4")
        kinds.add("split" if len(streams) > 2 else "single")
        s0 += len(streams); at += (len(c) + 15) & ~15; sc += (nbytes + 15) & ~15
    assert (s0, at, sc) == (len(srows), comp, scratch)
    assert kinds == {"stored", "lz4", "split", "single"}
    # the stored split of the corpus is one plane of a split block, not a whole chunk
    name, c = [(n, c) for n, c in corpus if n.startswith("stored split")][0]
    st = read_header(c)[4]
    assert 0 < sum(s[4] for s in st) < len(st)


def test_plan_refuses_what_is_not_for_the_device():
    good = dict(B.corpus())["ts4 X, 4 KiB blocks"]
    assert plan([good])[0] == 0

    def patched(at, value):
        c = bytearray(good); c[at] = value
        return bytes(c)
    cases = {
        "version 3": patched(0, 3),
        "bit shuffle": patched(2, good[2] | 0x4),
        "blosclz": patched(2, good[2] & 0x1f),
        "zlib": patched(2, (good[2] & 0x1f) | (3 << 5)),
        "typesize 2": patched(3, 2),
        "typesize 16": patched(3, 16),
        "truncated bstarts": good[:20],
        "truncated header": good[:15],
        "truncated stream": good[:len(good) - 1],
        "bstart inside the header": good[:16] + struct.pack("<i", 8) + good[20:],
        "negative nbytes": good[:4] + struct.pack("<i", -1) + good[8:],
        "blocksize 0": good[:8] + struct.pack("<i", 0) + good[12:],
        "position strings": utils_v2.pack_array(np.array(["chr1:100:ACGT" * 3] * 40)),
    }
    for name, c in cases.items():
        refused, srows, crows, comp, scratch = plan([good, c, good])
        assert refused == 1 and crows[1, 7] == 1 and crows[0, 7] == 0 and crows[2, 7] == 0, name
        assert comp == 2 * ((len(good) + 15) & ~15), name      # a refused chunk takes no room
    assert plan([good], max_nbytes=100)[0] == 1
    assert plan([good], max_streams=3)[0] == 1
    assert plan([], max_streams=0)[0] == 0


def test_the_default_writer_writes_the_bytes_it_always_wrote():
    lib = _lib.load()
    x, _y = B.candidates(24, seed=1)
    data = pickle.dumps(x, pickle.HIGHEST_PROTOCOL)
    out = ctypes.create_string_buffer(len(data) + 64)
    clen = ctypes.c_int64()
    assert lib.cv_blosc_compress_lz4(data, len(data), 4, out, len(out), ctypes.byref(clen)) == 0
    assert utils_v2.blosc_compress(data, 4) == out.raw[:clen.value]
    assert utils_v2.pack_array(x) == out.raw[:clen.value]
    assert utils_v2.PACK_BLOCKSIZE is None


@pytest.mark.parametrize("blocksize", [1024, 4096, 65536, 1 << 20])
def test_new_writer_round_trips(blocksize):
    x, y = B.candidates(60, seed=2)
    cb = ctypes.CDLL(CBLOSC) if os.path.exists(CBLOSC) else None
    for a in (x, y, x[:0], x[:1], np.arange(777, dtype=np.uint8)):
        c = utils_v2.pack_array(a, blocksize)
        assert c[3] == a.itemsize and struct.unpack_from("<i", c, 12)[0] == len(c)
        b = utils_v2.unpack_array(c)
        assert b.dtype == a.dtype and b.shape == a.shape and np.array_equal(a, b)
        if cb is not None:
            raw = pickle.dumps(a, pickle.HIGHEST_PROTOCOL)
            out = ctypes.create_string_buffer(len(raw))
            assert cb.blosc_decompress_ctx(c, out, ctypes.c_size_t(len(raw)), ctypes.c_int(1)) == len(raw)
            assert out.raw == raw


@pytest.mark.skipif(not os.path.exists(CBLOSC), reason="no c-blosc on this machine")
def test_new_writer_has_c_bloscs_layout():
    """the same block and split structure as the real c-blosc gives the same data (the streams differ: lz4 vs lz4hc)"""
    _total, XC, _YC, _PC = utils_v2.LoadBin(os.path.join(B.GOLDEN, "cblosc_x.bin"))
    real = bytes(XC[0])
    mine = utils_v2.blosc_compress(utils_v2.blosc_decompress(real), 4, 1 << 20)
    a, b = read_header(real), read_header(mine)
    assert a[:4] == b[:4] and [(s[2], s[3]) for s in a[4]] == [(s[2], s[3]) for s in b[4]] and len(a[4]) == 5


def test_without_a_gpu_the_route_is_the_hosts(monkeypatch):
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    x, _y = B.candidates(param.bloscBlockSize + 3, seed=3)
    bs = param.bloscBlockSize
    XC = [utils_v2.pack_array(x[s:s + bs]) for s in range(0, len(x) + bs, bs)]
    for env in (None, "device", "host"):
        if env is None:
            monkeypatch.delenv("CV_BIN_DECODE", raising=False)
        else:
            monkeypatch.setenv("CV_BIN_DECODE", env)
        assert utils_v2.bin_decode_route(XC, len(XC)) == "host"
        assert utils_v2.DecompressArrayDevice(XC, 0, len(x), len(x)) is None
    monkeypatch.setenv("CV_BIN_DECODE", "gpu")
    with pytest.raises(_lib.CvError):
        utils_v2.bin_decode_route(XC, len(XC))
    assert utils_v2.bin_layout(XC) == "own"
    assert utils_v2.bin_layout([utils_v2.pack_array(x[:bs], 65536)]) == "own64k"
    assert utils_v2.bin_layout([utils_v2.pack_array(x[:bs], 1 << 20)]) == "cblosc"
    assert set(utils_v2.bin_decode_counts()) == {"device", "host"}
