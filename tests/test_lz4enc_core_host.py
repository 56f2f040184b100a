"""The encode core of the device's .bin block writer (csrc/cv_lz4enc_core.hpp) in its host form, built here with
AddressSanitizer and UBSan (tests/native/lz4enc_core_driver.cpp gives every stream a heap block of exactly its size and
every output one of exactly its cap, neblock - 1).  Every LZ4 block the core writes is parsed here against the format's
end rules, decoded by the STRICT decoder of cv_lz4_core.hpp (inside the driver) and by lz4_decompress (through
cv_blosc_decompress), and must give back the input.  The kernel runs the same text and is held to these bytes by
test_gpu_blosc_pack.py."""
import ctypes
import ctypes.util
import os
import pickle
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import blosc_cases as B
from clairvoyante_amd import _lib, synth, utils_v2

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 65535                       # cve::STREAM_CAP


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("lz4enc_core") / "lz4enc_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "lz4enc_core_driver.cpp"), "-o", exe])
    return exe


def _run(driver, tmp_path, records):
    src, dst = str(tmp_path / "records"), str(tmp_path / "results")
    with open(src, "wb") as fh:
        for r in records:
            fh.write(r)
    p = subprocess.run([driver, src, dst], stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    return open(dst, "rb").read()


def encode_streams(driver, tmp_path, streams):
    """-> [(block under the cap n - 1 or None = stored, block under the generous cap or None)]; the strict decoder's
    verdict is asserted here"""
    out = _run(driver, tmp_path, [b"\x01" + struct.pack("<I", len(s)) + s for s in streams])
    res, at = [], 0
    for k, s in enumerate(streams):
        pair = []
        for _ in range(2):
            c = struct.unpack_from("<I", out, at)[0]; at += 4
            pair.append(out[at:at + c] if c else None); at += c
        assert out[at] == 1, "stream %d (%d bytes): the strict decoder does not give the input back" % (k, len(s))
        at += 1
        if pair[0] is not None:
            assert len(pair[0]) <= len(s) - 1, "stream %d: %d bytes written under a cap of %d" % (k, len(pair[0]), len(s) - 1)
        res.append(tuple(pair))
    assert at == len(out)
    return res


def parse_block(block, n):
    """an LZ4 block by the format's own rules -> ([(literals, match length or None, distance)], decoded bytes); asserts the
    end rules for a stream of n bytes"""
    seqs, raw, ip = [], bytearray(), 0
    while True:
        tok = block[ip]; ip += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = block[ip]; ip += 1; lit += b
                if b != 255:
                    break
        assert ip + lit <= len(block)
        raw += block[ip:ip + lit]; ip += lit
        if ip == len(block):
            assert lit >= 1, "the last sequence holds no literal"
            assert lit >= min(5, n), "fewer than 5 literals at the end"
            seqs.append((lit, None, 0))
            break
        dist = block[ip] | (block[ip + 1] << 8); ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = block[ip]; ip += 1; ml += b
                if b != 255:
                    break
        ml += 4
        assert 1 <= dist <= len(raw), "distance %d at output %d" % (dist, len(raw))
        assert len(raw) < n - 12, "a match starts within the last 12 bytes"
        assert len(raw) + ml <= n - 5, "a match reaches into the last 5 bytes"
        for _ in range(ml):
            raw.append(raw[-dist])
        seqs.append((lit, ml, dist))
    assert len(raw) == n
    if n < 13:
        assert len(seqs) == 1, "a stream of fewer than 13 bytes is literals only"
    return seqs, bytes(raw)


def lz4_decompress(block, n):
    """lz4_decompress of cv_hostio.cpp, reached through cv_blosc_decompress: the block as the one stream of a chunk"""
    return utils_v2.blosc_decompress(B.container(n, 1, n, (1 << 5) | 0x10, [[block]]))


def _find_lib(name):
    path = ctypes.util.find_library(name)
    if not path:
        path = next((os.path.join(d, "lib%s.so" % name) for d in (os.path.join(sys.prefix, "lib"),)
                     if os.path.exists(os.path.join(d, "lib%s.so" % name))), None)
    if path:
        try:
            return ctypes.CDLL(path)
        except OSError:
            return None
    return None


_liblz4 = _find_lib("lz4")                # the reference decoder, where this machine has it (the GPU machine may not)


def check(streams, got):
    """every block written decodes to its stream: by the rules, and by lz4_decompress; -> the parses under the generous cap"""
    parses = []
    for s, (tight, loose) in zip(streams, got):
        if len(s) == 0 or len(s) > CAP:
            assert tight is None and loose is None
            parses.append(None)
            continue
        assert loose is not None
        seqs, raw = parse_block(loose, len(s))
        assert raw == s
        assert lz4_decompress(loose, len(s)) == s
        if _liblz4 is not None:
            out = ctypes.create_string_buffer(len(s))
            assert _liblz4.LZ4_decompress_safe(loose, out, len(loose), len(s)) == len(s) and out.raw == s
        # the cap only decides whether the block is kept: it is the same block, or none
        assert tight == (loose if len(loose) <= len(s) - 1 else None)
        parses.append(seqs)
    return parses


def _rand(seed, n, lo=1, hi=200):
    return bytes(np.random.RandomState(seed).randint(lo, hi, n).astype(np.uint8))


def test_every_length_to_80(driver, tmp_path):
    streams, names = [], []
    for n in range(0, 81):
        pats = {"zero": bytes(n), "one byte set": bytes(n // 2) + b"\x07" + bytes(n - n // 2 - 1) if n else b"",
                "ramp": bytes(range(n)), "random": _rand(n, n, 0, 256)}
        for p in (1, 2, 3, 4, 5, 7):
            pats["period %d" % p] = bytes(1 + i % p for i in range(n))
        for name, s in pats.items():
            assert len(s) == n
            streams.append(s); names.append("%s, %d bytes" % (name, n))
    parses = check(streams, encode_streams(driver, tmp_path, streams))
    # the runs compress as soon as the end rules allow a match: 13 bytes hold none (only position 0 may start one), 14 do
    by = dict(zip(names, parses))
    for n in (1, 12, 13):
        assert len(by["zero, %d bytes" % n]) == 1
    for n in (14, 16):
        assert len(by["zero, %d bytes" % n]) == 2
    for n in (17, 18, 80):
        for name in ("zero", "period 1", "period 2", "period 3", "period 4"):
            assert len(by["%s, %d bytes" % (name, n)]) == 2, (name, n)
    assert by["zero, 80 bytes"][0][:2] == (1, 74)


LITS = (14, 15, 16, 269, 270, 271)
MATCHES = (18, 19, 20, 273, 274, 275)


def test_length_field_boundaries(driver, tmp_path):
    streams, want = [], []
    for L in LITS:
        for M in MATCHES:
            seed = L * 1000 + M
            run = _rand(seed, L - 1) + b"\xfb" + b"\xfb" * M              # L literals, then M bytes at distance 1
            streams.append(run + b"\xfc" + _rand(seed + 1, 20)); want.append((L, M))                  # at the start
            streams.append(_rand(seed + 2, 20) + b"\xfa" * 9 + run + b"\xfc" + _rand(seed + 3, 30)); want.append((L, M))   # in the middle
            for t in (0, 4, 5, 11, 12):                                                                # the match would end in the last 5 / 12
                streams.append(run + _rand(seed + 4, t)); want.append(None)
    parses = check(streams, encode_streams(driver, tmp_path, streams))
    for s, w, seqs in zip(streams, want, parses):
        if w is not None:
            assert w in [(lit, ml) for lit, ml, _d in seqs], "wanted %r among %r" % (w, seqs)


def test_at_the_device_cap(driver, tmp_path):
    x, _y = B.candidates(64, seed=3)
    plane = x.tobytes()[2::4]                                  # a byte plane of pileup-like floats
    body = (plane * (CAP // len(plane) + 1))[:CAP - 3000] + _rand(5, 3000, 0, 256)
    streams = [body[:CAP], body[:CAP - 1], bytes(CAP), body + b"\x00"]
    got = encode_streams(driver, tmp_path, streams)
    check(streams, got)
    assert got[0][0] is not None and len(got[0][0]) < CAP // 2
    assert len(got[2][0]) < 300                                 # one run: a few hundred length bytes
    assert got[3] == (None, None)                               # one byte above the cap: not this core's


def chunk_record(arr, blocksize):
    stream = pickle.dumps(arr, pickle.HIGHEST_PROTOCOL)
    off, ln = utils_v2.find_array_payload(stream)
    assert ln == arr.nbytes
    return b"\x02" + struct.pack("<5I", arr.itemsize, blocksize, off, ln, len(stream) - off - ln) + stream, stream


def _foreign_decoders():
    """[(name, (chunk, nbytes) -> bytes)]: libblosc where this machine has it"""
    lib = _find_lib("blosc")
    if lib is None:
        return []

    def dec(chunk, nbytes):
        out = ctypes.create_string_buffer(nbytes)
        assert lib.blosc_decompress(chunk, out, ctypes.c_size_t(nbytes)) == nbytes
        return out.raw
    return [("libblosc", dec)]


@pytest.mark.parametrize("blocksize", [512, 4096, 65536])
def test_whole_chunks(driver, tmp_path, blocksize):
    xs = [B.candidates(500, seed=7)[0], synth.make_candidates(500).numpy()]
    xs = [np.ascontiguousarray(x, dtype=np.float32) for x in xs]
    recs = [chunk_record(x, blocksize) for x in xs] + [chunk_record(xs[0][:37], blocksize)]
    out = _run(driver, tmp_path, [r for r, _s in recs])
    at = 0
    for k, (_r, stream) in enumerate(recs):
        total = struct.unpack_from("<I", out, at)[0]; at += 4
        chunk = out[at:at + total]; at += total
        assert out[at] == 1, "chunk %d: the plan and the strict decoder do not give the pickle back" % k
        at += 1
        assert total, "chunk %d came back HOST" % k
        assert struct.unpack_from("<i", chunk, 12)[0] == total
        assert utils_v2.blosc_decompress(chunk) == stream
        for name, dec in _foreign_decoders():
            assert dec(chunk, len(stream)) == stream, name
        host = utils_v2.blosc_compress(stream, 4, blocksize)
        assert chunk[:12] == host[:12]                           # the same header but for the length
        print("blocksize %d chunk %d: %d bytes, the host writer %d" % (blocksize, k, total, len(host)))
    assert at == len(out)


def _host_form(x, items, blocksize):
    """cv_blosc_pack_host_form over the chunks of `items` rows of x -> [chunk or None]"""
    lib = _lib.load()
    head, tail = utils_v2.pickle_envelope((items,) + x.shape[1:], x.dtype)
    chunks = len(x) // items
    row = x[0].nbytes
    nbytes = len(head) + items * row + len(tail)
    cap = chunks * (16 + nbytes)
    out = ctypes.create_string_buffer(cap)
    off, status = (ctypes.c_int64 * (chunks + 1))(), (ctypes.c_int32 * chunks)()
    _lib.check(lib.cv_blosc_pack_host_form(x.ctypes.data_as(ctypes.c_void_p), chunks, items * row, head, len(head), tail, len(tail), 4,
                                           blocksize, out, cap, off, status))
    return [out.raw[off[c]:off[c + 1]] if status[c] == 1 else None for c in range(chunks)]


def test_the_librarys_host_form_and_the_size_condition():
    """cv_blosc_pack_host_form (what the device is held to) on make_candidates(2 000) at blocksize 65 536: every chunk is
    the pickle again, and the X blocks total at most 1.5 times cv_blosc_compress_lz4_blocks's"""
    x = np.ascontiguousarray(synth.make_candidates(2000).numpy(), dtype=np.float32)
    chunks = _host_form(x, 500, 65536)
    mine = theirs = 0
    for c, chunk in enumerate(chunks):
        stream = pickle.dumps(x[c * 500:(c + 1) * 500], pickle.HIGHEST_PROTOCOL)
        assert chunk is not None and utils_v2.blosc_decompress(chunk) == stream
        assert np.array_equal(utils_v2.unpack_array(chunk).view(np.uint32), x[c * 500:(c + 1) * 500].view(np.uint32))
        mine += len(chunk); theirs += len(utils_v2.blosc_compress(stream, 4, 65536))
    print("device layout %d bytes, host writer %d: ratio %.3f" % (mine, theirs, mine / theirs))
    assert mine <= 1.5 * theirs


def test_random_bits_do_not_shrink_and_go_to_the_host():
    x = np.random.RandomState(1).randint(0, 1 << 32, size=(8, 33, 4, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert _host_form(x, 4, 4096) == [None, None]
