"""The three DEFLATE decoders on the host -- csrc/cv_inflate.cpp through cv_inflate_raw / cv_inflate_stream, and the host
forms of csrc/cv_inflate_core.hpp and csrc/cv_gzip_core.hpp (the text the GPU runs) through cv_gzip_chunk_host /
cv_gzip_header_at and the two stand-alone sanitizer drivers -- over streams zlib does not write: the members of
tests/foreign_cases.py, made bit by bit, and what libdeflate wrote.  zlib's inflate is the judge: its bytes for the valid
members, a refusal for the invalid ones."""
import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_writer as W
import foreign_cases as F
import gzip_cases as G
import test_bgzf_sanitized as BS
import test_gzip_core_host as GH

CANARY, GUARD = 0x5A, 64
HERE = os.path.dirname(os.path.abspath(__file__))
bgzf_driver = BS.driver                                      # the fixtures that build the two drivers with
gzip_driver = GH.driver                                      # -fsanitize=address,undefined


@pytest.fixture(scope="module")
def lib():
    from clairvoyante_amd import _lib
    return _lib.load()


def everything():
    return F.valid() + F.libdeflate_members()


def _src(data):
    return np.frombuffer(data + b"\xa5" * 8, dtype=np.uint8).copy()          # 8 readable bytes behind the stream


def inflate_raw(lib, data, size):
    src, dst = _src(data), np.full(GUARD + size + GUARD, CANARY, dtype=np.uint8)
    rc = lib.cv_inflate_raw(ctypes.c_void_p(src.ctypes.data), len(data), ctypes.c_void_p(dst.ctypes.data + GUARD), size)
    intact = bool(np.all(dst[:GUARD] == CANARY) and np.all(dst[GUARD + size:] == CANARY))
    return rc, dst[GUARD:GUARD + size].tobytes(), intact


def inflate_stream(lib, data, size, want):
    """block by block -> (bytes or None, calls, canaries intact)"""
    src, dst = _src(data), np.full(GUARD + size + GUARD, CANARY, dtype=np.uint8)
    bitpos, final, have, calls = ctypes.c_int64(0), ctypes.c_int32(0), 0, 0
    while not final.value:
        got = lib.cv_inflate_stream(ctypes.c_void_p(src.ctypes.data), len(data), ctypes.byref(bitpos), ctypes.c_void_p(dst.ctypes.data + GUARD),
                                    have, size, want, ctypes.byref(final))
        calls += 1
        if got < 0:
            have = None
            break
        assert got > 0 or final.value, "no progress"
        have += got
    intact = bool(np.all(dst[:GUARD] == CANARY) and np.all(dst[GUARD + size:] == CANARY))
    return (None if have is None else dst[GUARD:GUARD + have].tobytes()), calls, intact


def chunk(lib, data, start, end, hist):
    """-> (how, symbols or None, the bit it ended at); the symbols between canaries"""
    src = _src(data)
    p = ctypes.c_void_p(src.ctypes.data)
    count, ended = ctypes.c_int64(), ctypes.c_int64()
    how = lib.cv_gzip_chunk_host(p, len(data), start, end, None, 0, hist, ctypes.byref(count), ctypes.byref(ended))
    if how == G.BAD:
        return how, None, ended.value
    sym = np.full(GUARD + count.value + GUARD, CANARY * 257, dtype=np.uint16)
    again = ctypes.c_int64()
    how2 = lib.cv_gzip_chunk_host(p, len(data), start, end, ctypes.c_void_p(sym.ctypes.data + 2 * GUARD), count.value, hist, ctypes.byref(again),
                                  ctypes.byref(ended))
    assert (how2, again.value) == (how, count.value)
    assert np.all(sym[:GUARD] == CANARY * 257) and np.all(sym[GUARD + count.value:] == CANARY * 257)
    return how, sym[GUARD:GUARD + count.value], ended.value


# ---- valid members -------------------------------------------------------------------------------------------------------
def test_the_corpus_holds_what_it_is_named_for():
    """(the constructs are asserted where foreign_cases builds them; here: the sizes that go into the records)"""
    valid, invalid = F.valid(), F.invalid()
    assert len(valid) >= 26 and len(invalid) >= 20 and len(F.libdeflate_members()) == 8
    blocks = sum(len(m.blocks) for m in valid)
    print("valid members: %d (%d blocks, %d bytes of DEFLATE, %d bytes inflated); invalid: %d" %
          (len(valid), blocks, sum(len(m.data) for m in valid), sum(len(m.raw) for m in valid), len(invalid)))
    many = dict((m.name, m) for m in valid)["many_small_dynamic_blocks"]
    assert len(many.blocks) >= 300 and all(b.kind == W.DYNAMIC for b in many.blocks)


def test_inflate_raw_gives_zlibs_bytes(lib):
    for m in everything():
        rc, out, intact = inflate_raw(lib, m.data, len(m.raw))
        assert intact, m.name
        assert rc == len(m.raw) and out == m.raw, m.name


@pytest.mark.parametrize("want", [1, 4096])
def test_inflate_stream_gives_zlibs_bytes(lib, want):
    for m in everything():
        out, calls, intact = inflate_stream(lib, m.data, len(m.raw), want)
        assert intact and out == m.raw, m.name
        if m.blocks is not None and want == 1:                # a call per block that gave bytes, and one for what is left
            assert calls >= sum(1 for k, b in enumerate(m.blocks[:-1]) if m.blocks[k + 1].out_at > b.out_at)


def test_chunk_host_gives_zlibs_bytes_in_one_chunk(lib):
    for m in everything():
        how, sym, ended = chunk(lib, m.data, 0, -1, 0)
        assert how == G.FINAL and (ended + 7) // 8 == len(m.data), m.name
        assert not np.any(sym & G.MARK) and G.resolve(sym, b"") == m.raw, m.name


def test_chunk_host_cut_at_every_block_start(lib):
    """every block a chunk of its own, its window unknown: each LANDS on the next block's first bit, and the markers
    resolve against zlib's bytes in front"""
    cuts = 0
    for m in F.valid():
        out = b""
        for k, b in enumerate(m.blocks):
            last = k == len(m.blocks) - 1
            assert len(out) == b.out_at
            how, sym, ended = chunk(lib, m.data, b.bit, -1 if last else m.blocks[k + 1].bit, min(b.out_at, 32768))
            assert how == (G.FINAL if last else G.LANDED), "%s block %d: %d" % (m.name, k, how)
            assert last or ended == m.blocks[k + 1].bit
            out += G.resolve(sym, m.raw[max(0, b.out_at - 32768):b.out_at])
            cuts += 1
        assert out == m.raw, m.name
    assert cuts >= 350


def test_header_at_finds_exactly_the_complete_non_final_dynamic_headers(lib):
    seen = {True: 0, False: 0}
    for m in F.valid():
        src = _src(m.data)
        for b in m.blocks:
            want = b.kind == W.DYNAMIC and not b.final and b.complete
            assert lib.cv_gzip_header_at(ctypes.c_void_p(src.ctypes.data), len(m.data), b.bit) == int(want), (m.name, b.bit)
            seen[want] += 1
    data, _text, blocks = F.writer_gzip()
    src = _src(data)
    for k, (bit, _at, complete) in enumerate(blocks):
        want = complete and k < len(blocks) - 1
        assert lib.cv_gzip_header_at(ctypes.c_void_p(src.ctypes.data), len(data) - 8, bit) == int(want), k
        seen[want] += 1
    assert seen[True] >= 300 and seen[False] >= 30


# ---- invalid members -----------------------------------------------------------------------------------------------------
def test_invalid_members_are_refused_by_every_entry_point(lib):
    for name, data, isize in F.invalid():
        rc, _out, intact = inflate_raw(lib, data, isize)
        assert rc == -1 and intact, name
        for want in (1, 4096):
            out, _calls, intact = inflate_stream(lib, data, isize + 300, want)
            assert out is None and intact, name
        how, _sym, _ended = chunk(lib, data, 0, -1, 0)
        assert how == G.BAD, name
        # ... and with room for whatever it might make: the refusal is the header's or the token's, not the buffer's
        src = _src(data)
        sym = np.full(GUARD + 70000, CANARY * 257, dtype=np.uint16)
        count, ended = ctypes.c_int64(), ctypes.c_int64()
        how = lib.cv_gzip_chunk_host(ctypes.c_void_p(src.ctypes.data), len(data), 0, -1, ctypes.c_void_p(sym.ctypes.data), 70000, 0,
                                     ctypes.byref(count), ctypes.byref(ended))
        assert how == G.BAD and np.all(sym[70000:] == CANARY * 257), name
        assert lib.cv_gzip_header_at(ctypes.c_void_p(src.ctypes.data), len(data), 0) == 0, name


# ---- the host forms under AddressSanitizer / UBSan -------------------------------------------------------------------------
def test_the_bgzf_core_under_sanitizers(bgzf_driver, tmp_path):
    members = everything()
    got = BS.run(bgzf_driver, tmp_path, [(m.data, len(m.raw), zlib.crc32(m.raw)) for m in members])
    for m, g in zip(members, got):
        assert g is not None, "%s came back HOST" % m.name
        assert g == m.raw, m.name
    bad = F.invalid()
    got = BS.run(bgzf_driver, tmp_path, [(data, isize, 0) for _n, data, isize in bad] +
                 [(data, isize + 300, 0) for _n, data, isize in bad])
    assert got == [None] * (2 * len(bad))


def _pipeline(gzip_driver, tmp_path, data, raw, spacing):
    fn = str(tmp_path / "m.gz")
    with open(fn, "wb") as fh:
        fh.write(G.member(data, raw))
    rc, out, err = GH._pipeline(gzip_driver, fn, 10, spacing)
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    return rc, out, err


def test_the_gzip_core_under_sanitizers(gzip_driver, tmp_path):
    """finder, chunks with an unknown window, chain rule and resolution over every member as a gzip file (guesses every
    256 bytes: the members are short)"""
    for m in everything():
        rc, out, err = _pipeline(gzip_driver, tmp_path, m.data, m.raw, 256)
        assert rc == 0 and out == m.raw, (m.name, rc, err)
        if m.name == "many_small_dynamic_blocks":             # blocks of at most 200 bytes, complete codes: a header, and so
            chunks = int(dict(kv.split("=") for kv in err.split())["chunks"])      # a cut, in every stretch of 256 bytes
            assert chunks >= len(m.data) // 256
    for name, data, isize in F.invalid():
        rc, _out, _err = _pipeline(gzip_driver, tmp_path, data, b"\0" * isize, 256)
        assert rc == 2, name
    data, text, _blocks = F.writer_gzip()
    fn = str(tmp_path / "w.gz")
    with open(fn, "wb") as fh:
        fh.write(data)
    rc, out, err = GH._pipeline(gzip_driver, fn, 10, 1024)
    assert rc == 0 and out == text and "ERROR" not in err and "runtime error" not in err, err[-3000:]


@pytest.fixture(scope="module")
def tables_driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    exe = str(tmp_path_factory.mktemp("inflate_tables") / "inflate_tables_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-Wall", "-Werror", os.path.join(HERE, "native", "inflate_tables_driver.cpp"), "-o", exe])
    return exe


def test_the_first_level_tables_hold_exactly_the_short_codes(tables_driver, tmp_path):
    """cvi::fill against a table written down here: entry i of the 10-bit literal/length table and of the 8-bit distance
    table is (symbol << 4) | length of the code that the low bits of i spell, when that code has at most 10 / 8 bits, and 0
    ("walk the canonical code") otherwise; and cvi::symbol gives every code's symbol and length, whatever bits follow it --
    over the codes of every dynamic block of the corpus, the fixed code, and two that bookkeeping must refuse"""
    LBITS, DBITS = 10, 8
    codes = [(tuple(W.FIXED_LL), tuple(W.FIXED_DL))]
    for m in F.valid():
        for b in m.blocks:
            if b.kind == W.DYNAMIC:
                codes.append((tuple(b.ll) + (0,) * (288 - len(b.ll)), tuple(b.dl) + (0,) * (32 - len(b.dl))))
    codes = sorted(set(codes))
    refused = [(tuple([1] + list(W.FIXED_LL[1:])), tuple(W.FIXED_DL)), (tuple(W.FIXED_LL), (2, 2) + (0,) * 30)]
    with open(str(tmp_path / "codes"), "wb") as fh:
        for ll, dl in codes + refused:
            fh.write(bytes(ll) + bytes(dl))
    p = subprocess.run([tables_driver, str(tmp_path / "codes"), str(tmp_path / "tables")], stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    out, at = open(str(tmp_path / "tables"), "rb").read(), 0
    depths = set()
    for ll, dl in codes:
        assert out[at] == 1; at += 1
        for lens, tbits in ((ll, LBITS), (dl, DBITS)):
            want = np.zeros(1 << tbits, dtype=np.uint16)
            for s, (rev, l) in W.canonical(list(lens)).items():
                if l <= tbits:
                    want[rev::1 << l] = (s << 4) | l
            got = np.frombuffer(out, dtype=np.uint16, count=1 << tbits, offset=at); at += 2 << tbits
            assert np.array_equal(got, want)
        for which, lens in enumerate((ll, dl)):
            for s, l in enumerate(lens):
                if l:
                    depths.add((which, l))
                    for _junk in range(2):
                        assert struct.unpack_from("<hB", out, at) == (s, l); at += 3
    assert out[at:] == b"\0\0"
    assert depths >= set((0, l) for l in range(1, 16)) | set((1, l) for l in range(1, 16))


# ---- libdeflate ----------------------------------------------------------------------------------------------------------
def test_the_committed_fixtures_are_what_libdeflate_writes():
    import make_foreign_fixtures as M
    ld = M.load()
    if ld is None:
        pytest.skip("libdeflate is not installed here: the committed fixtures stand")
    made = M.generate(ld)
    assert sorted(made) == sorted(os.listdir(F.FIXTURES))
    for name, data in made.items():
        assert data == F.fixture(name), name
    sizes = [len(d) for d in made.values()]
    assert max(sizes) <= 540000 and sum(sizes) < 700000


def test_the_libdeflate_files_inflate(lib):
    """the gzip files as one chunk and streamed; the BAM's members one by one"""
    import textparse_cases as T
    import bam_device_cases as C
    text = T.volume_text(300)
    for level in (6, 12):
        data = F.fixture("volume300_level%d.gz" % level)
        assert zlib.decompress(data, 31) == text
        first = G.header_end(data)
        body = data[first:len(data) - 8]
        how, sym, _ended = chunk(lib, body, 0, -1, 0)
        assert how == G.FINAL and G.resolve(sym, b"") == text
        out, calls, intact = inflate_stream(lib, body, len(text), 65536)
        assert out == text and intact and calls > 3
    bam = os.path.join(F.FIXTURES, "noisy_libdeflate.bam")
    blob = open(bam, "rb").read()
    want = C.inflated(bam)
    got = b""
    for off, bsize, _at, isize in C.members(bam):
        rc, out, intact = inflate_raw(lib, blob[off + 18:off + bsize - 8], isize)
        assert rc == isize and intact
        got += out
    assert got == want and want[:4] == b"BAM\1" and len(C.members(bam)) >= 5
