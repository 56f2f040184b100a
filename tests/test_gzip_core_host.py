"""The decode core of the ordinary-gzip reader (csrc/cv_gzip_core.hpp) in its host form, before any of it meets a GPU:
through the library's host entry points against zlib, and -- built here with AddressSanitizer and UBSan from
tests/native/gzip_core_driver.cpp -- the whole scheme over the corpus and the decoy file, and the core over a few
thousand damaged streams."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import gzip_cases as G
import textparse_cases as T

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the sanitizer build's own recipe (the Makefile of tests/native is another suite's)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    out = str(tmp_path_factory.mktemp("gzip_driver") / "gzip_core_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(HERE, "native", "gzip_core_driver.cpp"), "-o", out, "-lz"], check=True)
    return out


def _env():
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def _write(path, data):
    with open(str(path), "wb") as fh:
        fh.write(data)
    return str(path)


def _chunk(lib, a, n, start, end, hist, write=True):
    count, ended = ctypes.c_int64(), ctypes.c_int64()
    src = ctypes.c_void_p(a.ctypes.data)
    how = lib.cv_gzip_chunk_host(src, n, start, end, None, 0, hist, ctypes.byref(count), ctypes.byref(ended))
    if how == G.BAD or not write:
        return how, count.value, ended.value, None
    sym = np.full(count.value + 16, 0x5A5A, dtype=np.uint16)
    again = ctypes.c_int64()
    how2 = lib.cv_gzip_chunk_host(src, n, start, end, sym.ctypes.data_as(ctypes.c_void_p), count.value, hist, ctypes.byref(again), ctypes.byref(ended))
    assert (how2, again.value) == (how, count.value) and np.all(sym[count.value:] == 0x5A5A)
    return how, count.value, ended.value, sym[:count.value]


@pytest.mark.parametrize("name", sorted(G.kernel_corpus()))
def test_a_whole_stream_as_one_chunk_against_zlib(name):
    from clairvoyante_amd import _lib
    lib = _lib.load()
    data, text, _f = G.kernel_corpus()[name]
    a, first = np.frombuffer(data, dtype=np.uint8), G.header_end(data)
    how, count, ended, sym = _chunk(lib, a, len(a) - 8, first * 8, -1, 0)
    assert how == G.FINAL and count == len(text) and (ended + 7) // 8 == len(a) - 8
    assert not np.any(sym & G.MARK) and G.resolve(sym, b"") == text


def test_header_test_and_chain_by_hand():
    """the headers the test finds in the first 300 000 bits of a file: every chunk between two of them lands exactly on
    the next, and the symbols resolve to zlib's bytes; an end that is no block start (one bit off) is passed over"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    data, text, _f = G.kernel_corpus()["level6_mem4"]
    a, first = np.frombuffer(data, dtype=np.uint8), G.header_end(data)
    n = len(a) - 8
    src = ctypes.c_void_p(a.ctypes.data)
    hits = [b for b in range(first * 8, first * 8 + 300000) if lib.cv_gzip_header_at(src, n, b)]
    assert len(hits) >= 10 and hits[0] == first * 8
    out = b""
    for k in range(len(hits) - 1):
        how, count, ended, sym = _chunk(lib, a, n, hits[k], hits[k + 1], 0 if k == 0 else 32768)
        assert (how, ended) == (G.LANDED, hits[k + 1])
        assert k == 0 or np.any(sym & G.MARK)
        out += G.resolve(sym, out[-32768:])
    assert out == text[:len(out)] and len(out) > 100000
    how, _count, ended, _sym = _chunk(lib, a, n, hits[2], hits[3] + 1, 32768, write=False)
    assert how == G.PASSED and ended > hits[3] + 1
    assert lib.cv_gzip_header_at(src, n, hits[3] + 1) == 0 and lib.cv_gzip_header_at(src, n, n * 8 - 2) == 0
    # a match that reaches in front of the stream's start
    how, _c, _e, _s = _chunk(lib, a, n, hits[2], hits[3], 0, write=False)
    assert how == G.BAD
    # a chunk that is cut off
    how, _c, _e, _s = _chunk(lib, a, (hits[3] >> 3) - 50, hits[2], -1, 32768, write=False)
    assert how == G.BAD


def _pipeline(driver, fn, first, spacing):
    p = subprocess.run([driver, "pipeline", fn, str(first), str(spacing)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=_env())
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("name", sorted(G.kernel_corpus()))
def test_the_scheme_under_sanitizers_against_zlib(driver, tmp_path, name):
    data, text, _f = G.kernel_corpus()[name]
    rc, out, err = _pipeline(driver, _write(tmp_path / "c.gz", data), G.header_end(data), 4096)
    assert rc == 0 and "ERROR" not in err and "runtime error" not in err, err
    assert out == text
    stats = dict(kv.split("=") for kv in err.split())
    assert int(stats["decoys"]) == 0


def test_the_chain_rule_rejects_the_decoys(driver, tmp_path):
    data, payload = G.decoy(T.volume_text(300))
    rc, out, err = _pipeline(driver, _write(tmp_path / "d.gz", data), G.header_end(data), 4096)
    assert rc == 0 and "ERROR" not in err and "runtime error" not in err, err
    assert out == payload == zlib.decompress(data, 31)
    stats = dict(kv.split("=") for kv in err.split())
    assert int(stats["decoys"]) >= 3                          # valid headers were found where no block starts, and dropped


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_damaged_streams_under_sanitizers(driver, tmp_path, seed):
    text = T.volume_text(300)[:60000]
    data = G.deflate(text, 6, 3)
    p = subprocess.run([driver, "fuzz", _write(tmp_path / "f.gz", data), str(G.header_end(data)), str(seed), "1200"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=_env())
    err = p.stderr.decode()
    assert p.returncode == 0 and "ERROR" not in err and "runtime error" not in err, err
    accepted = int(err.split("accepted=")[1].split()[0])
    print(err.strip())
    assert 0 < accepted < 1200
