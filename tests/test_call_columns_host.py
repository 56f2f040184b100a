"""callVarBam's row selection and candidate tokens in their host form (csrc/cv_callcols_core.hpp), held to the Python
definition: the filter of callVarBam.region_tensors plus utils_v2.PosBatch.from_columns (call_columns_cases.definition).
The core runs twice: in a stand-alone program built here with AddressSanitizer and UBSan
(tests/native/call_columns_driver.cpp: every output in a heap block of exactly its size; nothing is loaded into this
interpreter under a sanitizer), and as the library's cv_call_columns_host_form.  The references hold all 256 byte values
and ~20 000 random centres reach over both of their ends; ref_first is 0 and several hundred million, up to where the
coordinates take 10 digits.  The kernels run the same text and are held to it by test_gpu_call_columns.py."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from call_columns_cases import definition, random_case

HERE = os.path.dirname(os.path.abspath(__file__))

# (seed, ref_first, contig name): coordinates of 1..4, 9 / 10 (999 999 9xx -> 1 000 000 0xx) and 10 digits
CASES = [(1, 0, b"chr21"), (2, 300000000, b"c"), (3, 999997000, b"contig_0001.2|arrow_pilon|a-rather-long.name"), (4, 2100000000, b"ctgA")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("call_columns") / "call_columns_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "call_columns_driver.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed, first, ctg in CASES:
        c = random_case(seed, first, ctg=ctg)
        out.append((c, definition(*c)))
    return out


def _same(got, want, what):
    index, text, meta = got
    windex, wtext, wmeta = want
    assert np.array_equal(index, windex), what
    assert meta.shape == wmeta.shape and np.array_equal(meta, wmeta), what
    assert text == wtext, what


def test_the_definition_meets_every_case(cases):
    """the inputs are worth the name: rows dropped for each reason, short windows, every digit count"""
    for (ctg, centres, touched, ref, first), (index, text, meta) in cases:
        assert set(ref) == set(range(256))
        assert 2000 < len(index) < len(centres) - 2000
        assert (meta[:, 5] < 33).any() and (meta[:, 5] == 33).any() and meta[:, 5].min() >= 17
        ri = centres - 1 - first
        inside = (ri >= 16) & (ri < len(ref))
        centre_ok = np.array([0 <= r < len(ref) and bytes([ref[r]]).upper() in (b"A", b"C", b"G", b"T") for r in ri])
        assert (touched.astype(bool) & ~inside).any() and (touched.astype(bool) & inside & ~centre_ok).any() and (~touched.astype(bool) & inside & centre_ok).any()
        windows = text[int(meta[0, 4]):]
        assert any(b >= 0x80 for b in windows) and not any(97 <= b <= 122 for b in windows)
    digits = set()
    for _c, (_i, _t, meta) in cases:
        digits |= set(meta[:, 3].tolist())
    assert {2, 3, 4, 9, 10} <= digits


def test_the_core_under_sanitizers_is_the_definition(driver, cases, tmp_path):
    for (ctg, centres, touched, ref, first), want in cases:
        case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        with open(case, "wb") as f:
            f.write(struct.pack("<4q", len(ctg), len(centres), first, len(ref)))
            f.write(ctg + centres.astype("<i4").tobytes() + touched.tobytes() + ref)
        p = subprocess.run([driver, case, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = p.stderr.decode("utf-8", "replace")
        assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
        m = re.match(r"ok (\d+) centres, (\d+) kept, (\d+) bytes", p.stdout.decode())
        assert m, p.stdout
        n, k, nbytes = (int(g) for g in m.groups())
        raw = open(out, "rb").read()
        info = np.frombuffer(raw, dtype="<i8", count=4)
        assert info.tolist() == [k, nbytes, n, 0] and n == len(centres) and len(raw) == 32 + 56 * k + nbytes
        index = np.frombuffer(raw, dtype="<i8", count=k, offset=32)
        meta = np.frombuffer(raw, dtype="<i8", count=6 * k, offset=32 + 8 * k).reshape(k, 6)
        _same((index, raw[32 + 56 * k:], meta), want, "ref_first %d" % first)


def host_form(ctg, centres, touched, ref, first, slack=0):
    """cv_call_columns_host_form -> (index, text, meta) and what lies behind them"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    n = len(centres)
    c32 = np.ascontiguousarray(centres, dtype=np.int32)
    t8 = np.ascontiguousarray(touched, dtype=np.uint8)
    rf = np.frombuffer(ref, dtype=np.uint8)
    cap = len(ctg) + 43 * n
    index = np.full(n + 1, -7, dtype=np.int64); meta = np.full((n + 1, 6), -7, dtype=np.int64)
    text = np.full(cap + 1, 0xA5, dtype=np.uint8); info = np.zeros(4, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(lib.cv_call_columns_host_form(ctg, len(ctg), p(c32), p(t8), n, p(rf), first, len(ref), p(index), p(meta), p(text), cap, p(info)))
    k, nbytes = int(info[0]), int(info[1])
    assert info.tolist() == [k, nbytes, n, 0]
    assert (index[k:] == -7).all() and (meta[k:] == -7).all() and (text[nbytes:] == 0xA5).all()        # nothing behind the rows
    return index[:k].copy(), text[:nbytes].tobytes(), meta[:k].copy()


def test_the_librarys_host_form_is_the_definition(cases):
    for c, want in cases:
        _same(host_form(*c), want, "ref_first %d" % c[4])


def test_degenerate_sizes_and_refusals():
    from clairvoyante_amd import _lib
    lib = _lib.load()
    ref = b"ACGT" * 20
    none = np.zeros(0, dtype=np.int64)
    _same(host_form(b"ctgA", none, none, ref, 0), definition(b"ctgA", none, none, ref, 0), "no centre")
    centres = np.arange(1, 90, dtype=np.int64)
    for touched, r in ((np.zeros(89, np.uint8), ref), (np.ones(89, np.uint8), b"N" * 80)):       # nothing touched / no ACGT centre
        got = host_form(b"ctgA", centres, touched, r, 0)
        assert len(got[0]) == 0 and got[1] == b"ctgA"
        _same(got, definition(b"ctgA", centres, touched, r, 0), "nothing kept")
    need = ctypes.c_int64(-1)
    assert lib.cv_call_columns_workspace(-1, ctypes.byref(need)) == 1 and lib.cv_call_columns_workspace(5, None) == 1
    assert lib.cv_call_columns_workspace((1 << 27) + 1, ctypes.byref(need)) == 1
    c32 = np.arange(17, 21, dtype=np.int32); t8 = np.ones(4, np.uint8); rf = np.frombuffer(ref, dtype=np.uint8)
    index = np.zeros(4, np.int64); meta = np.zeros((4, 6), np.int64); text = np.zeros(256, np.uint8); info = np.zeros(4, np.int64)
    p = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    call = lambda **kw: lib.cv_call_columns_host_form(*[kw.get(k, v) for k, v in (
        ("ctg", b"ctgA"), ("ctg_len", 4), ("centres", p(c32)), ("touched", p(t8)), ("n", 4), ("ref", p(rf)), ("first", 0), ("ref_len", len(ref)),
        ("index", p(index)), ("meta", p(meta)), ("text", p(text)), ("cap", 4 + 43 * 4), ("info", p(info)))])
    assert call() == 0 and info.tolist()[0] == 4
    for bad in (dict(centres=None), dict(touched=None), dict(ref=None), dict(index=None), dict(meta=None), dict(text=None), dict(info=None),
                dict(centres=p(c32, 2)), dict(index=p(index, 4)), dict(meta=p(meta, 4)), dict(info=p(info, 4)),
                dict(cap=4 + 43 * 4 - 1), dict(first=-1), dict(n=-1), dict(ctg_len=1025), dict(ref_len=-1)):
        assert call(**bad) == 1, bad
        assert b"cv_call_columns_host_form" in lib.cv_last_error()
