"""PairWithNonVariants' switch and the host form of the gather its device route uses, without a GPU: CV_PAIR takes "host" and
"device" and nothing else, "device" without a GPU is the loop and counts() says so; cv_items_copy_host_form writes what a
Python restatement writes, with the room's unwritten bytes left alone; and the same core in a stand-alone program built here
with AddressSanitizer and UBSan (tests/native/items_copy_driver.cpp: the text, the arrays and the room in heap blocks of
exactly their bytes; nothing is loaded into this interpreter under a sanitizer)."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import items_copy_cases as ic
import pair_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))


def _files(tmp_path):
    var, can, bed = pc.fixture()
    return (pc.write(tmp_path / "var", var), pc.write(tmp_path / "can", can), pc.write(tmp_path / "r.bed", bed))


def test_an_unknown_value_raises(tmp_path, monkeypatch):
    from clairvoyante_amd import PairWithNonVariants as P
    var, can, bed = _files(tmp_path)
    for bad in ("gpu", "Device", "1"):
        monkeypatch.setenv("CV_PAIR", bad)
        with pytest.raises(ValueError, match="CV_PAIR must be 'host' or 'device'"):
            P.Pair(pc.args_of(var, can, bed, str(tmp_path / "out.gz")))
    assert not os.path.exists(str(tmp_path / "out.gz"))


def test_without_a_gpu_the_switch_gives_the_loop_and_counts_say_so(tmp_path, monkeypatch):
    from clairvoyante_amd import PairWithNonVariants as P
    from clairvoyante_amd import utils_v2
    var, can, bed = _files(tmp_path)
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    want = None
    for k, value in enumerate((None, "host", "device", "")):
        if value is None:
            monkeypatch.delenv("CV_PAIR", raising=False)
        else:
            monkeypatch.setenv("CV_PAIR", value)
        assert P.route() == "host"
        P.counts(reset=True)
        out = str(tmp_path / ("out%d.gz" % k))
        got, msgs, raised = pc.run(P.Pair, pc.args_of(var, can, bed, out))
        assert raised is None
        assert P.counts() == {"device_calls": 0, "host_calls": 1, "handed_over_calls": 0, "device_lines_bed": 0, "device_lines_var": 0,
                              "device_lines_can": 0}
        if want is None:
            want = (got, msgs, pc.inflated(out))
            assert pc.run(P.Pair_host, pc.args_of(var, can, bed, str(tmp_path / "loop.gz")), pc.SEED)[0] == got
            assert pc.inflated(str(tmp_path / "loop.gz")) == want[2] and 0 < got["o2"] < got["c"]
        assert (got, msgs, pc.inflated(out)) == want
    assert P.counts(reset=True)["host_calls"] == 1 and P.counts()["host_calls"] == 0


def _host_form(text, off, kept_len, out_cap, canary=64):
    """cv_items_copy_host_form over numpy copies, the room between two canaries -> (room, counts)"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    t = np.frombuffer(text, dtype=np.uint8).copy()
    off, kept_len = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(kept_len, dtype=np.int64)
    room = np.full(out_cap + 2 * canary, ic.FILL, dtype=np.uint8)
    counts = np.full(4, -1, dtype=np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None
    _lib.check(lib.cv_items_copy_host_form(p(t), len(t), len(off), p(off), p(kept_len), ctypes.c_void_p(room.ctypes.data + canary), out_cap,
                                           p(counts)))
    assert (room[:canary] == ic.FILL).all() and (room[canary + out_cap:] == ic.FILL).all()
    return room[canary:canary + out_cap].tobytes(), counts.tolist()


@pytest.mark.parametrize("name", sorted(ic.cases()))
def test_the_host_form_is_the_restatement(name):
    text, off, kept_len, out_cap = ic.cases()[name]
    want = ic.restated(text, off, kept_len, out_cap)
    assert _host_form(text, off, kept_len, out_cap) == want
    if name == "one byte short":
        last = int(kept_len[-1])
        assert want[0][-(last - 1):] == bytes([ic.FILL]) * (last - 1) and want[1][2] == out_cap + 1


def test_the_host_form_over_random_rows():
    rng = np.random.RandomState(23)
    for _ in range(40):
        n = int(rng.randint(0, 60))
        lengths = rng.randint(1, 400, n).astype(np.int64)
        text, off = ic.lines_text(lengths, seed=int(rng.randint(1 << 30)), gap=int(rng.randint(0, 20)))
        kept_len = lengths * (rng.randint(0, 2, n))
        order = rng.permutation(n)                           # the rows need not be in the text's order
        off, kept_len = off[order], kept_len[order]
        out_cap = max(int(kept_len.sum()) - int(rng.randint(0, 2)) * int(rng.randint(0, 300)), 0)
        assert _host_form(text, off, kept_len, out_cap) == ic.restated(text, off, kept_len, out_cap)


def test_the_host_form_refuses_what_the_device_entry_refuses():
    from clairvoyante_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64()
    assert lib.cv_items_copy_workspace(-1, ctypes.byref(need)) == 1 and b"cv_items_copy_workspace" in lib.cv_last_error()
    counts = np.zeros(4, dtype=np.int64)
    c = ctypes.c_void_p(counts.ctypes.data)
    assert lib.cv_items_copy_host_form(None, 0, 0, None, None, None, 0, None) == 1 and b"null argument" in lib.cv_last_error()
    assert lib.cv_items_copy_host_form(None, 4, 0, None, None, None, 0, c) == 1 and b"null argument" in lib.cv_last_error()
    assert lib.cv_items_copy_host_form(None, 0, 1, None, None, None, 0, c) == 1
    assert lib.cv_items_copy_host_form(None, 0, 0, None, None, None, -1, c) == 1 and b"out of range" in lib.cv_last_error()
    assert lib.cv_items_copy_host_form(None, 0, 0, None, None, None, 0, ctypes.c_void_p(counts.ctypes.data + 4)) == 1
    assert b"8-byte aligned" in lib.cv_last_error()
    assert lib.cv_items_copy_host_form(None, 0, 0, None, None, None, 0, c) == 0 and counts.tolist() == [0, 0, 0, 0]
    # lengths no caller should pass: nothing is written, nothing outside the room is touched
    text = b"0123456789\n"
    off = np.array([0, 5, -3, 2, 0], dtype=np.int64)
    kept = np.array([-4, 1 << 62, 3, 20, 11], dtype=np.int64)
    room, _counts = _host_form(text, off, kept, 16)
    assert room == bytes([ic.FILL]) * 16


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("items_copy") / "items_copy_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "items_copy_driver.cpp"),
                           "-o", exe])
    return exe


def test_the_core_under_sanitizers_is_the_restatement(driver, tmp_path):
    cases = dict(ic.cases())
    cases["wrong lengths"] = (b"0123456789\n", np.array([0, 5, -3, 2, 0], dtype=np.int64), np.array([-4, 1 << 62, 3, 20, 11], dtype=np.int64), 16)
    for k, name in enumerate(sorted(cases)):
        text, off, kept_len, out_cap = cases[name]
        src, dst = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        with open(src, "wb") as f:
            f.write(struct.pack("<q", len(text)) + text + struct.pack("<q", len(off)) + off.astype("<i8").tobytes() +
                    kept_len.astype("<i8").tobytes() + struct.pack("<q", out_cap))
        p = subprocess.run([driver, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = p.stderr.decode("utf-8", "replace")
        assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, (name, err[-4000:])
        raw = open(dst, "rb").read()
        got = (raw[32:], list(struct.unpack("<4q", raw[:32])))
        if name == "wrong lengths":
            assert got[0] == bytes([ic.FILL]) * 16
        else:
            assert got == ic.restated(text, off, kept_len, out_cap), name
