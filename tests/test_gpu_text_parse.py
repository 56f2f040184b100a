"""The text-tensor reader on the device (csrc/cv_textparse.hip, utils_v2.GetTensorDevice, callVar's choice of reader)
against the host reader cv_parse_tensor_text with one thread -- itself pinned to the reference's GetTensor by
tests/golden/gettensor_{a,b}.npz.  Every comparison is bit for bit; there is no tolerance anywhere."""
import ctypes
import gzip
import os
import re
import time
import types

import numpy as np
import pytest

import common
import textparse_cases as T

pytestmark = pytest.mark.gpu


def prepare(text, max_lines, offset=0):
    """the buffers of one cv_parse_tensor_text_dev call, `text` placed `offset` bytes into its device buffer"""
    import torch
    from clairvoyante_amd import _lib
    need = ctypes.c_int64()
    _lib.check(_lib.load().cv_parse_tensor_text_dev_workspace(len(text), max_lines, ctypes.byref(need)))
    cap = max(max_lines, 1)
    buf = torch.zeros(offset + len(text) + 64, dtype=torch.uint8, device="cuda")
    if len(text):
        buf[offset:offset + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    d = {"x": torch.full((cap, T.NV), float("nan"), device="cuda"), "meta": torch.full((cap, 6), -1, dtype=torch.int64, device="cuda"),
         "status": torch.full((cap,), 255, dtype=torch.uint8, device="cuda"), "info": torch.full((4,), -1, dtype=torch.int64, device="cuda"),
         "ws": torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda"), "buf": buf, "offset": offset, "len": len(text),
         "max_lines": max_lines}
    torch.cuda.synchronize()
    return d


def launch(d, stream=None):
    """enqueues the call on `stream` (default: the current one); d["host_seconds"] = host time of the call"""
    import torch
    from clairvoyante_amd import _lib
    st = stream if stream is not None else torch.cuda.current_stream()
    t0 = time.perf_counter()
    _lib.check(_lib.load().cv_parse_tensor_text_dev(
        ctypes.c_void_p(d["buf"].data_ptr() + d["offset"]), d["len"], d["max_lines"], ctypes.c_void_p(d["x"].data_ptr()),
        ctypes.c_void_p(d["meta"].data_ptr()), ctypes.c_void_p(d["status"].data_ptr()), ctypes.c_void_p(d["info"].data_ptr()),
        ctypes.c_void_p(d["ws"].data_ptr()), d["ws"].numel(), ctypes.c_void_p(st.cuda_stream)))
    d["host_seconds"] = time.perf_counter() - t0
    return d


def dev_parse(text, max_lines, offset=0):
    """cv_parse_tensor_text_dev over `text` -> dict of host arrays"""
    import torch
    d = launch(prepare(text, max_lines, offset))
    torch.cuda.synchronize()
    return to_host(d)


def to_host(d):
    info = d["info"].cpu().numpy()
    lines = int(info[1])
    return {"info": info, "status": d["status"].cpu().numpy()[:lines], "meta": d["meta"].cpu().numpy()[:lines],
            "x": d["x"].cpu().numpy()[:lines]}


def same_as_host(r, text, expect_host=0):
    """the ROW slots of a device result are the host's rows of the bytes it consumed"""
    consumed = int(r["info"][0])
    hc, _bad, hx, hmeta = T.host_parse(text[:consumed])
    rows = r["status"] == T.ROW
    assert int(r["info"][3]) == expect_host == int(np.count_nonzero(r["status"] == T.HOST))
    assert int(r["info"][2]) == int(np.count_nonzero(rows))
    assert set(np.unique(r["status"])) <= {T.SKIP, T.ROW, T.HOST}
    if expect_host == 0:
        assert hc == consumed and int(r["info"][2]) == hx.shape[0]
        assert np.array_equal(r["x"][rows].view(np.uint32), hx.view(np.uint32))
        assert np.array_equal(r["meta"][rows], hmeta)


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("offset", [0, 1, 15])
def test_reference_goldens_through_the_abi(which, offset):
    text = T.golden_text(which)
    d = np.load(os.path.join(T.GOLD, "gettensor_%s.npz" % which), allow_pickle=True)
    r = dev_parse(text, 1000, offset=offset)
    assert int(r["info"][0]) == len(text) and int(r["info"][1]) == text.count(b"\n")
    same_as_host(r, text, expect_host=0)
    rows = r["status"] == T.ROW
    assert np.array_equal(r["x"][rows].view(np.uint32), np.ascontiguousarray(d["X"], dtype=np.float32).reshape(-1, T.NV).view(np.uint32))
    pos = [b":".join(text[m[2 * k]:m[2 * k] + m[2 * k + 1]] for k in range(3)) for m in r["meta"][rows]]
    assert [p.decode().rsplit(":", 1)[0] + ":" + p.decode().rsplit(":", 1)[1].upper() for p in pos] == [str(p) for p in d["pos"]]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("textparse_gpu")
    out = {}
    for name, text in (("golden_a", T.golden_text("a")), ("golden_b", T.golden_text("b")), ("golden_a_nonl", T.golden_text("a").rstrip(b"\n")),
                       ("off_format", T.off_format_text()[0]), ("volume", T.volume_text()), ("blank_then_rows", T.blank_then_rows_text())):
        out[name] = str(d / (name + ".txt"))
        open(out[name], "wb").write(text)
    for w in "ab":
        out["golden_%s_gz" % w] = os.path.join(T.GOLD, "gettensor_%s.txt.gz" % w)
    return out


def _bad_reported(capsys):
    return sum(int(k) for k in re.findall(r"UnpackATensorRecord Failure \((\d+) malformed", capsys.readouterr().err))


def _same_batches(fn, num, monkeypatch, capsys, slab=None):
    from clairvoyante_amd import utils_v2
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    capsys.readouterr()
    want = T.collect(utils_v2.GetTensor(fn, num, log=False))
    bad_want = _bad_reported(capsys)
    got = T.collect(utils_v2.GetTensorDevice(fn, num, "cuda", log=False))
    bad_got = _bad_reported(capsys)
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert bad_got == bad_want
    assert got[2][-1] == 1 and not any(got[2][:-1])
    return got, bad_got


@pytest.mark.parametrize("name", ["golden_a", "golden_b", "golden_a_gz", "golden_b_gz", "golden_a_nonl"])
def test_reference_goldens_through_get_tensor_device(files, name, monkeypatch, capsys):
    got, bad = _same_batches(files[name], 16, monkeypatch, capsys)
    d = np.load(os.path.join(T.GOLD, "gettensor_%s.npz" % name[7]), allow_pickle=True)
    assert bad == 0
    assert np.array_equal(got[0], np.ascontiguousarray(d["X"], dtype=np.float32).reshape(-1, T.NV).view(np.uint32))
    assert [b":".join((c, p, s.upper())).decode() for c, p, s in got[1]] == [str(p) for p in d["pos"]]


def test_volume_in_the_producers_format():
    text = T.volume_text()
    lines = text.count(b"\n")
    assert lines >= 70000
    r = dev_parse(text, lines + 5, offset=3)
    assert int(r["info"][0]) == len(text) and int(r["info"][1]) == lines
    same_as_host(r, text, expect_host=0)
    assert 0 < np.count_nonzero(r["status"] == T.SKIP) < lines // 50
    assert np.any(np.signbit(r["x"][r["status"] == T.ROW]) & (r["x"][r["status"] == T.ROW] == 0))     # -0.0 came through


def test_off_format_lines_are_left_to_the_host_and_no_others(files, monkeypatch, capsys):
    text, want_status = T.off_format_text()
    r = dev_parse(text, len(want_status) + 1)
    assert int(r["info"][1]) == len(want_status) and int(r["info"][0]) == len(text)
    assert np.array_equal(r["status"], want_status), np.flatnonzero(r["status"] != want_status)
    same_as_host(r, text, expect_host=int(np.count_nonzero(want_status == T.HOST)))
    # the rows the device did accept are the host's rows of exactly those lines
    lines = text.split(b"\n")[:-1]
    kept = b"".join(l + b"\n" for l, s in zip(lines, r["status"]) if s == T.ROW)
    _c, bad, hx, _m = T.host_parse(kept)
    assert bad == 0 and np.array_equal(r["x"][r["status"] == T.ROW].view(np.uint32), hx.view(np.uint32))
    got, bad = _same_batches(files["off_format"], 50, monkeypatch, capsys)
    assert bad > 10


def test_crlf_file(tmp_path, monkeypatch, capsys):
    text = T.volume_text(300, seed=21).replace(b"\n", b"\r\n")
    r = dev_parse(text, 1000)
    assert np.all(r["status"][[len(l) > 1 for l in text.split(b"\n")[:-1]]] == T.HOST)
    fn = str(tmp_path / "crlf.txt"); open(fn, "wb").write(text)
    got, _bad = _same_batches(fn, 100, monkeypatch, capsys)
    assert len(got[1]) > 250


def test_slab_edges():
    from clairvoyante_amd import _lib
    text = T.volume_text(40, seed=4)
    lines = text.count(b"\n")
    for t, max_lines, want in ((b"", 10, (0, 0)), (text[:1500], 10, (0, 0)), (b"x" * 70000, 10, (0, 0)), (text, 0, (0, 0))):
        r = dev_parse(t, max_lines)
        assert tuple(r["info"]) == want + (0, 0)
    ends = [i for i, c in enumerate(text) if c == 10]
    for max_lines in (1, lines - 1, lines, lines + 1):
        r = dev_parse(text + b"chr1 5 partial line", max_lines, offset=7)
        k = min(max_lines, lines)
        assert int(r["info"][0]) == ends[k - 1] + 1 and int(r["info"][1]) == k
        same_as_host(r, text)


def test_bad_arguments_are_errors_before_any_launch():
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    need = ctypes.c_int64()
    assert lib.cv_parse_tensor_text_dev_workspace(100, 4, None) != 0
    assert lib.cv_parse_tensor_text_dev_workspace(-1, 4, ctypes.byref(need)) != 0
    assert lib.cv_parse_tensor_text_dev_workspace(100, -4, ctypes.byref(need)) != 0
    _lib.check(lib.cv_parse_tensor_text_dev_workspace(100, 1, ctypes.byref(need)))
    for args, word in (((None, 100, 1, p, p, p, p, p, 4096, None), "null"), ((p, 100, 1, p, p, p, p, None, 4096, None), "null"),
                       ((p, -1, 1, p, p, p, p, p, 4096, None), "range"), ((p, 100, -1, p, p, p, p, p, 4096, None), "range"),
                       ((p, 100, 1, p, p, p, p, p, need.value - 1, None), "workspace")):
        assert lib.cv_parse_tensor_text_dev(*args) != 0
        assert word in lib.cv_last_error().decode()
    assert lib.cv_text_gather_rows(None, p, 3, p, None) != 0 and lib.cv_text_gather_rows(p, p, -1, p, None) != 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


def test_gather_rows():
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    x = torch.randn(1000, T.NV, device="cuda")
    idx = torch.tensor([5, 3, 999, 0, 3], dtype=torch.int64, device="cuda")
    out = torch.zeros(5, T.NV, device="cuda")
    _lib.check(lib.cv_text_gather_rows(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(idx.data_ptr()), 5, ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(out, x[idx])


@pytest.mark.parametrize("name,num", [("volume", 256), ("blank_then_rows", 100)])
@pytest.mark.parametrize("slab", [4096, 65536, 1 << 20])
def test_slab_cuts(files, name, num, slab, monkeypatch, capsys):
    got, _bad = _same_batches(files[name], num, monkeypatch, capsys, slab)
    assert sum(got[3]) == len(got[1]) > 250


def test_default_slabs_and_stream_form(files, monkeypatch, capsys):
    got, _bad = _same_batches(files["volume"], 16384, monkeypatch, capsys)
    assert len(got[3]) >= 4
    monkeypatch.setenv("CV_TEXT", "stream")
    _same_batches(files["volume"], 16384, monkeypatch, capsys)


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tensors(tmp_path_factory):
    d = tmp_path_factory.mktemp("textparse_e2e")
    x = common.inputs(6000, seed=17)
    raw = x.copy()
    for i in range(1, 4):
        raw[:, :, :, i] += raw[:, :, :, 0]
    rng = np.random.RandomState(3)
    lines = []
    for j in range(raw.shape[0]):
        seq = "".join(rng.choice(list("ACGT"), 33))
        if j % 97 == 5:
            seq = seq[:16] + "N" + seq[17:]
        lines.append("%s %d %s %s" % ("chr%d" % (1 + j % 4), 10000 + 7 * j, seq, " ".join("%0.1f" % v for v in raw[j].reshape(-1))))
    text = ("\n".join(lines) + "\n").encode()
    out = {"plain": str(d / "t.txt"), "gz": str(d / "t.txt.gz"), "nonl": str(d / "nonl.txt"), "dir": str(d)}
    open(out["plain"], "wb").write(text)
    open(out["nonl"], "wb").write(text[:-1])
    with gzip.open(out["gz"], "wb") as fh:
        fh.write(text)
    return out


@pytest.fixture(scope="module")
def checkpoints(oracle, tmp_path_factory):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    d = tmp_path_factory.mktemp("textparse_ckpt")
    out = {}
    for arch, mod in (("full", clairvoyante_v3), ("slim", clairvoyante_v3_slim)):
        m = mod.Clairvoyante(); m.setParameters(common.bench_params(oracle, arch))
        out[arch] = str(d / arch / "model"); m.saveParameters(out[arch]); m.close()
    return out


def _run(tensors, checkpoints, form, arch, show_ref, tag):
    from clairvoyante_amd import callVar
    out = os.path.join(tensors["dir"], "%s_%s_%d_%s.vcf" % (form, arch, show_ref, tag))
    a = types.SimpleNamespace(tensor_fn=tensors[form], chkpnt_fn=checkpoints[arch], call_fn=out, qual=30, sampleName="S", ref_fn=None,
                              threads=None, showRef=show_ref, v3=True, v2=False, slim=arch == "slim")
    callVar.Run(a)
    return open(out, "rb").read()


@pytest.mark.parametrize("form", ["plain", "gz", "nonl"])
@pytest.mark.parametrize("arch", ["full", "slim"])
@pytest.mark.parametrize("show_ref", [False, True])
def test_callvar_gives_the_same_vcf_with_either_parser(tensors, checkpoints, form, arch, show_ref, monkeypatch):
    from clairvoyante_amd import utils_v2
    vcf = {}
    for side in ("device", "host"):
        monkeypatch.setenv("CV_TEXT_PARSE", side)
        before = dict(utils_v2.text_parse_counts)
        vcf[side] = _run(tensors, checkpoints, form, arch, show_ref, side)
        assert utils_v2.text_parse_counts[side] == before[side] + 1
    records = [l for l in vcf["host"].splitlines() if not l.startswith(b"#")]
    print("%s %s showRef=%s: %d records" % (form, arch, show_ref, len(records)))
    assert len(records) >= 200
    assert vcf["device"] == vcf["host"]


def test_the_input_chooses_the_parser(tensors, checkpoints, monkeypatch):
    from clairvoyante_amd import callVar, utils_v2
    monkeypatch.delenv("CV_TEXT_PARSE", raising=False)
    size = os.path.getsize(tensors["plain"])
    for floor, side in ((size, "device"), (size + 1, "host")):        # a file at the threshold and one byte below it
        monkeypatch.setattr(callVar, "TEXT_DEVICE_MIN_BYTES", (floor, floor))
        before = dict(utils_v2.text_parse_counts)
        _run(tensors, checkpoints, "plain", "full", False, "rule_" + side)
        after = utils_v2.text_parse_counts
        assert after[side] == before[side] + 1 and sum(after.values()) == sum(before.values()) + 1


# ---- asynchrony --------------------------------------------------------------------------------------------------------
def test_the_call_returns_before_the_work_in_front_of_it_ends():
    import torch
    text = T.volume_text(2000, seed=8)
    dev_parse(text, 3000)                                              # (first use: code objects loaded, pools warm)
    s = torch.cuda.Stream()
    a = torch.randn(8192, 8192, device="cuda")
    d = prepare(text, 3000)
    with torch.cuda.stream(s):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(30):
            a = (a @ a) * 1e-4
        e1.record(s)
    launch(d, s)
    still_running = not e1.query()
    torch.cuda.synchronize()
    long_ms = e0.elapsed_time(e1)
    print("long kernels %.1f ms, host time of the call %.3f ms" % (long_ms, d["host_seconds"] * 1e3))
    assert still_running and d["host_seconds"] * 1e3 < long_ms
    same_as_host(to_host(d), text)


def test_two_slabs_in_flight_on_two_streams():
    import torch
    ta, tb = T.volume_text(3000, seed=31), T.volume_text(2500, seed=32)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    da, db = prepare(ta, 4000), prepare(tb, 4000, offset=9)
    launch(da, sa); launch(db, sb)
    torch.cuda.synchronize()
    same_as_host(to_host(da), ta)
    same_as_host(to_host(db), tb)
