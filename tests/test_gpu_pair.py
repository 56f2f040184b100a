"""PairWithNonVariants on the GPU (CV_PAIR=device: clairvoyante_amd/bed_items.py _PairWalk, existing kernels composed) against
the loop that defines it (PairWithNonVariants.Pair_host): the inflated bytes of --output_fn, the returned dict and the log
lines, no tolerance.  Every test asserts PairWithNonVariants.counts(), so that neither a silent hand-over nor a call that
never reached the device can pass.  A line the device does not vouch for sends the WHOLE call to the loop: the loop's file,
the loop's exception, every log line once.  cv_items_copy_dev, the one new entry point, is held to its host form between
canaries.

Two of the planted lines cannot hand a call over when they stand in the BED file: a blank line and a line with a leading
blank.  The BED's bytes are never written, and the loop itself skips the one and split()s the other, so the device's BED
reader answers both as the loop does; the tests hold those two to the loop's result with the device call counted."""
import ctypes
import os

import numpy as np
import pytest

import items_copy_cases as ic
import pair_cases as pc

pytestmark = pytest.mark.gpu
FORMATS = ("plain", "gz", "bgzf")
SINKS = ("gzip", "bgzf", "bgzf_device")
R_ONE = 1000                                                  # an amp at which every usable candidate is taken


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_pair")
    var, can, bed = pc.fixture()
    out = {"dir": d, "var_lines": var, "can_lines": can, "bed_lines": bed, "loops": {}}
    for how in FORMATS:
        out["var", how] = pc.write(d / ("var." + how), var, how)
        out["can", how] = pc.write(d / ("can." + how), can, how)
        out["bed", how] = pc.write(d / ("conf.bed." + how), bed, how)
    return out


def _loop(files, use_bed, amp):
    """the loop's (dict, log lines, inflated bytes) over the fixture, once per (BED, amp)"""
    from clairvoyante_amd import PairWithNonVariants as pw
    if (use_bed, amp) not in files["loops"]:
        out = str(files["dir"] / ("loop_%d_%s.gz" % (use_bed, amp)))
        got, msgs, raised = pc.run(pw.Pair_host, pc.args_of(files["var", "plain"], files["can", "plain"],
                                                            files["bed", "plain"] if use_bed else None, out, amp=amp), pc.SEED)
        assert raised is None
        files["loops"][use_bed, amp] = (got, msgs, pc.inflated(out))
    return files["loops"][use_bed, amp]


@pytest.fixture
def device_route(monkeypatch):
    from clairvoyante_amd import PairWithNonVariants as pw
    monkeypatch.setenv("CV_PAIR", "device")
    monkeypatch.delenv("CV_BGZF_DEFLATE", raising=False)
    pw.counts(reset=True)
    return pw


def _host_answer(pw, args_of_out, tmp_path, name="want"):
    """the loop under Pair's seed line -> (dict, log lines, exception's type and text, the file's inflated bytes)"""
    out = str(tmp_path / (name + ".gz"))
    got, msgs, raised = pc.run(pw.Pair_host, args_of_out(out), pc.SEED)
    return got, msgs, (type(raised), str(raised)), _inflated_or_raw(out)


def _inflated_or_raw(fn):
    if not os.path.exists(fn):                               # (the loop raised before it opened its output)
        return None
    try:
        return pc.inflated(fn)
    except Exception:                                        # noqa: BLE001 -- a file cut short by the failure path
        return open(fn, "rb").read()


def _device_answer(pw, args_of_out, tmp_path, sink="gzip", monkeypatch=None, name="got"):
    if sink == "bgzf_device":
        monkeypatch.setenv("CV_BGZF_DEFLATE", "device")
    out = str(tmp_path / (name + ".gz"))
    a = args_of_out(out)
    a.bgzf = sink != "gzip"
    got, msgs, raised = pc.run(pw.Pair, a)
    assert msgs[0] == "PairWithNonVariants: seed %d" % pc.SEED
    return got, msgs[1:], (type(raised), str(raised)), _inflated_or_raw(out)


def _on_device(pw, var, can, bed=None):
    c = pw.counts(reset=True)
    assert (c["device_calls"], c["host_calls"], c["handed_over_calls"]) == (1, 0, 0), c
    assert (c["device_lines_var"], c["device_lines_can"]) == (var, can), c
    if bed is not None:
        assert c["device_lines_bed"] == bed, c


def _handed_over(pw):
    c = pw.counts(reset=True)
    assert (c["device_calls"], c["host_calls"], c["handed_over_calls"]) == (0, 1, 1), c
    assert c["device_lines_var"] == c["device_lines_can"] == c["device_lines_bed"] == 0, c


# with and without the BED, the three input forms, r < 1 and r == 1, the three sinks: every value of each with every value
# of two others at least once, not the whole product
MATRIX = [(bed, fmt, 2, "gzip") for bed in (True, False) for fmt in FORMATS] + \
         [(True, "plain", 2, "bgzf"), (False, "gz", 2, "bgzf_device"), (True, "bgzf", 2, "bgzf_device"),
          (True, "bgzf", R_ONE, "gzip"), (False, "plain", R_ONE, "bgzf"), (True, "gz", R_ONE, "bgzf_device"), (False, "bgzf", R_ONE, "gzip")]


@pytest.mark.parametrize("use_bed, fmt, amp, sink", MATRIX)
def test_the_route_equals_the_loop(files, device_route, monkeypatch, tmp_path, use_bed, fmt, amp, sink):
    from clairvoyante_amd import utils_v2
    pw = device_route
    want, msgs, text = _loop(files, use_bed, amp)
    if amp == R_ONE:
        assert want["r"] == 1 and want["o2"] == want["c"] > 0
    else:
        assert 0 < want["o2"] < want["c"] and 0 < want["r"] < 1
    args = lambda out: pc.args_of(files["var", fmt], files["can", fmt], files["bed", fmt] if use_bed else None, out, amp=amp)
    got = _device_answer(pw, args, tmp_path, sink, monkeypatch)
    # (the log lines name the input files: the loop ran over the plain ones)
    rename = lambda m: m.replace(files["var", "plain"], files["var", fmt]).replace(files["can", "plain"], files["can", fmt])
    assert got[2] == (type(None), "None") and got[0] == want and got[3] == text
    assert got[1] == [rename(m) for m in msgs] and len(got[1]) == (8 if use_bed else 7) and len(set(got[1])) == len(got[1])
    _on_device(pw, len(files["var_lines"]), len(files["can_lines"]), len(files["bed_lines"]) if use_bed else 0)
    if sink != "gzip":
        assert utils_v2.is_bgzf(str(tmp_path / "got.gz"))


@pytest.mark.parametrize("room", [None, 0])
@pytest.mark.parametrize("fmt", FORMATS)
def test_small_slabs_and_a_late_newline(files, device_route, monkeypatch, tmp_path, fmt, room):
    """slabs of 257 bytes cut nearly every line; the last line of each file lacks its newline and gets one, as strip() + "\\n"
    gives it.  room 0: no text stays resident between the passes, so both files are walked a second time"""
    from clairvoyante_amd import bed_items, utils_v2
    pw = device_route
    monkeypatch.setattr(utils_v2, "TRUTH_SLAB_BYTES", 257)
    monkeypatch.setattr(bed_items, "PAIR_RESIDENT_BYTES", room)
    want, msgs, text = _loop(files, True, 2)
    cut = {k: pc.write(tmp_path / (k + "." + fmt), files[k + "_lines"], fmt, last_newline=False) for k in ("var", "can", "bed")}
    got = _device_answer(pw, lambda out: pc.args_of(cut["var"], cut["can"], cut["bed"], out), tmp_path, "gzip" if room is None else "bgzf")
    assert got[2][0] is type(None) and got[0] == want and got[3] == text and text.endswith(b"\n")
    assert [m.split(" in ")[0] for m in got[1]] == [m.split(" in ")[0] for m in msgs]
    _on_device(pw, len(files["var_lines"]), len(files["can_lines"]), len(files["bed_lines"]))


def _edge_case(name, files):
    var, can, bed = files["var_lines"], files["can_lines"], files["bed_lines"]
    key = lambda l: l.split()[:2]
    if name == "every candidate on a truth key":
        return var, [l for l in can if key(l) in [key(v) for v in var]] + var[:30], bed
    if name == "an empty variant file":
        return [], can, bed
    if name == "an empty candidate file":
        return var, [], bed
    if name == "a contig only the candidates have, no BED":
        return var, can + [b"onlycan %d tail%d" % (p, p) for p in range(1, 120)], None
    if name == "a contig only the candidates have, with a BED":
        return var, can + [b"onlycan %d tail%d" % (p, p) for p in range(1, 120)], bed
    if name == "duplicate rows on both sides":
        return var + var[:50] + var[:50], can + can[:200] + can[100:300], bed
    raise KeyError(name)


EDGES = ("every candidate on a truth key", "an empty variant file", "an empty candidate file", "a contig only the candidates have, no BED",
         "a contig only the candidates have, with a BED", "duplicate rows on both sides")


@pytest.mark.parametrize("name", EDGES)
def test_edge_cases_in_the_inputs(files, device_route, tmp_path, name):
    pw = device_route
    var, can, bed = _edge_case(name, files)
    fmt = FORMATS[EDGES.index(name) % 3]
    fns = [pc.write(tmp_path / ("var." + fmt), var, fmt), pc.write(tmp_path / ("can." + fmt), can, fmt),
           pc.write(tmp_path / "conf.bed", bed) if bed is not None else None]
    args = lambda out: pc.args_of(fns[0], fns[1], fns[2], out, amp=0.5 if "contig only" in name else 2)
    want = _host_answer(pw, args, tmp_path)
    got = _device_answer(pw, args, tmp_path)
    assert want[2] == (type(None), "None") and got == want
    _on_device(pw, len(var), len(can))
    d, text = want[0], want[3]
    if name == "every candidate on a truth key":
        assert (d["c"], d["r"], d["o2"]) == (0, 1.0, 0) and len(can) > 20
    elif name == "an empty variant file":
        assert (d["v"], d["r"], d["o1"], d["o2"]) == (0, 0, 0, 0) and d["c"] > 0 and text == b""
    elif name == "an empty candidate file":
        assert (d["c"], d["o2"]) == (0, 0) and text == b"".join(l + b"\n" for l in var)
    elif name == "a contig only the candidates have, no BED":
        kept = text.count(b"\nonlycan ")
        assert 0 < kept < 119 and 0 < d["r"] < 1                # kept by its draw: some, not all
    elif name == "a contig only the candidates have, with a BED":
        assert b"onlycan" not in text and d["o2"] > 0
    else:
        assert d["v"] == len(var) and d["o1"] == len(var) and 0 < d["o2"] < d["c"]


PLANTS = {"a blank line": b"", "a leading blank": None, "one token": b"chr1", "007": b"chr1 007 x", "a carriage return": b"chr1 1234 x\r",
          "the byte 0x80": b"chr1 1235 \x80"}
BED_PLANTS = {"a blank line": b"", "a leading blank": b" chr1 5 9", "one token": b"chr1", "007": b"chr1 007 9", "a carriage return": b"chr1 5 9\r",
              "the byte 0x80": b"chr\x80 5 9"}
DEVICE_ANSWERS = {("bed", "a blank line"), ("bed", "a leading blank")}        # (see the module's docstring)


@pytest.mark.parametrize("plant", sorted(PLANTS))
@pytest.mark.parametrize("where", ["var", "can", "bed"])
def test_a_line_the_device_does_not_vouch_for_hands_the_call_over(files, device_route, tmp_path, where, plant):
    pw = device_route
    lines = {k: list(files[k + "_lines"]) for k in ("var", "can", "bed")}
    at = len(lines[where]) // 2
    bad = BED_PLANTS[plant] if where == "bed" else PLANTS[plant]
    if bad is None:
        bad = b" " + lines[where][at]
    lines[where].insert(at, bad)
    fmt = FORMATS[(sorted(PLANTS).index(plant) + ["var", "can", "bed"].index(where)) % 3]
    fns = {k: pc.write(tmp_path / (k + "." + fmt), v, fmt) for k, v in lines.items()}
    args = lambda out: pc.args_of(fns["var"], fns["can"], fns["bed"], out, amp=R_ONE)     # (every usable row is written, a planted one too)
    want = _host_answer(pw, args, tmp_path)
    got = _device_answer(pw, args, tmp_path)
    assert got == want
    if want[3] is not None and bad.strip() and (where == "var" or (where == "can" and b"123" in bad)):
        assert b"\n" + bad.strip() + b"\n" in want[3]                            # the planted row is in the loop's file, stripped
    assert len(set(got[1])) == len(got[1]) and len(got[1]) <= 8          # no log line twice
    if (where, plant) in DEVICE_ANSWERS:
        assert want[2] == (type(None), "None")
        _on_device(pw, len(lines["var"]), len(lines["can"]))
    else:
        _handed_over(pw)
    if plant in ("one token",):
        assert want[2][0] is IndexError
    if plant == "the byte 0x80" and where == "bed":
        assert want[2][0] is UnicodeDecodeError


# ---- cv_items_copy_dev against its host form ----------------------------------------------------------------------------------
CANARY = 4096


def _both_forms(text, off, kept_len, out_cap):
    """-> (room, counts) of cv_items_copy_host_form and of cv_items_copy_dev, the device's room between two canaries that
    must come back untouched"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = np.frombuffer(text, dtype=np.uint8).copy()
    off, kept_len = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(kept_len, dtype=np.int64)
    n = len(off)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data) if a.size else None
    room = np.full(out_cap, ic.FILL, dtype=np.uint8)
    counts = np.full(4, -1, dtype=np.int64)
    _lib.check(lib.cv_items_copy_host_form(hp(t), len(t), n, hp(off), hp(kept_len), hp(room), out_cap, hp(counts)))
    P = _lib.ptr
    # the text between canaries too: a read outside it is not seen, but the layout puts the room's neighbours under watch
    d_text, d_off, d_len = torch.from_numpy(t).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(kept_len).to(dev)
    d_room = torch.full((out_cap + 2 * CANARY,), ic.FILL, dtype=torch.uint8, device=dev)
    d_counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    need = _lib.workspace(lib.cv_items_copy_workspace, n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.cv_items_copy_dev(P(d_text), len(t), n, P(d_off), P(d_len), ctypes.c_void_p(d_room.data_ptr() + CANARY), out_cap,
                                     P(d_counts), P(ws), need, _lib.stream_arg(dev)))
    torch.cuda.current_stream(dev).synchronize()
    got = d_room.cpu().numpy()
    assert (got[:CANARY] == ic.FILL).all() and (got[CANARY + out_cap:] == ic.FILL).all(), "a byte outside the room changed"
    assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_len.cpu().numpy(), kept_len)
    return (room.tobytes(), counts.tolist()), (got[CANARY:CANARY + out_cap].tobytes(), d_counts.cpu().tolist())


@pytest.mark.parametrize("name", sorted(ic.cases()))
def test_the_gather_by_given_lengths_is_its_host_form(name):
    text, off, kept_len, out_cap = ic.cases()[name]
    host, device = _both_forms(text, off, kept_len, out_cap)
    assert host == ic.restated(text, off, kept_len, out_cap) and device == host
    if name == "one byte short":
        last = int(kept_len[-1])
        assert last > 1 and device[0][-(last - 1):] == bytes([ic.FILL]) * (last - 1) and device[1][2] == out_cap + 1


def test_the_gather_past_the_copy_kernels_line():
    """ik_copy runs at most 65 536 blocks of 4 waves, one wave per row: 262 144 + 65 rows make its waves take a second row"""
    n = 65536 * 4 + 65
    rng = np.random.RandomState(31)
    lengths = rng.randint(8, 17, n).astype(np.int64)
    text, off = ic.lines_text(lengths, seed=32)
    kept_len = lengths * (np.arange(n) % 3 == 0)
    out_cap = int(kept_len.sum())
    host, device = _both_forms(text, off, kept_len, out_cap)
    want = b"".join(text[o:o + m] for o, m in zip(off[::3].tolist(), lengths[::3].tolist()))
    assert host == (want, [0, 0, out_cap, 0]) and device == host and kept_len[65536 * 4:].sum() > 0


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_the_device_file_reads_back_as_the_loops(device_route, monkeypatch, tmp_path):
    """tensor-shaped rows: Pair --bgzf with the device deflate, read back through utils_v2.GetTrainingArray"""
    from clairvoyante_amd import utils_v2
    pw = device_route
    rng = np.random.RandomState(8)
    row = lambda c, p: ("%s %d %s %s" % (c, p, "ACGTACGTACGTACGTACGTACGTACGTACGTA", " ".join("%d" % v for v in rng.randint(0, 30, 528)))).encode()
    var_keys = [("chr1", 100 + 7 * k) for k in range(12)]
    can_keys = [("chr1", 101 + 7 * k) for k in range(40)] + var_keys[:3]
    var_fn = pc.write(tmp_path / "var.gz", [row(c, p) for c, p in var_keys], "bgzf")
    can_fn = pc.write(tmp_path / "can.gz", [row(c, p) for c, p in can_keys], "bgzf")
    truth_fn = pc.write(tmp_path / "truth", [("%s %d A C 0 1" % (c, p)).encode() for c, p in var_keys])
    got = []
    for name, how in (("loop.gz", "host"), ("device.bgzf.gz", "device")):
        out = str(tmp_path / name)
        monkeypatch.setenv("CV_PAIR", how)
        monkeypatch.setenv("CV_BGZF_DEFLATE", how)
        pw.counts(reset=True)
        d = pw.Pair(pc.args_of(var_fn, can_fn, None, out, amp=2, seed=4, bgzf=True))
        c = pw.counts()
        assert (c["device_calls"], c["host_calls"], c["handed_over_calls"]) == ((1, 0, 0) if how == "device" else (0, 1, 0))
        total, XC, YC, PC = utils_v2.GetTrainingArray(out, truth_fn, None, shuffle=False)
        got.append((d, total) + tuple(np.concatenate([utils_v2.unpack_array(c) for c in chunks]) for chunks in (XC, YC, PC)))
    assert got[0][0] == got[1][0] and 0 < got[0][0]["o2"] < 40
    assert got[0][1] == got[1][1] > 12 and list(got[0][4]) == list(got[1][4]) and len(got[0][4]) == got[0][1]
    assert np.array_equal(got[0][2], got[1][2]) and np.array_equal(got[0][3], got[1][3]) and got[0][3][:, 4].sum() == 12
    assert utils_v2.is_bgzf(str(tmp_path / "device.bgzf.gz")) and pc.inflated(str(tmp_path / "device.bgzf.gz")) == pc.inflated(str(tmp_path / "loop.gz"))
