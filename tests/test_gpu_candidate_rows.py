"""The candidate list on the device, both ends (opt-in): ExtractVariantCandidates' rows written in HBM
(csrc/cv_candrows_dev.hip, CV_CANDIDATE_ROWS=device) and CreateTensor.read_candidates through the device's line pass
(CV_CANDIDATE_LIST=device).  The host loops are the definitions: every byte and every array here is compared with theirs,
the planted arrays with cv_candidate_rows_host_form (held to snprintf + std::stable_sort by
test_candidate_rows_core_host.py, whose driver also supplies the table of edge cases planted here)."""
import ctypes
import gzip
import io
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

import candlist_cases as cc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- planted arrays through the C ABI ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """the driver's table of edge cases: count patterns, reference windows, contig name lengths"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("candrows_table") / "candrows_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(HERE, "native", "candrows_core_driver.cpp"), "-o", exe])
    out = subprocess.check_output([exe, "dump"]).decode().split("\n")
    return {"counts": np.array([[int(v) for v in l.split()[1:]] for l in out if l.startswith("C ")], dtype=np.int32),
            "windows": [(int(l.split()[1]), bytes.fromhex(l.split()[2])) for l in out if l.startswith("W ")],
            "names": [int(l.split()[1]) for l in out if l.startswith("G ")]}


def planted(table, rows, which):
    """`rows` output rows over window `which`: every position of it, one in front and one behind, the count patterns in
    turn, in a shuffled order with two indices outside the entries"""
    first0, ref = table["windows"][which % len(table["windows"])]
    n = rows + 3
    pos0 = first0 - 1 + (np.arange(n, dtype=np.int64) * 7) % (len(ref) + 2)
    c7 = table["counts"][(np.arange(n) * 5 + which) % len(table["counts"])]
    order = np.random.RandomState(rows * 31 + which).permutation(n)[:rows].astype(np.int64)
    if rows >= 4:
        order[1], order[rows - 2] = -1, n
    return first0, ref, pos0, np.ascontiguousarray(c7), order


def rows_dev(ctg, order, pos0, c7, ref, first0, phase, cap_short=0):
    """cv_candidate_rows_dev into a buffer with canaries -> (text, off, status, the whole buffer, where the text stands)"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    P = _lib.ptr
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows, n = len(order), len(pos0)
    order_d, pos_d, c7_d = T(order), T(pos0), T(c7)
    ref_d = T(np.frombuffer(ref, dtype=np.uint8).copy())
    off = torch.full((rows + 1,), -7, dtype=torch.int64, device=dev)
    status = torch.full((max(rows, 1),), 9, dtype=torch.uint8, device=dev)
    need = _lib.workspace(lib.cv_candidate_rows_workspace, rows)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    st = _lib.stream_arg(dev)

    def call(text, cap):
        _lib.check(lib.cv_candidate_rows_dev(ctg, len(ctg), P(order_d), rows, n, P(pos_d), None, P(c7_d), P(ref_d), first0, len(ref),
                                             ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(status.data_ptr()), text, cap,
                                             ctypes.c_void_p(ws.data_ptr()), need, st))
    call(None, 0)
    total = int(off[rows])
    buf = torch.full((total + 96,), 0xA5, dtype=torch.uint8, device=dev)
    at = 32 + (phase - (buf.data_ptr() + 32)) % 16
    call(ctypes.c_void_p(buf.data_ptr() + at), total - cap_short)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return b[at:at + total].tobytes(), off.cpu().numpy(), status.cpu().numpy()[:rows], b, at


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 130])
@pytest.mark.parametrize("phase", [0, 1, 15])
def test_planted_rows_equal_the_host_form(table, rows, phase):
    for which in range(len(table["windows"])) if rows == 65 else (rows + phase,):
        first0, ref, pos0, c7, order = planted(table, rows, which)
        want, woff, wstatus = cc.host_form(b"ctgA", order, pos0, c7, ref, first0)
        got, off, status, buf, at = rows_dev(b"ctgA", order, pos0, c7, ref, first0, phase)
        assert np.array_equal(off, woff) and np.array_equal(status, wstatus)
        assert got == want
        assert (buf[:at] == 0xA5).all() and (buf[at + len(want):] == 0xA5).all()
        assert (np.diff(off)[status == 1] == 0).all()
        if rows >= 63:
            assert 0 < status.sum() < rows                  # rows of both kinds: 0x80, a negative count, outside the window


def test_contig_names_of_every_length(table):
    first0, ref, pos0, c7, order = planted(table, 65, 3)
    for n in table["names"]:
        ctg = bytes(97 + (i * 7 + n) % 26 for i in range(n))
        want, woff, wstatus = cc.host_form(ctg, order, pos0, c7, ref, first0)
        got, off, status, buf, at = rows_dev(ctg, order, pos0, c7, ref, first0, 5)
        assert got == want and np.array_equal(off, woff) and np.array_equal(status, wstatus)
        assert (buf[:at] == 0xA5).all() and (buf[at + len(want):] == 0xA5).all()
        assert status.all() == (n > 255) and (n <= 255 or off[-1] == 0)


@pytest.mark.parametrize("rows", [1, 65, 130])
def test_a_short_text_cap_leaves_the_short_row_and_everything_behind_it_unwritten(table, rows):
    first0, ref, pos0, c7, order = planted(table, rows, 2)
    if rows == 1:                                             # (a row the device vouches for)
        order[0] = int(np.flatnonzero(cc.host_form(b"chr20", None, pos0, c7, ref, first0)[2] == 0)[0])
    want, woff, wstatus = cc.host_form(b"chr20", order, pos0, c7, ref, first0)
    last = int(np.flatnonzero(wstatus == 0)[-1])
    got, off, status, buf, at = rows_dev(b"chr20", order, pos0, c7, ref, first0, 9, cap_short=1)
    keep = int(woff[last])
    assert np.array_equal(off, woff) and got[:keep] == want[:keep]
    assert (buf[:at] == 0xA5).all() and (buf[at + keep:] == 0xA5).all()


@pytest.mark.parametrize("name,pos0,late,last_pos", [
    ("no_tail", [1, 2, 5, 9], [0, 0, 0, 0], 10),
    ("only_tail", [4, 4, 6, 7], [0, 1, 0, 0], 4),
    ("late_twin_behind_its_regular_entry", [1, 3, 3, 5, 5, 8, 9, 9], [0, 0, 1, 0, 1, 0, 0, 1], 8),
    ("empty", [], [], 3),
    ("many", None, None, 3000),
])
def test_candidate_order_on_planted_lists(name, pos0, late, last_pos):
    import torch
    from clairvoyante_amd import pileup
    from clairvoyante_amd.ExtractVariantCandidates import candidate_order
    if pos0 is None:
        rng = np.random.RandomState(4)
        pos0 = np.sort(rng.randint(0, 6000, 5000))
        late = np.concatenate(([0], (pos0[1:] == pos0[:-1]).astype(np.int64)))
    res = {"pos0": np.array(pos0, dtype=np.int64), "late": np.array(late, dtype=np.int32), "last_pos": last_pos}
    sel = {"pos0": torch.from_numpy(res["pos0"]).cuda(), "late": torch.from_numpy(res["late"]).cuda(), "last_pos": last_pos}
    got = pileup.candidate_order_device(sel).cpu().numpy()
    assert np.array_equal(got, candidate_order(res))


# ---- through MakeCandidates -------------------------------------------------------------------------------------------------
def make(monkeypatch, route, args, batch=None):
    """MakeCandidates under CV_CANDIDATE_ROWS=route -> (its return value, the counts of both sides)"""
    from clairvoyante_amd import ExtractVariantCandidates as evc, pileup
    monkeypatch.setenv("CV_CANDIDATE_ROWS", route)
    if batch is not None:
        monkeypatch.setattr(pileup, "CANDROWS_BATCH", batch)
    evc.candidate_row_counts(reset=True)
    ret = evc.MakeCandidates(args)
    return ret, evc.candidate_row_counts()


def to_pipe(monkeypatch, route, args, batch=None):
    out = io.BytesIO()
    monkeypatch.setattr(sys, "stdout", types.SimpleNamespace(buffer=out, write=lambda s: None, flush=lambda: None))
    ret, counts = make(monkeypatch, route, args, batch)
    monkeypatch.undo()
    return out.getvalue(), ret, counts


@pytest.mark.parametrize("name", cc.EVC_CASES)
def test_device_rows_equal_host_rows_and_the_golden_rows(name, tmp_path, monkeypatch):
    """the golden cases (a ctgStart / ctgEnd window and a BED among them) into gzip -c, --bgzf and PIPE, rows crossing
    batches of 7: the host route's bytes, the reference's rows, every row on the device"""
    args, want = cc.golden_evc_args(name, tmp_path / "host.gz")
    rows, counts = make(monkeypatch, "host", args)
    host = cc.inflate(args.can_fn)
    assert host.decode().splitlines() == want == rows and counts == {"host": len(want), "device": 0}
    for kind in ("gz", "bgzf", "PIPE"):
        args, _ = cc.golden_evc_args(name, "PIPE" if kind == "PIPE" else tmp_path / ("dev." + kind), bgzf=kind == "bgzf")
        if kind == "PIPE":
            got, ret, counts = to_pipe(monkeypatch, "device", args, batch=7)
        else:
            ret, counts = make(monkeypatch, "device", args, batch=7)
            got = cc.inflate(args.can_fn)
        assert got == host
        assert ret == len(want) and counts == {"host": 0, "device": len(want)}


def synth_files(tmp_path, seed, profile):
    from clairvoyante_amd import synth_pileup as sp
    prof = sp.NOISY_PROFILE if profile == "noisy" else sp.DEFAULT_PROFILE
    ref, lines = sp.make_alignments(seed=700 + seed, ref_len=8000, n_reads=1500, profile=prof, stack=6)
    base = str(tmp_path / ("synth%d" % seed))
    open(base + ".sam", "w").write("\n".join(lines) + "\n")
    open(base + ".fa", "w").write(">ctgA\n%s\n" % ref)
    open(base + ".fa.fai", "w").close()
    return base, ref


def synth_args(base, can_fn, **over):
    a = cc.evc_args("plain", can_fn, bam_fn=base + ".sam", ref_fn=base + ".fa")
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("seed,profile,mincov,thr,window", [(21, "default", 4, 0.125, None), (22, "noisy", 1, 0.05, (2000, 5000)),
                                                            (23, "noisy", 0, 0.3, None), (24, "default", 6, 0.2, (1, 7000))])
def test_device_rows_equal_host_rows_on_random_alignments(seed, profile, mincov, thr, window, tmp_path, monkeypatch):
    base, _ref = synth_files(tmp_path, seed, profile)
    from clairvoyante_amd import CreateTensor
    over = dict(minCoverage=mincov, threshold=thr, minMQ=5)
    if window:
        over.update(ctgStart=window[0], ctgEnd=window[1])
        monkeypatch.setattr(CreateTensor, "EXPAND", 300)     # the loaded reference starts inside the contig: ref_first > 0
    rows, _ = make(monkeypatch, "host", synth_args(base, tmp_path / "host.gz", **over))
    host = cc.inflate(tmp_path / "host.gz")
    ret, counts = make(monkeypatch, "device", synth_args(base, tmp_path / "dev.gz", bgzf=seed % 2 == 0, **over), batch=7 if seed == 21 else None)
    assert cc.inflate(tmp_path / "dev.gz") == host and len(rows) > 20
    assert ret == len(rows) and counts == {"host": 0, "device": len(rows)}


def test_a_reference_byte_of_0x80_or_more_sends_exactly_its_batch_to_the_host(tmp_path, monkeypatch):
    from clairvoyante_amd import ExtractVariantCandidates as evc
    base, ref = synth_files(tmp_path, 21, "default")
    rows, _ = make(monkeypatch, "host", synth_args(base, tmp_path / "plain.gz"))
    at = [int(r.split()[1]) for r in rows]
    p = next(q for q in at[8:] if at.count(q) == 1)         # a row behind the first batch of 7, without a late twin
    planted_ref = bytearray(ref.encode())
    planted_ref[p - 1] = 0xE9
    monkeypatch.setattr(evc, "load_reference", lambda *a: bytes(planted_ref))
    rows, _ = make(monkeypatch, "host", synth_args(base, tmp_path / "host.gz"))
    host = cc.inflate(tmp_path / "host.gz")
    k = [int(r.split()[1]) for r in rows].index(p)
    assert b" %d \xc3\xa9 " % p in host                     # chr() + .encode(): two bytes
    ret, counts = make(monkeypatch, "device", synth_args(base, tmp_path / "dev.gz"), batch=7)
    assert cc.inflate(tmp_path / "dev.gz") == host
    in_batch = min(7, len(rows) - k // 7 * 7)
    assert ret == len(rows) and counts == {"host": in_batch, "device": len(rows) - in_batch}


def test_a_seeded_training_sample_keeps_the_rows_the_host_keeps(tmp_path, monkeypatch):
    """--gen4Training --seed 5 at 2 * candidates / genomeSize = 0.1: only the kept entries are ordered and printed"""
    base, _ref = synth_files(tmp_path, 22, "noisy")
    over = dict(gen4Training=True, seed=5, candidates=1, genomeSize=20)
    every, _ = make(monkeypatch, "host", synth_args(base, tmp_path / "all.gz", gen4Training=True, seed=5, candidates=10, genomeSize=10))
    rows, _ = make(monkeypatch, "host", synth_args(base, tmp_path / "host.gz", **over))
    assert 0 < len(rows) < len(every) and 0.05 * len(every) < len(rows) < 0.2 * len(every)
    ret, counts = make(monkeypatch, "device", synth_args(base, tmp_path / "dev.gz", **over), batch=7)
    assert cc.inflate(tmp_path / "dev.gz") == cc.inflate(tmp_path / "host.gz")
    assert ret == len(rows) and counts == {"host": 0, "device": len(rows)}
    # without --seed the host loop runs whatever the switch says
    ret, counts = make(monkeypatch, "device", synth_args(base, tmp_path / "unseeded.gz", gen4Training=True, candidates=1, genomeSize=20))
    assert isinstance(ret, list) and counts == {"host": len(ret), "device": 0}


@pytest.mark.parametrize("route", ["host", "device"])
def test_no_read_gives_the_message_status_0_and_an_empty_list(route, tmp_path, monkeypatch, capfd):
    base, _ref = synth_files(tmp_path, 21, "default")
    open(base + ".sam", "w").close()
    with pytest.raises(SystemExit) as e:
        make(monkeypatch, route, synth_args(base, tmp_path / "none.gz"))
    assert e.value.code == 0
    assert "No read has been process" in capfd.readouterr().err
    assert cc.inflate(tmp_path / "none.gz") == b""


# ---- part 2: read_candidates --------------------------------------------------------------------------------------------------
def read_both(monkeypatch, fn, lo, hi, ctg="ctgA", slab=None):
    """read_candidates on both routes -> (host outcome, device outcome, the device call's counts)"""
    from clairvoyante_amd import CreateTensor, utils_v2
    if slab is not None:
        monkeypatch.setattr(utils_v2, "TRUTH_SLAB_BYTES", slab)
    monkeypatch.setenv("CV_CANDIDATE_LIST", "host")
    host = cc.outcome(CreateTensor.read_candidates, cc.can_args(fn, ctg), lo, hi)
    monkeypatch.setenv("CV_CANDIDATE_LIST", "device")
    CreateTensor.candidate_list_counts(reset=True)
    dev = cc.outcome(CreateTensor.read_candidates, cc.can_args(fn, ctg), lo, hi)
    return host, dev, CreateTensor.candidate_list_counts()


@pytest.mark.parametrize("slab", [None, 257])
def test_read_candidates_over_the_committed_lists(slab, monkeypatch):
    for name in ("plain", "noisy", "region"):
        fn = os.path.join(cc.G, name + ".can")
        lines = len(open(fn, "rb").read().splitlines())
        for lo, hi in [(None, None), (500, 1500)]:
            host, dev, counts = read_both(monkeypatch, fn, lo, hi, slab=slab)
            assert host[0] == "ok" and cc.same_outcome(host, dev) and len(host[1]) > (0 if lo else 40)
            assert counts["device_calls"] == 1 and counts["host_calls"] == 0 and counts["device_lines"] == lines


@pytest.mark.parametrize("name,data", cc.PLAIN_LISTS, ids=cc.ids(cc.PLAIN_LISTS))
def test_read_candidates_over_hand_made_lists(name, data, tmp_path, monkeypatch):
    fn = tmp_path / (name + ".can")
    fn.write_bytes(data)
    for ctg in ("ctgA", "ctgAA", "ctgC"):
        for lo, hi in cc.BOUNDS:
            host, dev, counts = read_both(monkeypatch, fn, lo, hi, ctg=ctg)
            assert host[0] == "ok" and cc.same_outcome(host, dev)
            assert counts["device_calls"] == 1 and counts["handed_over_calls"] == 0 and counts["host_calls"] == 0


def test_read_candidates_over_an_interleaved_list_in_every_form(tmp_path, monkeypatch):
    """three contigs line by line with duplicates, as plain text, .gz and BGZF, in slabs of 257 bytes"""
    from clairvoyante_amd.utils_v2 import BgzfWriter
    rng = np.random.RandomState(8)
    pos = rng.randint(1, 3000, 2500)
    data = b"".join(b"ctgA %d A 9 A 5 C 4\nctgB %d C 1 C 1\nctgAA %d x\n" % (p, p + 1, p + 2) for p in pos)
    plain, gz, bg = tmp_path / "l.can", tmp_path / "l.can.gz", tmp_path / "l.bgzf.gz"
    plain.write_bytes(data)
    gzip.open(str(gz), "wb").write(data)
    w = BgzfWriter(str(bg), block=4000)
    w.write(data)
    w.close()
    for fn in (plain, gz, bg):
        for ctg, (lo, hi) in [("ctgA", (None, None)), ("ctgB", (100, 2000)), ("ctgAA", (None, None))]:
            host, dev, counts = read_both(monkeypatch, fn, lo, hi, ctg=ctg, slab=257)
            assert host[0] == "ok" and cc.same_outcome(host, dev) and len(host[1]) > 500
            assert counts["device_calls"] == 1 and counts["device_lines"] == 7500


@pytest.mark.parametrize("name,data", cc.HAND_OVER, ids=cc.ids(cc.HAND_OVER))
def test_lines_the_device_does_not_vouch_for_hand_the_call_over(name, data, tmp_path, monkeypatch):
    fn = tmp_path / (name + ".can")
    fn.write_bytes(data)
    for slab in (None, 257):
        for lo, hi in [(None, None), (4, 9)]:
            host, dev, counts = read_both(monkeypatch, fn, lo, hi, slab=slab)
            assert cc.same_outcome(host, dev)
            assert counts["handed_over_calls"] == 1 and counts["host_calls"] == 1 and counts["device_calls"] == 0


def test_read_candidates_over_the_lists_the_device_wrote(tmp_path, monkeypatch):
    data = None
    for kind in ("gz", "bgzf"):
        args, want = cc.golden_evc_args("noisy", tmp_path / ("dev." + kind), bgzf=kind == "bgzf")
        make(monkeypatch, "device", args)
        data = cc.inflate(args.can_fn)
    (tmp_path / "dev.can").write_bytes(data)
    for fn in ("dev.can", "dev.gz", "dev.bgzf"):
        for lo, hi in [(None, None), (300, 2500)]:
            host, dev, counts = read_both(monkeypatch, tmp_path / fn, lo, hi, slab=257)
            assert host[0] == "ok" and cc.same_outcome(host, dev) and len(host[1]) > (0 if lo else 20)
            assert counts["device_calls"] == 1


# ---- closing the loop ---------------------------------------------------------------------------------------------------------
def test_tensors_from_a_device_written_list_read_on_the_device_equal_the_all_host_pair(tmp_path, monkeypatch):
    from clairvoyante_amd import CreateTensor
    base = os.path.join(cc.G, "noisy")

    def tensors(route, can_fn, out):
        monkeypatch.setenv("CV_CANDIDATE_LIST", route)
        CreateTensor.candidate_list_counts(reset=True)
        a = types.SimpleNamespace(bam_fn=base + ".sam", ref_fn=base + ".fa", can_fn=str(can_fn), tensor_fn=str(tmp_path / out), minMQ=0,
                                  ctgName="ctgA", ctgStart=None, ctgEnd=None, samtools=cc.FAKE, dcov=250, minCoverage=0,
                                  considerleftedge=True, bgzf=False)
        CreateTensor.OutputAlnTensor(a)
        return cc.inflate(a.tensor_fn), CreateTensor.candidate_list_counts()

    args, _ = cc.golden_evc_args("noisy", tmp_path / "host.can.gz")
    make(monkeypatch, "host", args)
    args, want = cc.golden_evc_args("noisy", tmp_path / "dev.can.gz", bgzf=True)
    make(monkeypatch, "device", args)
    host_rows, hc = tensors("host", tmp_path / "host.can.gz", "host.tensor.gz")
    dev_rows, dc = tensors("device", tmp_path / "dev.can.gz", "dev.tensor.gz")
    assert dev_rows == host_rows and host_rows.count(b"\n") > 40
    assert hc["host_calls"] == 1 and dc["device_calls"] == 1 and dc["device_lines"] == len(want)
