"""ChooseItemInBed / CountNumInBed / RandomSampling on the GPU (clairvoyante_amd/bed_items.py with CV_BED_ITEMS=device,
csrc/cv_beditems_dev.hip) against the host loops that define them: the bytes written, the counts, the exception raised and
the sampled positions, no tolerance.  Every test asserts the counters of bed_items.counts(), so that neither a silent
hand-over nor a dropped line can pass.  An irregular line hands the REST of the file to the host's per-line function."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

import bed_items_cases as bc
import truth_cases as tc

pytestmark = pytest.mark.gpu
FORMATS = ("plain", "gz", "bgzf")
LINE_CAP = 8192


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bed_items"))
    out = {"dir": d, "items": bc.item_lines(), "bed_lines": tc.bed_lines()}
    for how in FORMATS:
        out["items", how] = tc.write_lines(os.path.join(d, "items." + how), out["items"], how)
        out["bed", how] = tc.write_lines(os.path.join(d, "conf.bed." + how), out["bed_lines"], how)
    out["want"] = bc.host_answer(out["items", "plain"], out["bed", "plain"])
    return out


@pytest.fixture
def device_route(monkeypatch):
    from clairvoyante_amd import bed_items
    monkeypatch.setenv("CV_BED_ITEMS", "device")
    bed_items.counts(reset=True)
    return bed_items


def _device_answer(bed_items, items_fn, bed_fn):
    out = io.BytesIO()
    try:
        tally, raised = bed_items.choose_items(items_fn, bed_fn, out), None
    except Exception as e:                                   # noqa: BLE001
        tally, raised = None, e
    return out.getvalue(), tally, raised


def _on_device(bed_items, lines, calls=1):
    c = bed_items.counts(reset=True)
    assert c["host_lines"] == 0 and c["host_calls"] == 0 and c["handed_over_calls"] == 0 and c["device_calls"] == calls, c
    assert c["device_lines"] == lines, c


def test_the_expectation_is_worth_the_name(files):
    text, tally, raised = files["want"]
    lines = files["items"]
    assert raised is None and tally[0] == len(lines) == 2000 and 0.1 * 2000 < tally[1] < 0.9 * 2000
    sizes = np.array([len(l) for l in lines])
    assert (sizes < 40).sum() == 500 and sizes[sizes >= 40].min() >= 2000 and sizes.max() <= 3700 and sizes.max() > 3300
    ctgs = {l.split()[0] for l in lines}
    assert len(ctgs) >= 5 and bc.LACKING.encode() in ctgs and len(files["bed_lines"]) > 400
    kept = {l.split()[0] for l in text.split(b"\n") if l}
    assert len(kept) >= 4 and bc.LACKING.encode() not in kept


@pytest.mark.parametrize("slab", [None, 4096, 257])
@pytest.mark.parametrize("fmt", FORMATS)
def test_choose_and_count_equal_the_host_loop(files, device_route, monkeypatch, fmt, slab):
    """slabs of 4096 and 257 bytes: a 257-byte slab is shorter than most lines, so every line crosses several seams"""
    from clairvoyante_amd import utils_v2
    bed_items = device_route
    if slab is not None:
        monkeypatch.setattr(utils_v2, "TRUTH_SLAB_BYTES", slab)
    text, tally, _none = files["want"]
    got = _device_answer(bed_items, files["items", fmt], files["bed", fmt])
    assert got[2] is None and got[1] == tally and got[0] == text
    _on_device(bed_items, 2000)
    assert bed_items.count_items(files["items", fmt], files["bed", fmt]) == tally
    _on_device(bed_items, 2000)


def test_degenerate_inputs(files, device_route, tmp_path):
    bed_items = device_route
    d = str(tmp_path)
    items = files["items"][:300]
    everything = tc.write_lines(os.path.join(d, "all.bed"), [b"%s 0 1000000000" % c.encode() for c in tc.CONTIGS + (bc.LACKING,)], "plain")
    nothing = tc.write_lines(os.path.join(d, "none.bed"), [b"elsewhere 0 1000000000"], "gz")
    one = tc.write_lines(os.path.join(d, "one.bed"), [b"chr1\t100\t2500"], "bgzf")
    short = tc.write_lines(os.path.join(d, "short.bed"), [b"a 0 5"], "plain")
    fn = tc.write_lines(os.path.join(d, "items"), items, "bgzf")
    cut_kept = tc.write_lines(os.path.join(d, "cut_kept"), items + [b"chr1 150 last and kept"], "plain", last_newline=False)
    cut_dropped = tc.write_lines(os.path.join(d, "cut_dropped"), items + [b"chr1 99 last and dropped"], "gz", last_newline=False)
    empty = tc.write_lines(os.path.join(d, "empty"), [], "plain")
    four = tc.write_lines(os.path.join(d, "four"), [b"a 1"], "plain")
    cap = tc.write_lines(os.path.join(d, "cap"), [b"a 1 " + b"x" * (LINE_CAP - 4), b"a 2"], "plain")
    for items_fn, bed_fn, lines in ((fn, everything, 300), (fn, nothing, 300), (fn, one, 300), (cut_kept, files["bed", "plain"], 301),
                                    (cut_dropped, files["bed", "plain"], 301), (cut_kept, everything, 301), (empty, everything, 0),
                                    (four, short, 1), (cap, short, 2)):
        want = bc.host_answer(items_fn, bed_fn)
        got = _device_answer(bed_items, items_fn, bed_fn)
        assert want[2] is None and got == want, (items_fn, bed_fn)
        _on_device(bed_items, lines)
        assert bed_items.count_items(items_fn, bed_fn) == want[1]
        _on_device(bed_items, lines)
    assert bc.host_answer(fn, everything)[1] == (300, 300) and bc.host_answer(fn, nothing)[1] == (300, 0)
    assert bc.host_answer(cut_kept, everything)[0].endswith(b"last and kept") and bc.host_answer(four, short)[0] == b"a 1\n"
    assert len(bc.host_answer(cap, short)[0]) == LINE_CAP + 1 + 4
    # one byte more than CV_TRUTH_LINE_CAP: only the host answers, and it answers the same
    over = tc.write_lines(os.path.join(d, "over"), [b"a 3", b"a 1 " + b"x" * (LINE_CAP - 3), b"a 2"], "plain")
    want = bc.host_answer(over, short)
    assert _device_answer(bed_items, over, short) == want and len(want[0]) == 4 + LINE_CAP + 2 + 4
    c = bed_items.counts(reset=True)
    assert (c["handed_over_calls"], c["device_calls"], c["host_calls"], c["device_lines"], c["host_lines"]) == (1, 0, 0, 0, 3)


IRREGULAR = (("blank", b""), ("one_token", b"chr1"), ("leading_zeros", b"chr1 007"), ("plus_sign", b"chr1 +150 x"),
             ("carriage_return", b"chr1 150 x\r"), ("high_byte", b"chr1 150 caf\x80"))


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("k", range(len(IRREGULAR)), ids=[i[0] for i in IRREGULAR])
def test_one_irregular_line_hands_the_rest_to_the_host(files, device_route, monkeypatch, tmp_path, k, where):
    from clairvoyante_amd import utils_v2
    bed_items = device_route
    monkeypatch.setattr(utils_v2, "TRUTH_SLAB_BYTES", 65536)
    name, line = IRREGULAR[k]
    items = list(files["items"][:400])
    at = {"first": 0, "middle": 200, "last": len(items)}[where]
    items.insert(at, line)
    fn = tc.write_lines(str(tmp_path / "items"), items, FORMATS[k % 3], last_newline=(k % 2 == 0))
    bed = files["bed", "plain"]
    want = bc.host_answer(fn, bed)
    got = _device_answer(bed_items, fn, bed)
    assert got[0] == want[0] and got[1] == want[1] and type(got[2]) is type(want[2]) and str(got[2]) == str(want[2])
    assert {"blank": IndexError, "one_token": IndexError}.get(name, type(None)) is type(want[2])
    c = bed_items.counts(reset=True)
    assert c["handed_over_calls"] == 1 and c["device_calls"] == 0 and c["host_calls"] == 0
    if want[2] is None:
        assert c["device_lines"] + c["host_lines"] == 401 and c["host_lines"] >= 401 - at
    if where != "first":
        assert c["device_lines"] > 0
    # counting hands over in the same way
    try:
        tally, raised = bed_items.count_items(fn, bed), None
    except Exception as e:                                   # noqa: BLE001
        tally, raised = None, e
    assert tally == want[1] and type(raised) is type(want[2])
    assert bed_items.counts(reset=True)["handed_over_calls"] == 1


def test_a_bad_bed_line_sends_the_whole_call_to_the_host(files, device_route, tmp_path):
    bed_items = device_route
    bed_lines = list(files["bed_lines"])
    bed_lines.insert(100, b"chr1 0100 2500")
    bed = tc.write_lines(str(tmp_path / "conf.bed"), bed_lines, "plain")
    fn = tc.write_lines(str(tmp_path / "items"), files["items"][:300], "plain")
    want = bc.host_answer(fn, bed)
    assert want[2] is None and _device_answer(bed_items, fn, bed) == want
    c = bed_items.counts(reset=True)
    assert (c["device_lines"], c["handed_over_calls"], c["host_calls"], c["device_calls"]) == (0, 1, 1, 0)


# ---- the entry points called directly: nothing outside the room they are given ---------------------------------------------
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def test_the_keep_kernels_stay_inside_their_room(files):
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    names, bed_off, begin, emax = bc.bed_tables(files["bed", "plain"])
    d_off, d_begin, d_emax = (torch.from_numpy(a).to(dev) for a in (bed_off, begin, emax))
    lines = files["items"][:200]
    raw = b"".join(l + b"\n" for l in lines)
    n = len(raw)
    for shift in (0, 3, 13):                                 # the slab itself off the 16-byte granules
        text = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        text[shift:shift + n].copy_(torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()))
        E = lambda k, dt=torch.int64: torch.full((k,) if isinstance(k, int) else k, -7, dtype=dt, device=dev)
        m = len(lines) + 3
        pos, run, off, ln, tok, info = E(m), E(m, torch.int32), E(m), E(m), E((m, 2)), E(8)
        need = ctypes.c_int64()
        _lib.check(lib.cv_item_lines_workspace(n, m, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        tp = ctypes.c_void_p(text.data_ptr() + shift)
        _lib.check(lib.cv_item_lines_dev(tp, n, m, _ptr(pos), _ptr(run), _ptr(off), _ptr(ln), _ptr(tok), _ptr(info), _ptr(ws), need.value, st))
        used, nl, rows, _s, host, runs = info.cpu().tolist()[:6]
        assert (used, nl, rows, host) == (n, 200, 200, 0) and (pos[rows:] == -7).all() and (tok[runs:] == -7).all()
        t = tok[:runs].cpu().numpy()
        run_ctg = torch.tensor([names.index(raw[o:o + l]) if raw[o:o + l] in names else -1 for o, l in t], dtype=torch.int32, device=dev)
        want = b"".join(l + b"\n" for l in lines if _hit(names, bed_off, begin, emax, l))
        assert 0 < len(want) < n
        _lib.check(lib.cv_items_keep_workspace(rows, ctypes.byref(need)))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        for lead in (16, 21):                                # the destination on and off the granules
            room = torch.full((lead + len(want) + 64,), 0xA5, dtype=torch.uint8, device=dev)
            cnt = E(4)
            _lib.check(lib.cv_items_keep_dev(tp, n, rows, _ptr(pos), _ptr(run), _ptr(off), _ptr(ln), _ptr(run_ctg), runs, len(names),
                                             _ptr(d_off), _ptr(d_begin), _ptr(d_emax), 1, ctypes.c_void_p(room.data_ptr() + lead), len(want),
                                             _ptr(cnt), _ptr(ws), need.value, st))
            got = room.cpu().numpy()
            assert cnt.cpu().tolist() == [200, want.count(b"\n"), len(want), 0]
            assert got[lead:lead + len(want)].tobytes() == want and (got[:lead] == 0xA5).all() and (got[lead + len(want):] == 0xA5).all()
            # room for less than the kept bytes: what does not fit is not written, the counters say what was wanted
            room.fill_(0xA5)
            _lib.check(lib.cv_items_keep_dev(tp, n, rows, _ptr(pos), _ptr(run), _ptr(off), _ptr(ln), _ptr(run_ctg), runs, len(names),
                                             _ptr(d_off), _ptr(d_begin), _ptr(d_emax), 1, ctypes.c_void_p(room.data_ptr() + lead), len(want) - 1,
                                             _ptr(cnt), _ptr(ws), need.value, st))
            got = room.cpu().numpy()
            assert cnt.cpu().tolist()[2] == len(want) and (got[:lead] == 0xA5).all() and (got[lead + len(want) - 1:] == 0xA5).all()


def _hit(names, bed_off, begin, emax, line):
    tok = line.split()
    if tok[0] not in names:
        return False
    c = names.index(tok[0])
    b, e = begin[bed_off[c]:bed_off[c + 1]], emax[bed_off[c]:bed_off[c + 1]]
    k = int(np.searchsorted(b, int(tok[1]), side="right"))
    return k > 0 and e[k - 1] > int(tok[1])


def test_the_sampler_stays_inside_its_room():
    import torch
    from clairvoyante_amd import _lib, bed_items, draws
    lib = _lib.load()
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    want = bed_items.sample_positions_host("chr7", 1, 5001, 0.5, None, 11)
    need = ctypes.c_int64()
    _lib.check(lib.cv_sample_positions_workspace(5000, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    for cap in (len(want), len(want) - 7, 0):
        room = torch.full((cap + 16,), -0x5A5A5A5A, dtype=torch.int64, device=dev)
        cnt = torch.full((2,), -7, dtype=torch.int64, device=dev)
        _lib.check(lib.cv_sample_positions_dev(11, draws.fnv1a32("chr7"), 1, 5000, 0.5, 0, None, None, ctypes.c_void_p(room.data_ptr() + 64), cap,
                                               _ptr(cnt), _ptr(ws), need.value, st))
        got = room.cpu().numpy()
        assert cnt.cpu().tolist() == [cap, len(want)]
        assert np.array_equal(got[8:8 + cap], want[:cap]) and (got[:8] == -0x5A5A5A5A).all() and (got[8 + cap:] == -0x5A5A5A5A).all()


# ---- sampling ---------------------------------------------------------------------------------------------------------------
_host_samples = {}


def _host_sample(start, end, prob, with_bed):
    from clairvoyante_amd import bed_items
    key = (start, end, prob, with_bed)
    if key not in _host_samples:
        _host_samples[key] = bed_items.sample_positions_host("chr21", start, end, prob, bc.sample_intervals() if with_bed else None, 5)
    return _host_samples[key]


@pytest.mark.parametrize("tile", [None, 4096, 1000])
def test_sampling_equals_the_host(device_route, monkeypatch, tile):
    """tiles of 4 096 and 1 000 positions put 25-100 seams in the range, and 1 000 is no multiple of 64"""
    bed_items = device_route
    if tile is not None:
        monkeypatch.setattr(bed_items, "SAMPLE_TILE", tile)
    intervals = bc.sample_intervals()
    assert len(intervals) == 60 and max(e for _b, e in intervals) > 100001
    calls = 0
    for start in (1, 40001):
        for prob in (0.0, 0.01, 0.5, 1.0):
            for with_bed in (True, False):
                want = _host_sample(start, 100001, prob, with_bed)
                got = bed_items.sample_positions(
                    "chr21", start, 100001, prob, intervals if with_bed else None, 5)
                assert got.dtype == np.int64 and np.array_equal(got, want), (start, prob, with_bed)
                calls += 1
    covered = _host_sample(1, 100001, 1.0, True)
    assert 5000 < len(covered) < 60000 and covered[-1] == 100000 and len(_host_sample(1, 100001, 1.0, False)) == 100000
    assert 0.004 * len(covered) < len(_host_sample(1, 100001, 0.01, True)) < 0.02 * len(covered)
    c = bed_items.counts(reset=True)
    assert c["device_calls"] == calls and c["host_calls"] == 0 and c["device_positions"] == 8 * (100000 + 60000)


def test_sampling_with_too_little_room_repeats_the_tile(device_route, monkeypatch):
    bed_items = device_route
    monkeypatch.setattr(bed_items, "SAMPLE_TILE", 30000)
    monkeypatch.setattr(bed_items, "SAMPLE_FIRST_CAP", 5)
    want = _host_sample(1, 100001, 0.5, True)
    assert len(want) > 1000
    assert np.array_equal(bed_items.sample_positions("chr21", 1, 100001, 0.5, bc.sample_intervals(), 5), want)
    assert len(bed_items.sample_positions("chr21", 7, 7, 0.5, None, 5)) == 0 and len(bed_items.sample_positions("chr21", 1, 50, 1.0, [], 5)) == 0


def test_sampling_above_two_to_the_32(device_route):
    """the position is two counter words of the draw: the high one must reach the kernel"""
    bed_items = device_route
    want = bed_items.sample_positions_host("chr21", 5000000000, 5000003000, 0.5, None, 5)
    low = bed_items.sample_positions_host("chr21", 5000000000 - (1 << 32), 5000003000 - (1 << 32), 0.5, None, 5)
    assert 1300 < len(want) < 1700 and not np.array_equal(want - (1 << 32), low)
    assert np.array_equal(bed_items.sample_positions("chr21", 5000000000, 5000003000, 0.5, None, 5), want)


def test_random_sampling_prints_the_same_under_both_routes(tmp_path, monkeypatch, capfdbinary):
    from clairvoyante_amd import RandomSampling, bed_items
    ref = str(tmp_path / "ref.fa")
    with open(ref + ".fai", "wb") as f:
        f.write(b"chr21\t100000\t7\t60\t61\n")
    bed = str(tmp_path / "s.bed")
    with open(bed, "wb") as f:
        f.write(b"".join(b"chr21\t%d\t%d\n" % (b, e + 1) for b, e in bc.sample_intervals()))
    out = {}
    for how in ("host", "device"):
        monkeypatch.setenv("CV_BED_ITEMS", how)
        bed_items.counts(reset=True)
        monkeypatch.setattr(sys, "argv", ["RandomSampling.py", "--ref_fn", ref, "--ctgName", "chr21", "--bed_fn", bed, "--seed", "5",
                                          "--candidates", "100", "--genomeSize", "1000"])
        capfdbinary.readouterr()
        RandomSampling.main()
        out[how] = capfdbinary.readouterr().out
        c = bed_items.counts(reset=True)
        assert (c["device_calls"], c["host_calls"]) == ((1, 0) if how == "device" else (0, 1))
    want = _host_sample(1, 100000, 0.2, True)
    assert out["device"] == out["host"] == b"".join(b"chr21\t%d\n" % p for p in want) and len(want) > 1000
