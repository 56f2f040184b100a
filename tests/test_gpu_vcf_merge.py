"""The VCF merge on the device (csrc/cv_vcfmerge_dev.hip, CV_VCF_MERGE=device; opt-in).  The host route of vcf_merge.py is
the definition: the .vcf.gz and the .tbi of the device route equal its files byte for byte, with vcf_merge.counts() showing
where the work ran, so that neither a silent hand-over nor a dropped record can pass.  The arrays of the two entry points
are compared with cv_vcf_merge_host_form / cv_vcf_windows_host_form (held to the definition and run under the sanitizers
by test_vcf_merge_core_host.py), with canaries behind every output array.

vm_gather assembles the text of 64 output records in an LDS tile when it is at most TILE_TEXT = 16 384 bytes, and writes
record by record otherwise: tiles of exactly 16 384 and of 16 385 bytes, at output phases 0 and 15, a call whose three
tiles take the two paths in turn, and an out_cap too small for the text (a range that does not fit is not written, every
other output is unchanged) -- inputs from tests/vcf_merge_big_cases.py.  The sizes the kernels were written for, past
their launch caps, are in test_gpu_launch_caps.py, the gather past 2^32 bytes in test_gpu_past_4gib.py.
Seconds on one MI355X (pytest --durations): each of these eleven cases under 0.005."""
import ctypes
import os

import numpy as np
import pytest

import vcf_merge_cases as vc

pytestmark = pytest.mark.gpu


def _both(tmp_path, monkeypatch, files, fai, block, threads):
    """merge on the host route and on the device route -> (host bytes, device bytes) of (.vcf.gz, .tbi), device counters"""
    from clairvoyante_amd import vcf_merge
    out = {}
    for route in ("host", "device"):
        monkeypatch.setenv("CV_VCF_MERGE", route)
        fn = str(tmp_path / ("%s.vcf.gz" % route))
        vcf_merge.counts(reset=True)
        got = vcf_merge.merge(files, fn, fai_fn=fai, block=block, threads=threads)
        out[route] = (open(fn, "rb").read(), open(fn + ".tbi", "rb").read(), vcf_merge.counts(), got)
    return out


def _device_only(c, total):
    return (c["device_calls"], c["host_calls"], c["handed_over_calls"], c["device_records"], c["host_records"]) == (1, 0, 0, total, 0)


@pytest.mark.parametrize("total", vc.COUNTS)
@pytest.mark.parametrize("block", vc.BLOCKS)
def test_the_device_route_writes_the_host_routes_bytes(total, block, tmp_path, monkeypatch):
    files, fai, _per = vc.build(tmp_path, total)
    out = _both(tmp_path, monkeypatch, files, fai, block, 1 if (total + (block or 0)) % 2 else 16)
    assert out["device"][0] == out["host"][0] and out["device"][1] == out["host"][1]
    assert _device_only(out["device"][2], total), out["device"][2]
    assert out["device"][3]["route"] == "device" and out["device"][3]["records"] == total


@pytest.mark.parametrize("form", ["gz", "bgzf"])
@pytest.mark.parametrize("total,threads", [(65, 16), (2000, 1)])
def test_compressed_inputs(form, total, threads, tmp_path, monkeypatch):
    files, fai, _per = vc.build(tmp_path, total, form=form)
    out = _both(tmp_path, monkeypatch, files, fai, 4096, threads)
    assert out["device"][0] == out["host"][0] and out["device"][1] == out["host"][1]
    assert _device_only(out["device"][2], total), out["device"][2]


HANDED_OVER = {
    "END=": vc.rec("chr1", 15000000, "A", "<DEL>", info="SVTYPE=DEL;END=15100000"),
    "carriage return": vc.rec("chr1", 15000000, "A", "C")[:-1] + b"\r\n",
    "over 8 KiB": vc.rec("chr1", 15000000, "A" * 8200, "A"),
    "no last newline": None,
    "7 columns": b"chr1\t15000000\t.\tA\tC\t3\t.\n",
}


@pytest.mark.parametrize("what", sorted(HANDED_OVER))
def test_what_the_device_does_not_vouch_for_goes_to_the_host_loop(what, tmp_path, monkeypatch):
    """the same bytes, or the same exception, and counted as handed over"""
    from clairvoyante_amd import vcf_merge
    files, fai, per = vc.build(tmp_path, 257)
    body = b"".join(per[3])
    body = body[:-1] if HANDED_OVER[what] is None else body + HANDED_OVER[what]
    vc.write_file(files[3], vc.HEADER + body, "plain")
    if what == "7 columns":
        for route in ("host", "device"):
            monkeypatch.setenv("CV_VCF_MERGE", route)
            vcf_merge.counts(reset=True)
            with pytest.raises(ValueError, match="8 columns"):
                vcf_merge.merge(files, str(tmp_path / "o.vcf.gz"), fai_fn=fai)
            c = vcf_merge.counts()
            assert c["device_calls"] == 0 and c["device_records"] == 0 and c["handed_over_calls"] == (route == "device")
        return
    out = _both(tmp_path, monkeypatch, files, fai, 512, 4)
    assert out["device"][0] == out["host"][0] and out["device"][1] == out["host"][1]
    c = out["device"][2]
    total = 257 + (HANDED_OVER[what] is not None)
    assert (c["device_calls"], c["host_calls"], c["handed_over_calls"], c["device_records"], c["host_records"]) == (0, 1, 1, 0, total), c


def test_a_header_mismatch_raises_on_the_device_route_too(tmp_path, monkeypatch):
    from clairvoyante_amd import vcf_merge
    files, fai, per = vc.build(tmp_path, 65)
    vc.write_file(files[3], vc.HEADER.replace(b"SAMPLE", b"OTHER") + b"".join(per[3]), "plain")
    monkeypatch.setenv("CV_VCF_MERGE", "device")
    with pytest.raises(ValueError, match="chr1_10000000_20000000"):
        vcf_merge.merge(files, str(tmp_path / "o.vcf.gz"), fai_fn=fai)


# ---- the two entry points through the C ABI ---------------------------------------------------------------------------------
CANARY = 0x5A


class _Guarded(object):
    """a device array of `count` items of `dtype` with 256 canary bytes on either side, at a chosen phase"""

    def __init__(self, torch, dev, count, dtype, phase=0):
        self.size = count * np.dtype(dtype).itemsize
        self.buf = torch.full((self.size + 512 + 16,), CANARY, dtype=torch.uint8, device=dev)
        self.at = 256 + (phase - (self.buf.data_ptr() + 256)) % 16
        self.dtype, self.count = dtype, count
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.at)

    def read(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.at] == CANARY).all() and (b[self.at + self.size:] == CANARY).all(), "a canary was overwritten"
        return b[self.at:self.at + self.size].view(self.dtype)


def _dev_call(a, phase=0, ws_shift=0, ws_short=0, out_cap=None):
    """cv_vcf_merge_dev + cv_vcf_windows_dev over line_arrays' dict, every output guarded -> dict like vc.host_form's;
    out_cap: the room the call is told the output text has (default: all of it; what is not written holds CANARY)"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    P = _lib.ptr
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    n, nrank, n_text = a["n"], a["nrank"], a["n_text"]
    text = T(a["text"])
    assert text.data_ptr() % 16 == 0
    pos, run, off, ln, rr = T(a["pos"]), T(a["run"]), T(a["off"]), T(a["len"]), T(a["run_rank"])
    G = lambda count, dt, ph=0: _Guarded(torch, dev, count, dt, ph)
    g = {"srank": G(max(n, 1), np.int32), "sbeg": G(max(n, 1), np.int64), "send": G(max(n, 1), np.int64), "ooff": G(n + 1, np.int64),
         "text": G(n_text, np.uint8, phase), "chunks": G(4 * max(n, 1), np.int64), "stats": G(4 * nrank, np.int64), "info": G(8, np.int64)}
    need = _lib.workspace(lib.cv_vcf_merge_workspace, n)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256 + ws_shift
    st = _lib.stream_arg(dev)
    _lib.check(lib.cv_vcf_merge_dev(P(text), n_text, n, P(pos), P(run), P(off), P(ln), P(rr), a["nruns"], nrank, g["srank"].ptr, g["sbeg"].ptr,
                                    g["send"].ptr, g["ooff"].ptr, g["text"].ptr, n_text if out_cap is None else out_cap, g["chunks"].ptr, g["stats"].ptr, g["info"].ptr,
                                    ctypes.c_void_p(base), need - ws_short, st))
    torch.cuda.synchronize()
    o = {k: v.read().copy() for k, v in g.items()}
    o["chunks"] = o["chunks"].reshape(4, max(n, 1))
    o["stats"] = o["stats"].reshape(4, nrank)
    count, maxend = o["stats"][2], o["stats"][3]
    o["win_off"] = np.concatenate(([0], np.cumsum(np.where(count > 0, ((maxend - 1) >> 14) + 1, 0)))).astype(np.int64)
    nwin = int(o["win_off"][-1])
    win = G(max(nwin, 1), np.int64)
    _lib.check(lib.cv_vcf_windows_dev(n, g["srank"].ptr, g["sbeg"].ptr, g["send"].ptr, g["ooff"].ptr, nrank, P(T(o["win_off"])), win.ptr,
                                      nwin, st))
    torch.cuda.synchronize()
    o["win"] = win.read().copy()
    return o


def _same(o, w, n, n_text):
    nc, nwin = int(w["info"][1]), int(w["win_off"][-1])
    assert o["info"].tolist() == w["info"].tolist()
    for k in ("srank", "sbeg", "send"):
        assert np.array_equal(o[k][:n], w[k][:n]), k
    assert np.array_equal(o["ooff"], w["ooff"]) and np.array_equal(o["stats"], w["stats"]) and np.array_equal(o["win_off"], w["win_off"])
    assert np.array_equal(o["chunks"][:, :nc], w["chunks"][:, :nc]) and np.array_equal(o["win"][:nwin], w["win"][:nwin])
    nbytes = int(w["info"][2])                              # (a line not vouched for takes no room: the text ends sooner)
    assert nbytes <= n_text and o["text"][:nbytes].tobytes() == w["text"][:nbytes].tobytes()


@pytest.mark.parametrize("total", vc.COUNTS)
@pytest.mark.parametrize("phase", [0, 1, 15])
def test_the_entry_points_equal_the_host_forms_and_leave_the_canaries(total, phase):
    a = vc.line_arrays(vc.records(total))
    _same(_dev_call(a, phase), vc.host_form(a), a["n"], a["n_text"])


def test_long_records_take_the_wave_per_record_path():
    """tiles of more than 16 KiB (64 records of 300 to 700 bytes), and a line not vouched for among them"""
    per = [[vc.rec("chr2", 100 + 37 * (k % 50), "ACGT"[k % 4] * (1 + k % 300), "A", info="LENGUESS=%d" % (k % 9 + 1),
                   gt="0/1" + ":" + "x" * (200 + (k * 7) % 300)) for k in range(200)]]
    a = vc.line_arrays(per)
    for phase in (0, 7):
        _same(_dev_call(a, phase), vc.host_form(a), a["n"], a["n_text"])
    per[0].insert(70, vc.rec("chr2", 5, "A", "C", info="DP=3;END=9"))
    a = vc.line_arrays(per)
    o, w = _dev_call(a), vc.host_form(a)
    assert o["info"][0] == 1 == w["info"][0]
    _same(o, w, a["n"], a["n_text"])


# ---- the gather's tile line (TILE_TEXT = 16 384 bytes of 64 records), and an output that is too small ---------------------------
@pytest.mark.parametrize("total,phase", [(16384, 0), (16384, 15), (16385, 0), (16385, 15)])
def test_a_tile_of_exactly_16384_bytes_and_of_one_more(total, phase):
    """16 384 bytes fill the LDS tile (at phase 15 it ends at byte 16 399 of its 16 416); 16 385 take the wave-per-record path"""
    import vcf_merge_big_cases as B
    a = B.tile_case(total)
    assert a["n"] == 64 and a["n_text"] == total and B.TILE_TEXT == 16384
    _same(_dev_call(a, phase), vc.host_form(a), a["n"], a["n_text"])


@pytest.mark.parametrize("phase", [0, 3, 15])
def test_both_paths_write_neighbouring_ranges_of_one_output(phase):
    import vcf_merge_big_cases as B
    a = B.three_tile_case()
    o, w = _dev_call(a, phase), vc.host_form(a)
    tiles = np.diff(w["ooff"][[0, 64, 128, 192]])
    assert tiles[0] < B.TILE_TEXT < tiles[1] and tiles[2] < B.TILE_TEXT
    _same(o, w, a["n"], a["n_text"])


@pytest.mark.parametrize("which", ["the first tile's end", "one byte less", "the whole text minus 1", "nothing"])
def test_an_output_too_small_for_the_text(which):
    """nothing of a tile's range that does not fit below out_cap is written: the text is the host form's over a buffer of
    the same sentinel, every other output is what it is with room for all"""
    import vcf_merge_big_cases as B
    a = B.three_tile_case()
    full = vc.host_form(a)
    first = int(full["ooff"][64])
    cap, kept = {"the first tile's end": (first, 1), "one byte less": (first - 1, 0), "the whole text minus 1": (a["n_text"] - 1, 2),
                 "nothing": (0, 0)}[which]
    o, w = _dev_call(a, 5, out_cap=cap), vc.host_form(a, out_cap=cap, fill=CANARY)
    edge = int(full["ooff"][64 * kept])
    assert np.array_equal(o["text"], w["text"][:a["n_text"]])
    assert np.array_equal(o["text"][:edge], full["text"][:edge]) and (o["text"][edge:] == CANARY).all() and edge <= cap
    for k in ("info", "ooff", "srank", "sbeg", "send", "stats", "win_off", "win"):
        assert np.array_equal(o[k][:len(full[k])], full[k][:len(o[k])]) and np.array_equal(w[k], full[k]), k
    nc = int(full["info"][1])
    assert np.array_equal(o["chunks"][:, :nc], full["chunks"][:, :nc]) and np.array_equal(w["chunks"], full["chunks"])


def test_workspaces_and_arguments_are_refused_with_a_message():
    from clairvoyante_amd import _lib
    a = vc.line_arrays(vc.records(65))
    with pytest.raises(_lib.CvError, match="workspace holds"):
        _dev_call(a, ws_short=1)
    with pytest.raises(_lib.CvError, match="256-byte aligned"):
        _dev_call(a, ws_shift=8)
    lib = _lib.load()
    need = ctypes.c_int64()
    assert lib.cv_vcf_merge_workspace(-1, ctypes.byref(need)) != 0 and b"out of range" in lib.cv_last_error()
    assert lib.cv_vcf_merge_workspace((1 << 30) + 1, ctypes.byref(need)) != 0
    b = dict(a, nrank=0)
    with pytest.raises(_lib.CvError, match="contig ranks"):
        vc.host_form(b)
