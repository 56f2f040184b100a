"""Text tensor rows written on the device (csrc/cv_rowtext_dev.hip) against the host formatter: through the C ABI
(cv_tensor_rows_text_dev == cv_format_tensor_row + "\\n", joined), through pileup.format_rows_device (batches with a row
the device does not vouch for come back as format_rows' bytes and are counted on the host side), and through CreateTensor
over the committed pileup fixtures for its three sinks: the same text, the same BGZF file, the same VCF behind it."""
import ctypes
import gzip
import io
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden", "pileup")
FAKE = "%s %s" % (sys.executable, os.path.join(HERE, "golden", "fake_samtools.py"))
pytestmark = pytest.mark.gpu

CANARY = 256
NV = 33 * 16
EDGE_VALUES = (0.0, 9.0, 10.0, 99.0, 100.0, 250.0, 999.0, 1000.0, 65535.0, 16777215.0, -0.0)
NOT_VOUCHED = (-1.0, 0.5, 16777216.0, float("nan"), float("inf"))


def make_ref(n, seed=3):
    """lower and upper case, N: the bytes must come out as they are"""
    return bytes(np.random.RandomState(seed).choice(np.frombuffer(b"ACGTNacgtn", dtype=np.uint8), n))


def make_counts(rows, seed):
    """raw pileup-like counts: mostly small, every digit count present"""
    rng = np.random.RandomState(seed)
    x = rng.randint(0, 60, size=(rows, 33, 4, 4)).astype(np.float32)
    big = rng.rand(rows, 33, 4, 4) < 0.05
    x[big] = (10 ** rng.randint(0, 8, size=int(big.sum()))).astype(np.float32)
    x[rng.rand(rows, 33, 4, 4) < 0.5] = 0
    return x


def host_rows(ctg, centres, ref, first0, counts):
    """cv_format_tensor_row + "\\n" per row; seq = what of [new_pos - 17, new_pos + 16) lies inside the window"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(16384)
    cb = ctg.encode()
    counts = np.ascontiguousarray(counts, dtype=np.float32)
    out = []
    for k, c in enumerate(centres):
        p = int(c) - first0
        seq = ref[max(p - 17, 0):max(p + 16, 0)]
        n = lib.cv_format_tensor_row(cb, int(c), seq, len(seq), counts[k].ctypes.data_as(ctypes.c_void_p), buf, len(buf))
        assert n > 0
        out.append(buf.raw[:n] + b"\n")
    return out


def dev_rows(ctg, centres, ref, first0, counts, write=True, slack=0):
    """cv_tensor_rows_text_dev -> (text bytes, off [rows + 1], status [rows], the CANARY bytes behind the text).  The text
    buffer holds exactly off[rows] (+ slack) bytes in front of the canary and starts at an odd address."""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    rows = len(centres)
    cb = ctg.encode()
    dev = torch.device("cuda")
    cen = torch.from_numpy(np.ascontiguousarray(centres, dtype=np.int64)).to(dev)
    cnt = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.float32).reshape(rows, 33, 4, 4)).to(dev)
    rf = torch.from_numpy(np.frombuffer(ref, dtype=np.uint8).copy()).to(dev)
    off = torch.full((rows + 1,), -7, dtype=torch.int64, device=dev)
    status = torch.full((max(rows, 1),), 9, dtype=torch.uint8, device=dev)
    need = ctypes.c_int64(0)
    _lib.check(lib.cv_tensor_rows_text_workspace(rows, ctypes.byref(need)))
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(text, cap):
        _lib.check(lib.cv_tensor_rows_text_dev(cb, len(cb), ptr(cen), rows, ptr(rf) if len(ref) else None, first0, len(ref), ptr(cnt),
                                               ptr(off), ptr(status), text, cap, ptr(ws), ws.numel(), stream))
        torch.cuda.synchronize()
    call(None, 0)
    off0, status0 = off.cpu().numpy().copy(), status.cpu().numpy()[:rows].copy()
    if not write:
        return b"", off0, status0, b""
    total = int(off0[rows]) + slack
    room = torch.full((3 + total + CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    text = room[3:]                                          # an odd address: every 16-byte phase occurs among the rows
    call(ctypes.c_void_p(text.data_ptr()), total)
    assert np.array_equal(off.cpu().numpy(), off0) and np.array_equal(status.cpu().numpy()[:rows], status0), \
        "the length-only call and the writing call disagree"
    got = room.cpu().numpy().tobytes()
    assert got[:3] == b"\xa5" * 3, "bytes in front of the text were written"
    return got[3:3 + total], off0, status0, got[3 + total:]


def check_against_host(ctg, centres, ref, first0, counts):
    want = host_rows(ctg, centres, ref, first0, counts)
    text, off, status, tail = dev_rows(ctg, centres, ref, first0, counts)
    assert tail == b"\xa5" * CANARY, "the canary behind the text was written"
    assert not status.any()
    lens = np.array([len(w) for w in want], dtype=np.int64)
    assert np.array_equal(off, np.concatenate(([0], np.cumsum(lens))))
    assert off[len(centres)] == sum(len(w) for w in want)
    assert text == b"".join(want)
    return text


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 257])
def test_row_counts(rows):
    ref = make_ref(3000)
    centres = 20 + np.sort(np.random.RandomState(rows).choice(2900, rows, replace=False)).astype(np.int64)
    text = check_against_host("ctgA", centres, ref, 0, make_counts(rows, 100 + rows))
    assert text.count(b"\n") == rows


def test_values_and_whole_rows():
    """every edge value at every place of a lane's run and of the row; the shortest and the longest row"""
    rows = []
    for i, v in enumerate(EDGE_VALUES):
        a = np.zeros(NV, dtype=np.float32); a[[0, 8, 9, 263, 521, 522, NV - 1]] = v; rows.append(a)
        b = make_counts(1, 7 + i).reshape(NV); b[i::len(EDGE_VALUES)] = v; rows.append(b)
        rows.append(np.full(NV, v, dtype=np.float32))
    rows.append(np.zeros(NV, dtype=np.float32))
    rows.append(np.full(NV, 16777215.0, dtype=np.float32))
    rows.append(np.resize(np.asarray(EDGE_VALUES, dtype=np.float32), NV))
    counts = np.stack(rows)
    centres = 100 + 3 * np.arange(len(rows), dtype=np.int64)
    text = check_against_host("ctgA", centres, make_ref(500), 0, counts)
    lines = text.split(b"\n")[:-1]
    assert len(lines[-3]) == len(b"ctgA %d " % int(centres[-3])) + 33 + NV * 4       # all zeros: " 0.0"
    assert len(lines[-2]) == len(b"ctgA %d " % int(centres[-2])) + 33 + NV * 11      # all " 16777215.0"
    assert b"-" not in text                                                          # -0.0 prints 0.0


@pytest.mark.parametrize("ctg_len", [1, 5, 255])
def test_centres_contigs_and_windows(ctg_len):
    ref = make_ref(700, seed=ctg_len)
    counts = make_counts(12, 40 + ctg_len)
    centres = np.array([int("1234567890123"[:d]) for d in range(1, 13)], dtype=np.int64)     # 1 .. 12 digits
    ctg = ("chr21" * 51)[:ctg_len]
    check_against_host(ctg, centres, ref, 0, counts)
    # a window that does not start at 0, and ends 5 bytes behind one centre: that row's seq is short
    first0 = 1000
    near = first0 + np.array([17, 18, 40, 300, 683, 690, 694, 695, 699, 700, 716, 717], dtype=np.int64)
    text = check_against_host(ctg, near, ref, first0, counts)
    row = text.split(b"\n")[7].split(b" ")                   # centre 1695: new_pos 695, the window ends at 700
    assert row[1] == b"1695" and row[2] == ref[678:700] and len(row[2]) == 22
    assert row[2] != row[2].upper()                          # lower case is kept


def test_contig_name_of_256_bytes_goes_to_the_host():
    counts = make_counts(5, 1)
    centres = np.arange(100, 105, dtype=np.int64)
    _text, off, status, _tail = dev_rows("x" * 256, centres, make_ref(300), 0, counts, write=False)
    assert (status == 1).all() and not off.any()
    text, off, status, tail = dev_rows("x" * 256, centres, make_ref(300), 0, counts, slack=64)
    assert (status == 1).all() and not off.any() and text == b"\xa5" * 64 and tail == b"\xa5" * CANARY


def test_length_only_call_and_a_cap_too_small():
    counts = make_counts(65, 2)
    centres = np.arange(100, 165, dtype=np.int64)
    ref = make_ref(300)
    want = host_rows("ctgA", centres, ref, 0, counts)
    _t, off, status, _c = dev_rows("ctgA", centres, ref, 0, counts, write=False)
    assert off[65] == sum(len(w) for w in want) and not status.any()
    # text_cap one row short: the rows that fit are written, the last one is not, nothing behind the cap is
    text, off, status, tail = dev_rows("ctgA", centres, ref, 0, counts, slack=-len(want[-1]))
    assert text == b"".join(want[:-1]) and tail == b"\xa5" * CANARY


@pytest.mark.parametrize("bad", NOT_VOUCHED)
def test_rows_the_device_does_not_vouch_for(bad):
    from clairvoyante_amd import pileup
    import torch
    rows = 9
    counts = make_counts(rows, 11)
    flat = counts.reshape(rows, NV)
    flat[2, 0] = bad; flat[4, NV - 1] = bad; flat[5, 300] = bad
    centres = np.arange(200, 200 + rows, dtype=np.int64)
    ref = make_ref(400)
    text, off, status, tail = dev_rows("ctgA", centres, ref, 0, counts)
    assert status.tolist() == [0, 0, 1, 0, 1, 1, 0, 0, 0] and tail == b"\xa5" * CANARY
    good = [w for w, s in zip(host_rows("ctgA", centres, ref, 0, counts), status) if not s]
    assert text == b"".join(good)                            # the neighbours are written, the row itself has length 0
    assert all(off[r + 1] == off[r] for r in (2, 4, 5))
    # the wrapper: the batch comes back as format_rows' bytes and counts on the host side
    pileup.row_format_counts(reset=True)
    blocks = list(pileup.format_rows_device("ctgA", centres, ref, 0, torch.from_numpy(counts).cuda()))
    want = b"".join(r + b"\n" for r in pileup.format_rows("ctgA", centres, ref, 0, counts))
    assert b"".join(blocks) == want and len(blocks) == 1
    assert pileup.row_format_counts() == {"host": rows, "device": 0}


def test_wrapper_batches_and_counts():
    from clairvoyante_amd import pileup
    import torch
    rows = 150
    counts = make_counts(rows, 5)
    counts.reshape(rows, NV)[130, 7] = 0.5                   # third batch of 64: the host's
    centres = 50 + 2 * np.arange(rows, dtype=np.int64)
    ref = make_ref(500)
    want = [r + b"\n" for r in pileup.format_rows("ctgA", centres, ref, 0, counts)]
    pileup.row_format_counts(reset=True)
    t = torch.from_numpy(counts).cuda()
    blocks = list(pileup.format_rows_device("ctgA", centres, ref, 0, t, batch=64))
    assert blocks == [b"".join(want[0:64]), b"".join(want[64:128]), b"".join(want[128:])]
    assert pileup.row_format_counts() == {"host": 22, "device": 128}
    # the reference already in HBM, a shifted window
    sl = torch.from_numpy(np.frombuffer(ref[40:], dtype=np.uint8).copy()).cuda()
    got = b"".join(pileup.format_rows_device("ctgA", centres[10:100], sl, 40, t[10:100]))
    assert got == b"".join(r + b"\n" for r in pileup.format_rows("ctgA", centres[10:100], ref[40:], 40, counts[10:100]))
    with pytest.raises(Exception):
        next(pileup.format_rows_device("ctgA", centres, ref, 0, torch.from_numpy(counts)))      # tensors not on a GPU


# ---- CreateTensor over the committed fixtures ---------------------------------------------------------------------------
def ct_args(name, tmp_path, out, **over):
    base = os.path.join(G, name)
    a = dict(bam_fn=base + ".sam", ref_fn=base + ".fa", can_fn=base + ".can", tensor_fn=out if out == "PIPE" else str(tmp_path / out),
             minMQ=0, ctgName="ctgA", ctgStart=None, ctgEnd=None, samtools=FAKE, dcov=250, minCoverage=0,
             considerleftedge=True)
    a.update(over)
    return types.SimpleNamespace(**a)


def run_ct(monkeypatch, side, args):
    """OutputAlnTensor under CV_ROW_FORMAT=side -> (text written to standard output or b"", rows per side)"""
    from clairvoyante_amd import CreateTensor, pileup
    monkeypatch.setenv("CV_ROW_FORMAT", side)
    out = io.BytesIO()
    monkeypatch.setattr(sys, "stdout", types.SimpleNamespace(buffer=out, write=lambda s: None, flush=lambda: None))
    pileup.row_format_counts(reset=True)
    res = CreateTensor.OutputAlnTensor(args)
    monkeypatch.undo()
    return out.getvalue(), pileup.row_format_counts(), len(res["centers"])


@pytest.mark.parametrize("name,over", [("plain", {}), ("noisy", {"ctgStart": 0, "ctgEnd": 2000, "minCoverage": 2, "dcov": 3}),
                                       ("long", {}), ("sparse", {})])
def test_createtensor_writes_the_same_bytes_on_either_side(name, over, tmp_path, monkeypatch):
    texts = {}
    for side in ("host", "device"):
        piped, counts, rows = run_ct(monkeypatch, side, ct_args(name, tmp_path, "PIPE", **over))
        assert rows > 20 and counts == ({"host": rows, "device": 0} if side == "host" else {"host": 0, "device": rows})
        gz = ct_args(name, tmp_path, side + ".gz", **over)
        _, counts, _ = run_ct(monkeypatch, side, gz)
        assert counts[side] == rows and sum(counts.values()) == rows
        bg = ct_args(name, tmp_path, side + ".bgzf.gz", bgzf=True, **over)
        _, counts, _ = run_ct(monkeypatch, side, bg)
        assert counts[side] == rows and sum(counts.values()) == rows
        texts[side] = (piped, gzip.open(gz.tensor_fn, "rb").read(), open(bg.tensor_fn, "rb").read())
        assert piped.count(b"\n") == rows
    host, device = texts["host"], texts["device"]
    assert device[0] == host[0] and device[1] == host[1] == host[0]
    assert device[2] == host[2] and gzip.decompress(device[2]) == host[0]              # the BGZF FILE bytes are equal


def test_callvar_reads_the_device_written_file(tmp_path, monkeypatch, oracle):
    sys.path.insert(0, HERE)
    from clairvoyante_amd import callVar, clairvoyante_v3
    from common import bench_params
    m = clairvoyante_v3.Clairvoyante()
    m.init()
    m.setParameters(bench_params(oracle, "full", seed=11))
    chk = str(tmp_path / "model-000001")
    m.saveParameters(chk)
    m.close()
    vcf = {}
    for side in ("host", "device"):
        a = ct_args("plain", tmp_path, side + ".bgzf.gz", bgzf=True)
        _, counts, rows = run_ct(monkeypatch, side, a)
        assert counts[side] == rows > 20
        v = types.SimpleNamespace(tensor_fn=a.tensor_fn, chkpnt_fn=chk, call_fn=str(tmp_path / (side + ".vcf")), qual=None,
                                  sampleName="SAMPLE", ref_fn=os.path.join(G, "plain.fa"), threads=None, showRef=False, v3=True,
                                  v2=False, slim=False)
        callVar.Run(v)
        vcf[side] = open(v.call_fn).read()
    assert vcf["device"] == vcf["host"] and len([l for l in vcf["host"].splitlines() if not l.startswith("#")]) > 10


def test_an_unknown_side_raises(tmp_path, monkeypatch):
    from clairvoyante_amd import CreateTensor
    monkeypatch.setenv("CV_ROW_FORMAT", "gpu")
    with pytest.raises(ValueError, match="host or device"):
        CreateTensor.OutputAlnTensor(ct_args("plain", tmp_path, "bad.gz"))
