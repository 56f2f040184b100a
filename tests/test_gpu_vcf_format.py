"""VCF records written on the device (csrc/cv_vcf_dev.hip) against the host formatter.  Through the C ABI:
cv_vcf_records_dev == cv_vcf_records_host_form (text, off, status, info: the same core, on either side) and every DEVICE
record == cv_format_vcf of that candidate alone.  Through the drivers: callVar / callVarBam under CV_VCF_FORMAT=host and
=device write byte-identical VCF files, the device side takes every batch of a clean input, a batch with a candidate the
device does not vouch for goes back to the host whole, and what the host refuses it refuses on either route."""
import ctypes
import os
import shutil
import types

import numpy as np
import pytest

import common

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden", "pileup")
pytestmark = pytest.mark.gpu

CANARY = 256
NONE, DEVICE, HOST = 0, 1, 2
SEQ = "ACGTACGTACGTACGTACGTACGTACGTACGTA"


# ---- batches ---------------------------------------------------------------------------------------------------------------
class Batch(object):
    """candidates as cv_format_vcf takes them: call [n,8] int32, qual [n,4] fp32, x [n,33,4,4] fp32, tokens = [(contig,
    position, sequence)] as bytes"""

    def __init__(self, call, qual, x, tokens):
        self.call, self.qual, self.x, self.tokens = call, qual, x, list(tokens)
        self.n = len(self.tokens)
        parts, off = [], 0
        self.meta = np.empty((self.n, 6), dtype=np.int64)
        for i, t in enumerate(self.tokens):
            for k in range(3):
                self.meta[i, 2 * k] = off; self.meta[i, 2 * k + 1] = len(t[k])
                parts.append(t[k]); off += len(t[k])
        self.buf = np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy()


def random_batch(n, seed, planted=()):
    """clean candidates (every 19th at depth 0), then `planted`: (index, function of (call, qual, x, tokens))"""
    rng = np.random.RandomState(seed)
    call = np.zeros((n, 8), dtype=np.int32)
    call[:, 0] = rng.randint(0, 4, n); call[:, 1] = rng.randint(0, 2, n); call[:, 2] = rng.randint(0, 6, n)
    call[:, 3] = rng.randint(0, 4, n); call[:, 4] = rng.randint(0, 4, n)
    p = np.sort(rng.rand(n, 2).astype(np.float32) * np.float32(0.999) + np.float32(1e-6), axis=1)
    qual = np.zeros((n, 4), dtype=np.float32)
    qual[:, 0] = p[:, 1]; qual[:, 1] = p[:, 0]
    qual[:, 2] = rng.randint(1, 90, n)
    qual[7::19, 2] = 0
    x = rng.randint(-20, 60, size=(n, 33, 4, 4)).astype(np.float32)
    x[rng.rand(n, 33, 4, 4) < 0.4] = 0
    letters = np.frombuffer(b"ACGTacgt", dtype=np.uint8)
    tokens = [[b"chr%d" % (1 + i % 23), b"%d" % (1000 + 13 * i + int(rng.randint(0, 9))), bytes(rng.choice(letters, 17 + (i * 7) % 17))]
              for i in range(n)]
    for i, f in planted:
        f(call[i], qual[i], x[i], tokens[i])
    return Batch(call, qual, x, tokens)


def _lib():
    from clairvoyante_amd import _lib as L
    return L, L.load()


def host_one(b, i, show_ref, qual):
    """cv_format_vcf over candidate i alone -> its bytes (b"" for no record), or the CvError it raises"""
    L, lib = _lib()
    out = ctypes.create_string_buffer(1024)
    nlen, nrec = ctypes.c_int64(), ctypes.c_int64()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    meta = np.ascontiguousarray(b.meta[i:i + 1])
    rc = lib.cv_format_vcf(p(b.call[i:i + 1]), p(b.qual[i:i + 1]), 1, p(b.x[i:i + 1]), None, p(b.buf), p(meta), None, int(show_ref),
                           0 if qual is None else 1, 0 if qual is None else qual, out, 1024, ctypes.byref(nlen), ctypes.byref(nrec))
    L.check(rc)
    return out.raw[:nlen.value]


def host_batch(b, show_ref, qual):
    """cv_format_vcf over the whole batch in ONE call -> its bytes (a batch without a candidate the host refuses)"""
    L, lib = _lib()
    cap = b.n * (int(b.meta[:, 1].max()) + 160)
    out = ctypes.create_string_buffer(cap)
    nlen, nrec = ctypes.c_int64(), ctypes.c_int64()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    L.check(lib.cv_format_vcf(p(b.call), p(b.qual), b.n, p(b.x), None, p(b.buf), p(b.meta), None, int(show_ref), 0 if qual is None else 1,
                              0 if qual is None else qual, out, cap, ctypes.byref(nlen), ctypes.byref(nrec)))
    return out.raw[:nlen.value], nrec.value


def _indexed(b, rng, xrow, pos_row):
    """the batch with its tensors / its meta rows stored in another order, and the index arrays that name them"""
    x, meta, xr, pr = b.x, b.meta, None, None
    if xrow:
        xr = rng.permutation(b.n).astype(np.int64)
        x = np.empty_like(b.x); x[xr] = b.x
    if pos_row:
        pr = rng.permutation(b.n).astype(np.int64)
        meta = np.empty_like(b.meta); meta[pr] = b.meta
    return np.ascontiguousarray(x), np.ascontiguousarray(meta), xr, pr


def host_form(b, show_ref=True, qual=None, xrow=False, pos_row=False, seed=5):
    """cv_vcf_records_host_form -> (text, off, status, info)"""
    L, lib = _lib()
    x, meta, xr, pr = _indexed(b, np.random.RandomState(seed), xrow, pos_row)
    off = np.full(b.n + 1, -7, dtype=np.int64); status = np.full(b.n, 9, dtype=np.uint8); info = np.full(4, -7, dtype=np.int64)
    cap = b.n * (int(b.meta[:, 1].max()) + 160)
    text = np.zeros(cap, dtype=np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    L.check(lib.cv_vcf_records_host_form(p(b.call), p(b.qual), b.n, p(x), p(xr), p(b.buf), p(meta), p(pr), int(show_ref),
                                         0 if qual is None else 1, 0 if qual is None else qual, p(off), p(status), p(info), p(text), cap))
    return text[:off[b.n]].tobytes(), off, status, info


def dev_records(b, show_ref=True, qual=None, xrow=False, pos_row=False, seed=5, write=True, slack=0, phase=3):
    """cv_vcf_records_dev -> (text bytes, off [n + 1], status [n], info [4], the CANARY bytes behind the text).  The text
    buffer holds exactly off[n] (+ slack) bytes in front of the canary and starts `phase` bytes behind an aligned address."""
    import torch
    L, lib = _lib()
    dev = torch.device("cuda")
    x, meta, xr, pr = _indexed(b, np.random.RandomState(seed), xrow, pos_row)
    up = lambda a: torch.from_numpy(a).to(dev) if a is not None else None
    call_d, qual_d, x_d, buf_d, meta_d, xr_d, pr_d = (up(a) for a in (b.call, b.qual, x, b.buf, meta, xr, pr))
    off = torch.full((b.n + 1,), -7, dtype=torch.int64, device=dev)
    status = torch.full((b.n,), 9, dtype=torch.uint8, device=dev)
    info = torch.full((4,), -7, dtype=torch.int64, device=dev)
    need = ctypes.c_int64(0)
    L.check(lib.cv_vcf_records_workspace(b.n, ctypes.byref(need)))
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(text, cap):
        L.check(lib.cv_vcf_records_dev(ptr(call_d), ptr(qual_d), b.n, ptr(x_d), ptr(xr_d), ptr(buf_d), ptr(meta_d), ptr(pr_d),
                                       int(show_ref), 0 if qual is None else 1, 0 if qual is None else qual, ptr(off), ptr(status),
                                       ptr(info), text, cap, ptr(ws), ws.numel(), stream))
        torch.cuda.synchronize()
    run(None, 0)
    off0, status0, info0 = off.cpu().numpy().copy(), status.cpu().numpy().copy(), info.cpu().numpy().copy()
    if not write:
        return b"", off0, status0, info0, b""
    total = int(off0[b.n]) + slack
    room = torch.full((phase + total + CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    run(ctypes.c_void_p(room.data_ptr() + phase), total)
    assert np.array_equal(off.cpu().numpy(), off0) and np.array_equal(status.cpu().numpy(), status0) and \
        np.array_equal(info.cpu().numpy(), info0), "the length-only call and the writing call disagree"
    got = room.cpu().numpy().tobytes()
    assert got[:phase] == b"\xa5" * phase, "bytes in front of the text were written"
    return got[phase:phase + total], off0, status0, info0, got[phase + total:]


def check_batch(b, **kw):
    """device == host form, every DEVICE record == cv_format_vcf of its candidate alone, and the text of a batch without
    a HOST candidate == cv_format_vcf over the batch in one call; -> (text, status)"""
    want_text, want_off, want_status, want_info = host_form(b, **{k: v for k, v in kw.items() if k != "phase"})
    text, off, status, info, tail = dev_records(b, **kw)
    assert tail == b"\xa5" * CANARY, "the canary behind the text was written"
    assert np.array_equal(status, want_status) and np.array_equal(off, want_off) and np.array_equal(info, want_info)
    assert text == want_text
    assert info.tolist() == [len(text), int((status == DEVICE).sum()), int((status == HOST).sum()), 0] and off[b.n] == len(text)
    for i in range(b.n):
        line = text[off[i]:off[i + 1]]
        if status[i] == HOST:
            assert line == b""
        else:
            assert line == host_one(b, i, kw.get("show_ref", True), kw.get("qual")), i
            assert (status[i] == DEVICE) == bool(line) and (not line or line.endswith(b"\n"))
    if not (status == HOST).any():
        assert (text, int(info[1])) == host_batch(b, kw.get("show_ref", True), kw.get("qual"))
    return text, status


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_batch_sizes(n):
    text, status = check_batch(random_batch(n, 100 + n))
    assert text.count(b"\n") == int((status == DEVICE).sum()) and not (status == HOST).any()
    if n >= 63:
        assert (status == NONE).any() and (status == DEVICE).sum() > n // 2


@pytest.mark.parametrize("xrow,pos_row", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("show_ref,qual", [(False, None), (True, 3), (False, 0)])
def test_options(xrow, pos_row, show_ref, qual):
    b = random_batch(300, 7)
    text, status = check_batch(b, show_ref=show_ref, qual=qual, xrow=xrow, pos_row=pos_row)
    none = (b.qual[:, 2] == 0) | ((b.call[:, 0] == 0) & (not show_ref))
    assert np.array_equal(status == NONE, none) and np.array_equal(status == DEVICE, ~none)
    assert (b"\tPASS\t" in text and b"\tLowQual\t" in text) if qual == 3 else b"LowQual" not in text
    assert text == host_form(b, show_ref=show_ref, qual=qual)[0]             # the index arrays do not change the bytes


@pytest.mark.parametrize("phase", [0, 13])
def test_text_alignments(phase):
    check_batch(random_batch(130, 21), phase=phase)


def test_length_only_call_and_a_cap_too_small():
    b = random_batch(65, 2)
    want, want_off, _s, _i = host_form(b)
    _t, off, status, info, _c = dev_records(b, write=False)
    assert np.array_equal(off, want_off) and info[0] == len(want) and not (status == HOST).any()
    last = int(np.flatnonzero(status == DEVICE)[-1])
    # text_cap one record short: the records that fit are written, the last one is not, nothing behind the cap is
    text, off, status, info, tail = dev_records(b, slack=-(int(off[last + 1]) - int(off[last])))
    assert text == want[:off[last]] and tail == b"\xa5" * CANARY and info[0] == len(want)
    # room to spare: nothing behind off[n] is written
    text, off, status, info, tail = dev_records(b, slack=64)
    assert text == want + b"\xa5" * 64 and tail == b"\xa5" * CANARY


def _edges():
    """(name, planted function, expected status, bytes the record must hold)"""
    def centre_af(v, dp=32.0):
        def f(c, q, x, t):
            c[:5] = (1, 0, 2, 1, 2); q[2] = dp; x[16, 1, 3] = v; t[2] = SEQ.encode()      # (centre A: the allele is C)
        return f

    def lengths(var_type, inferred, seq_len=33, var_len=5):
        def f(c, q, x, t):
            c[:5] = (var_type, 0, var_len, 1, 2); q[2] = 32.0; x[:] = 0; t[2] = SEQ[:seq_len].encode()
            x[17:, :, 0] = 2.0
            x[17:17 + inferred, :, var_type - 1] = 1.0
            x[17:17 + inferred, 2, var_type - 1] = 3.0
        return f

    def tok(k, value, var_type=1):
        def f(c, q, x, t):
            c[:5] = (var_type, 0, 2, 1, 2); q[2] = 32.0; t[k] = value
        return f

    def quals(p1, p2, dp=32.0):
        def f(c, q, x, t):
            c[:5] = (1, 0, 2, 1, 2); q[0] = p1; q[1] = p2; q[2] = dp
        return f

    def decisions(k, v):
        def f(c, q, x, t):
            c[:5] = (1, 0, 2, 1, 2); c[k] = v; q[2] = 32.0
        return f

    def depth(v):
        def f(c, q, x, t):
            c[:5] = (1, 0, 2, 1, 2); q[2] = v; x[16, :, 3] = 1.0
        return f
    nan, inf = float("nan"), float("inf")
    e = [("af 1/32", centre_af(1.0), DEVICE, b":0.0312\n"), ("af 3/32", centre_af(3.0), DEVICE, b":0.0938\n"),
         ("af 5/32", centre_af(5.0), DEVICE, b":0.1562\n"), ("af 7/32", centre_af(7.0), DEVICE, b":0.2188\n"),
         ("af -1/32", centre_af(-1.0), DEVICE, b":-0.0312\n"), ("af 1/20000", centre_af(1.0, 20000.0), DEVICE, b":20000:0.000"),
         ("af 3/20000", centre_af(3.0, 20000.0), DEVICE, b":20000:0.000"), ("af -0", centre_af(-0.0), DEVICE, b":-0.0000\n"),
         ("af tiny negative", centre_af(-1.0, 16777215.0), DEVICE, b":16777215:-0.0000\n"), ("af absurd", centre_af(3e38, 1.0), HOST, b""),
         ("af nan", centre_af(nan), HOST, b""), ("dp 1", depth(1.0), DEVICE, b":1:1.0000\n"), ("dp 2^24", depth(16777216.0), HOST, b""),
         ("dp 2.5", depth(2.5), HOST, b""), ("dp -3", depth(-3.0), HOST, b""), ("dp nan", depth(nan), HOST, b""),
         ("dp inf", depth(inf), HOST, b""), ("dp 0", depth(0.0), NONE, b""),
         ("ins length 0", lengths(2, 0, var_len=0), DEVICE, b"\tA\tAA\t"), ("del length 0", lengths(3, 0, var_len=0), DEVICE, b"\tAC\tA\t"),
         ("ins 4", lengths(2, 4), DEVICE, b"\tAGGGG\t"), ("ins 15", lengths(2, 15), DEVICE, b"LENGUESS=15\t"),
         ("ins 16", lengths(2, 16), DEVICE, b"\t<INS>\t"), ("del 4", lengths(3, 4), DEVICE, b"LENGUESS=4\t"),
         ("del 15", lengths(3, 15), DEVICE, b"\tACGTACGTACGTACGT\tA\t"), ("del 16", lengths(3, 16), DEVICE, b"SVTYPE=DEL\t"),
         ("del 3, seq 17", lengths(3, 0, 17, 3), DEVICE, b"\t.\tA\tA\t"), ("del 15, seq 21", lengths(3, 15, 21), DEVICE, b"\t.\tACGTA\tA\t"),
         ("lower case", tok(2, SEQ.lower().encode(), 3), DEVICE, b"\t.\tACG\tA\t"), ("seq 16", tok(2, SEQ[:16].encode()), HOST, b""),
         ("centre N ref", tok(2, (SEQ[:16] + "N" + SEQ[17:]).encode(), 0), HOST, b""),
         ("centre N ins", tok(2, (SEQ[:16] + "N" + SEQ[17:]).encode(), 2), DEVICE, b"\tN\tN"),
         ("contig 1", tok(0, b"7"), DEVICE, b"7\t"), ("contig 255", tok(0, b"q" * 255), DEVICE, b"q" * 255 + b"\t"),
         ("contig 256", tok(0, b"q" * 256), HOST, b""), ("leading zeros", tok(1, b"007"), DEVICE, b"\t7\t.\t"),
         ("18 digits", tok(1, b"9" * 18), DEVICE, b"\t" + b"9" * 18 + b"\t"), ("19 digits", tok(1, b"1234567890123456789"), HOST, b""),
         ("plus", tok(1, b"+5"), HOST, b""), ("minus", tok(1, b"-5"), HOST, b""), ("blank", tok(1, b" 5"), HOST, b""),
         ("carriage return", tok(1, b"5\r"), HOST, b""), ("empty position", tok(1, b""), HOST, b""),
         ("p2 == p1", quals(0.75, 0.75), DEVICE, b"\t0\t"), ("p2 == 0", quals(0.75, 0.0), DEVICE, b"\t2998\t"),
         ("negative quality", quals(0.001, 0.75), DEVICE, b"\t-28\t")]
    for dp in (32.0, 0.0):
        e += [("p1 nan, dp %g" % dp, quals(nan, 0.5, dp), HOST, b""), ("p2 nan, dp %g" % dp, quals(0.5, nan, dp), HOST, b""),
              ("p2 inf, dp %g" % dp, quals(0.5, inf, dp), HOST, b""), ("p1 inf, dp %g" % dp, quals(inf, 0.5, dp), HOST, b""),
              ("p1 negative, dp %g" % dp, quals(-0.5, 0.5, dp), HOST, b"")]
    e += [("varType 4", decisions(0, 4), HOST, b""), ("varType -1", decisions(0, -1), HOST, b""), ("zygosity 2", decisions(1, 2), HOST, b""),
          ("length 6", decisions(2, 6), HOST, b""), ("1/1", decisions(1, 1), DEVICE, b"\t1/1:")]
    return e


def test_the_edges_in_one_batch():
    edges = _edges()
    b = random_batch(3 * len(edges), 9, [(3 * k + 1, f) for k, (_name, f, _st, _hold) in enumerate(edges)])
    text, off, status, info, tail = dev_records(b)
    want = host_form(b)
    assert tail == b"\xa5" * CANARY and text == want[0] and np.array_equal(off, want[1]) and np.array_equal(status, want[2])
    assert np.array_equal(info, want[3])
    L, _lib_ = _lib()
    for k, (name, _f, st, hold) in enumerate(edges):
        i = 3 * k + 1
        line = text[off[i]:off[i + 1]]
        assert status[i] == st, name
        if st == HOST:                       # the host prints it, or refuses it with its own message
            assert line == b""
            try:
                host_one(b, i, True, None)
            except L.CvError as err:
                assert "cv_format_vcf: record 0" in str(err), name
        else:
            assert line == host_one(b, i, True, None) and hold in line, (name, line)
    for i in range(0, b.n, 3):               # the neighbours of a HOST candidate are written
        if status[i] == DEVICE:
            assert text[off[i]:off[i + 1]] == host_one(b, i, True, None)


def test_argument_checks():
    import torch
    L, lib = _lib()
    need = ctypes.c_int64(-1)
    assert lib.cv_vcf_records_workspace(0, ctypes.byref(need)) == 0 and need.value >= 0
    assert lib.cv_vcf_records_workspace(-1, ctypes.byref(need)) == 1 and lib.cv_vcf_records_workspace(5, None) == 1
    assert lib.cv_vcf_records_dev(None, None, 0, None, None, None, None, None, 0, 0, 0, None, None, None, None, 0, None, 0, None) == 0
    assert lib.cv_vcf_records_host_form(None, None, 0, None, None, None, None, None, 0, 0, 0, None, None, None, None, 0) == 0
    b = random_batch(4, 1)
    t = {k: torch.from_numpy(v).cuda() for k, v in (("call", b.call), ("qual", b.qual), ("x", b.x), ("buf", b.buf), ("meta", b.meta))}
    small = torch.zeros(64, dtype=torch.int64, device="cuda")
    status = torch.zeros(8, dtype=torch.uint8, device="cuda")
    L.check(lib.cv_vcf_records_workspace(4, ctypes.byref(need)))
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
    good = dict(call=t["call"].data_ptr(), qual=t["qual"].data_ptr(), n=4, x=t["x"].data_ptr(), xrow=None, buf=t["buf"].data_ptr(),
                meta=t["meta"].data_ptr(), pos_row=None, off=small.data_ptr() + 32, status=status.data_ptr(), info=small.data_ptr(),
                ws=ws.data_ptr(), ws_bytes=need.value)

    def rc(**over):
        a = dict(good, **over)
        r = lib.cv_vcf_records_dev(a["call"], a["qual"], a["n"], a["x"], a["xrow"], a["buf"], a["meta"], a["pos_row"], 1, 0, 0, a["off"],
                                   a["status"], a["info"], None, 0, a["ws"], a["ws_bytes"], None)
        torch.cuda.synchronize()
        return r
    assert rc() == 0
    for over in (dict(n=-1), dict(call=None), dict(qual=None), dict(x=None), dict(buf=None), dict(meta=None), dict(off=None),
                 dict(status=None), dict(info=None), dict(ws=None), dict(ws_bytes=need.value - 1), dict(call=good["call"] + 2),
                 dict(qual=good["qual"] + 1), dict(x=good["x"] + 2), dict(meta=good["meta"] + 4), dict(off=good["off"] + 4),
                 dict(info=good["info"] + 4), dict(xrow=good["info"] + 4), dict(pos_row=good["info"] + 4), dict(ws=good["ws"] + 8)):
        assert rc(**over) == 1, over
        assert lib.cv_last_error()


# ---- through the drivers ----------------------------------------------------------------------------------------------------
ROWS = 3000


@pytest.fixture(scope="module")
def tensors(tmp_path_factory):
    """a text tensor file of ROWS rows (some with N at the centre), the same as BGZF"""
    from clairvoyante_amd import utils_v2
    d = tmp_path_factory.mktemp("vcf_format")
    raw = common.inputs(ROWS, seed=23).copy()
    for i in range(1, 4):
        raw[:, :, :, i] += raw[:, :, :, 0]
    rng = np.random.RandomState(4)
    lines = []
    for j in range(ROWS):
        seq = "".join(rng.choice(list("ACGTacgt"), 33))
        if j % 97 == 5:
            seq = seq[:16] + "N" + seq[17:]
        lines.append("%s %d %s %s" % ("chr%d" % (1 + j % 4), 10000 + 7 * j, seq, " ".join("%0.1f" % v for v in raw[j].reshape(-1))))
    text = ("\n".join(lines) + "\n").encode()
    out = {"plain": str(d / "t.txt"), "bgzf": str(d / "t.bgzf.gz"), "dir": str(d)}
    open(out["plain"], "wb").write(text)
    with utils_v2.BgzfWriter(out["bgzf"]) as w:
        w.write(text)
    return out


@pytest.fixture(scope="module")
def model(oracle, tmp_path_factory):
    from clairvoyante_amd import clairvoyante_v3
    m = clairvoyante_v3.Clairvoyante()
    m.init()
    m.setParameters(common.bench_params(oracle, "full", seed=11))
    chk = str(tmp_path_factory.mktemp("vcf_format_ckpt") / "model-000001")
    m.saveParameters(chk)
    yield m, chk
    m.close()


def call_file(model, monkeypatch, fn, out, route, parse, show_ref, qual):
    """callVar.Test over fn under CV_VCF_FORMAT=route, CV_TEXT_PARSE=parse -> (the VCF's bytes, what vcf_format_counts grew by)"""
    from clairvoyante_amd import callVar, utils_v2
    monkeypatch.setenv("CV_VCF_FORMAT", route)
    monkeypatch.setenv("CV_TEXT_PARSE", parse)
    a = types.SimpleNamespace(tensor_fn=fn, chkpnt_fn=model[1], call_fn=out, qual=qual, sampleName="S", ref_fn=None, threads=None,
                              showRef=show_ref, v3=True, v2=False, slim=False, batch_size=1024)
    before = callVar.vcf_format_counts()
    callVar.Test(a, model[0], utils_v2)
    after = callVar.vcf_format_counts()
    return open(out, "rb").read(), {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("show_ref", [False, True])
@pytest.mark.parametrize("qual", [None, 30])
def test_callvar_writes_the_same_vcf_on_either_route(tensors, model, monkeypatch, show_ref, qual):
    vcf = {}
    for route in ("host", "device"):
        for parse in ("host", "device"):
            out = os.path.join(tensors["dir"], "%s_%s_%d_%s.vcf" % (route, parse, show_ref, qual))
            vcf[route, parse], grew = call_file(model, monkeypatch, tensors["plain"], out, route, parse, show_ref, qual)
            other = "device" if route == "host" else "host"
            assert grew[route] >= 2 and grew[other] == 0 and grew["handed_over"] == 0, (route, parse, grew)
    records = [l for l in vcf["host", "host"].splitlines() if not l.startswith(b"#")]
    assert len(records) >= (ROWS - 100 if show_ref else 100)
    for key, text in vcf.items():
        assert text == vcf["host", "host"], key


def test_callvar_over_a_bgzf_file(tensors, model, monkeypatch):
    """the text exists on the device only: the records read the tokens where the parser left them (through Run)"""
    from clairvoyante_amd import callVar
    vcf = {}
    for route in ("host", "device"):
        out = os.path.join(tensors["dir"], "bgzf_%s.vcf" % route)
        vcf[route], grew = call_file(model, monkeypatch, tensors["bgzf"], out, route, "device", True, 20)
        assert grew[route] >= 1 and grew["handed_over"] == 0 and grew["host" if route == "device" else "device"] == 0
    assert vcf["device"] == vcf["host"] and vcf["host"].count(b"\n") > ROWS - 100
    a = types.SimpleNamespace(tensor_fn=tensors["bgzf"], chkpnt_fn=model[1], call_fn=os.path.join(tensors["dir"], "run.vcf"), qual=20,
                              sampleName="S", ref_fn=None, threads=None, showRef=True, v3=True, v2=False, slim=False)
    monkeypatch.setenv("CV_VCF_FORMAT", "device")
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    before = callVar.vcf_format_counts()
    callVar.Run(a)
    assert callVar.vcf_format_counts()["device"] > before["device"]
    assert open(a.call_fn, "rb").read() == vcf["host"]


def test_callvarbam_with_the_native_reader(model, tmp_path, monkeypatch):
    from bam_writer import write_bam
    from clairvoyante_amd import callVar, callVarBam
    base = os.path.join(G, "noisy")
    recs = [l.rstrip("\n") for l in open(base + ".sam") if not l.startswith("@")]
    bam = str(tmp_path / "noisy.bam")
    write_bam(bam, recs, [("ctgA", 2600), ("other", 10)], block_payload=9001)
    fa = str(tmp_path / "ref.fa")
    shutil.copy(base + ".fa", fa)
    with open(fa + ".fai", "w") as fh:       # the 70-column FASTA of the generator: ">ctgA synthetic\n" is 16 bytes
        fh.write("ctgA\t2600\t16\t70\t71\n")
    vcf = {}
    for route in ("host", "device"):
        monkeypatch.setenv("CV_VCF_FORMAT", route)
        a = callVarBam.build_parser().parse_args(["--chkpnt_fn", model[1], "--ref_fn", fa, "--ctgName", "ctgA", "--threshold", "0.125",
                                                  "--minCoverage", "2", "--bam_fn", bam, "--samtools", "native", "--qual", "10",
                                                  "--call_fn", str(tmp_path / (route + ".vcf"))])
        before = callVar.vcf_format_counts()
        callVarBam.Run(a)
        after = callVar.vcf_format_counts()
        grew = {k: after[k] - before[k] for k in after}
        assert grew[route] >= 1 and grew["handed_over"] == 0 and grew["host" if route == "device" else "device"] == 0, grew
        vcf[route] = open(a.call_fn, "rb").read()
    assert vcf["device"] == vcf["host"] and sum(1 for l in vcf["host"].splitlines() if not l.startswith(b"#")) > 10


def _from_device(model, monkeypatch, route, pos, batch, plant=None):
    """callVar.CallFromDevice over 700 rows in HBM -> (text, what vcf_format_counts grew by)"""
    import io
    import torch
    from clairvoyante_amd import callVar
    monkeypatch.setenv("CV_VCF_FORMAT", route)
    x = torch.from_numpy(common.inputs(700, seed=31)).cuda()
    if plant is not None:
        keep = callVar.predict_and_reduce

        def planted(m, xd):
            call, qual = keep(m, xd)
            plant(call, qual)
            return call, qual
        monkeypatch.setattr(callVar, "predict_and_reduce", planted)
    a = types.SimpleNamespace(showRef=True, qual=15)
    fh = io.StringIO()
    before = callVar.vcf_format_counts()
    callVar.CallFromDevice(a, model[0], fh, x, pos, batch=batch)
    after = callVar.vcf_format_counts()
    return fh.getvalue(), {k: after[k] - before[k] for k in after}


def test_a_batch_with_a_position_the_device_does_not_take(model, monkeypatch):
    """"+4321" is an integer to the host (it prints 4321); the device leaves it, and its batch goes back whole"""
    from clairvoyante_amd.utils_v2 import PosBatch
    strings = ["ctg%d:%d:%s" % (i % 3, 500 + i, SEQ) for i in range(700)]
    strings[333] = "ctg0:+4321:" + SEQ
    clean = list(strings); clean[333] = "ctg0:4321:" + SEQ
    host, grew = _from_device(model, monkeypatch, "host", PosBatch.from_strings(strings), 256)
    assert grew == {"host": 3, "device": 0, "handed_over": 0}
    dev, grew = _from_device(model, monkeypatch, "device", PosBatch.from_strings(strings), 256)
    assert grew == {"host": 1, "device": 2, "handed_over": 1}
    assert dev == host and "ctg0\t4321\t" in host
    text, grew = _from_device(model, monkeypatch, "device", PosBatch.from_strings(clean), 256)
    assert grew == {"host": 0, "device": 3, "handed_over": 0} and text == host
    # a function for the positions, as callVarBam's callers may give one
    text, grew = _from_device(model, monkeypatch, "device", lambda i: clean[i], 700)
    assert grew == {"host": 0, "device": 1, "handed_over": 0} and text == host


def test_a_nan_product_raises_the_hosts_message_on_both_routes(model, monkeypatch):
    from clairvoyante_amd import _lib as L
    from clairvoyante_amd.utils_v2 import PosBatch
    pos = PosBatch.from_strings(["ctg1:%d:%s" % (500 + i, SEQ) for i in range(700)])

    def plant(call, qual):
        qual[5, 0] = float("nan")
    for route in ("host", "device"):
        with pytest.raises(L.CvError, match="record 5: quality is not a finite number"):
            _from_device(model, monkeypatch, route, pos, 700, plant)
        monkeypatch.undo()


def test_an_unknown_route_raises(model, monkeypatch):
    from clairvoyante_amd import callVar
    monkeypatch.setenv("CV_VCF_FORMAT", "gpu")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        callVar.vcf_format_route()
    with pytest.raises(ValueError, match="'host' or 'device'"):
        list(callVar.called_batches(types.SimpleNamespace(showRef=False, qual=None), model[0], (b for b in ())))
