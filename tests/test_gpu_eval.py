"""The evaluation report on the device: cv_eval_counts against train.evaluation_counts_host, Clairvoyante.evaluateCounts
against the host report over m.predict, and the drivers (evaluate, evaluateListOfModels, calTrainDevDiff) with the set
resident in HBM and streamed."""
import contextlib
import ctypes
import io
import logging
import pickle
import sys
import types

import numpy as np
import pytest

import common
import eval_cases

pytestmark = pytest.mark.gpu

SENTINEL = 7777
LAUNCH_CAP = 256                # workgroups of 256 candidates (csrc/cv_eval.hip, EV_GRID): 70 001 candidates exceed it


def _split(out16):
    return out16[:, 0:4], out16[:, 4:6], out16[:, 6:10], out16[:, 10:16]


def _host_counts(out16, Y):
    from clairvoyante_amd import train
    return train.evaluation_counts_host(*_split(out16), Y)


def _fresh_counts():
    import torch
    c = torch.zeros(64, dtype=torch.int64, device="cuda")
    c[3] = SENTINEL; c[60:] = SENTINEL
    return c


def _call(out_d, y_d, n, counts):
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    rc = lib.cv_eval_counts(ctypes.c_void_p(out_d.data_ptr()), ctypes.c_void_p(y_d.data_ptr()),
                            int(y_d.dtype == torch.float64), n, ctypes.c_void_p(counts.data_ptr()), None)
    torch.cuda.synchronize()
    return rc


def _with_sentinels(c):
    c = np.array(c, dtype=np.int64); c[3] = SENTINEL; c[60:] = SENTINEL
    return c


@pytest.mark.parametrize("ydtype", [np.float32, np.float64], ids=["y32", "y64"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 70001])
def test_kernel_counts_match_the_host_report(n, ydtype):
    """arbitrary outputs and labels, no model: a lane mask (1, 63, 65), a wave tail, the workgroup flush (255 .. 257),
    several workgroups (1 000) and the grid stride (70 001 > 256 workgroups); the crafted rows -- ties, -0.0, NaN in
    outputs and labels -- on row 0, the last row and both sides of the 64-lane and 256-thread boundaries"""
    import torch
    assert n < 70001 or n > LAUNCH_CAP * 256
    out16, Y = eval_cases.planted(n, seed=n % 97, ydtype=ydtype)
    want = _host_counts(out16, Y)
    if n >= 1000:                                   # precondition on the reference alone: no cell is trivially right
        assert (want[eval_cases.CELLS] > 0).all()
    assert want[0] == n
    out_d, y_d = torch.from_numpy(out16).cuda(), torch.from_numpy(Y).cuda()
    counts = _fresh_counts()
    assert _call(out_d, y_d, n, counts) == 0
    got = counts.cpu().numpy()
    print("n=%d %s: device %s" % (n, np.dtype(ydtype).name, got[:3].tolist()))
    assert np.array_equal(got, _with_sentinels(want))
    # the call ADDS: a second one into the same tensor gives twice the counts, the unused entries keep their value
    assert _call(out_d, y_d, n, counts) == 0
    assert np.array_equal(counts.cpu().numpy(), _with_sentinels(2 * want))


def test_kernel_on_the_crafted_rows_alone():
    """every row is one where a tie rule decides; also against the per-candidate loop of the reference's report"""
    import torch
    for ydtype in (np.float32, np.float64):
        out16, Y = eval_cases.adversarial_rows(ydtype)
        want = _host_counts(out16, Y)
        assert np.array_equal(want, eval_cases.counts_per_row(out16, Y))
        counts = torch.zeros(64, dtype=torch.int64, device="cuda")
        assert _call(torch.from_numpy(out16).cuda(), torch.from_numpy(Y).cuda(), len(out16), counts) == 0
        assert np.array_equal(counts.cpu().numpy(), want)


def test_kernel_on_the_table_rows():
    """order 3,1,0,2 / 2,0,1,3 / 3,2,1,0 / 1,0,3,2 and argmax 0 / 0 / 0 / 1, for every truth index, as literals"""
    import torch
    for row, order, am in eval_cases.TABLE:
        for truth in range(4):
            out16 = np.zeros((1, 16), dtype=np.float32); out16[0, 0:4] = row; out16[0, 6:10] = row
            Y = np.zeros((1, 16), dtype=np.float32); Y[0, truth] = 1; Y[0, 6 + truth] = 1
            counts = torch.zeros(64, dtype=torch.int64, device="cuda")
            assert _call(torch.from_numpy(out16).cuda(), torch.from_numpy(Y).cuda(), 1, counts) == 0
            c = counts.cpu().numpy()
            assert (c[0], c[1], c[2]) == (1, int(truth == order[0]), int(truth in order[:2])), (row, truth)
            assert c[8 + truth * 4 + am] == 1 and c[8:24].sum() == 1 and c[4] == 1 and c[24] == 1


def test_float64_labels_are_compared_as_float64():
    """[1, 1 + 2^-40, 0, 0] has its maximum at index 1; rounded to fp32 the two would tie and index 0 would win"""
    import torch
    out16 = np.zeros((1, 16), dtype=np.float32); out16[0, 1] = 1; out16[0, 5] = 1
    Y = np.zeros((1, 16)); Y[0, 0:4] = [1, 1 + 2.0 ** -40, 0, 0]; Y[0, 4:6] = [1, 1 + 2.0 ** -40]
    for y, top1, cell in ((Y, 1, 4 + 1 * 2 + 1), (Y.astype(np.float32), 0, 4 + 0 * 2 + 1)):
        counts = torch.zeros(64, dtype=torch.int64, device="cuda")
        assert _call(torch.from_numpy(out16).cuda(), torch.from_numpy(y).cuda(), 1, counts) == 0
        c = counts.cpu().numpy()
        assert c[1] == top1 and c[cell] == 1 and c[4:8].sum() == 1
        assert np.array_equal(c, _host_counts(out16, y))


def test_argument_checks():
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    out16, Y = eval_cases.random_rows(8, seed=1, ydtype=np.float32)
    out_d, y_d = torch.from_numpy(out16).cuda(), torch.from_numpy(Y).cuda()
    counts = _fresh_counts()
    before = counts.cpu().numpy()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    # n == 0: nothing is touched, whatever the pointers are
    assert lib.cv_eval_counts(p(out_d), p(y_d), 0, 0, p(counts), None) == 0
    assert lib.cv_eval_counts(None, None, 0, 0, None, None) == 0
    for args, word in (((None, p(y_d), 0, 8, p(counts)), b"null"), ((p(out_d), None, 0, 8, p(counts)), b"null"),
                       ((p(out_d), p(y_d), 0, 8, None), b"null"), ((p(out_d), p(y_d), 0, -1, p(counts)), b"negative"),
                       ((p(out_d, 4), p(y_d), 0, 1, p(counts)), b"aligned"), ((p(out_d), p(y_d, 8), 0, 1, p(counts)), b"aligned"),
                       ((p(out_d), p(y_d), 0, 8, p(counts, 4)), b"aligned")):
        assert lib.cv_eval_counts(*args, None) == 1
        msg = lib.cv_last_error()
        assert b"cv_eval_counts" in msg and word in msg, msg
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), before)


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_evaluate_counts_equals_the_host_report_over_predict(oracle, arch):
    import torch
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    x = common.inputs(1500, stress=8)
    n = x.shape[0]
    _, Y = eval_cases.planted(n, seed=4, ydtype=np.float64)
    m = (clairvoyante_v3 if arch == "full" else clairvoyante_v3_slim).Clairvoyante()
    try:
        m.setParameters(common.bench_params(oracle, arch))
        out16 = np.concatenate(m.predict(x), axis=1)
        for y in (Y, Y.astype(np.float32)):
            want = _host_counts(out16, y)
            got = m.evaluateCounts(x, y)
            assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (64,)
            assert np.array_equal(got.cpu().numpy(), want)
            # device tensors, in two parts into one tensor
            xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
            acc = m.evaluateCounts(xd[:700], yd[:700])
            assert m.evaluateCounts(xd[700:], yd[700:], acc) is acc
            assert np.array_equal(acc.cpu().numpy(), want)
        with pytest.raises(ValueError):
            m.evaluateCounts(x, Y[:-1])
    finally:
        m.close()


# ---- the drivers ---------------------------------------------------------------------------------------------------

N_BIN = 1700


@pytest.fixture(scope="module")
def small_bin(tmp_path_factory):
    """a 1 700-candidate .bin (three whole blocks and a ragged one) and two slim checkpoints"""
    from clairvoyante_amd import clairvoyante_v3_slim, synth, utils_v2
    d = tmp_path_factory.mktemp("evalbin")
    xt, cls, rf, alt, il = synth.make_candidates(N_BIN, seed=31, return_class=True)
    y = synth.make_labels(cls, rf, alt, il).numpy().astype(np.float64); x = xt.numpy()
    XC = [utils_v2.pack_array(x[s:s + 500]) for s in range(0, N_BIN + 1, 500)]
    YC = [utils_v2.pack_array(y[s:s + 500]) for s in range(0, N_BIN + 1, 500)]
    binfn = str(d / "e.bin")
    with open(binfn, "wb") as fh:
        pickle.dump(N_BIN, fh); pickle.dump(XC, fh); pickle.dump(YC, fh); pickle.dump([], fh)
    prefixes = []
    m = clairvoyante_v3_slim.Clairvoyante()
    for seed in (1, 2):
        m.setParameters(common.bench_params(None, "slim", seed=seed))
        prefixes.append(str(d / ("model-%06d" % seed))); m.saveParameters(prefixes[-1])
    m.close()
    return types.SimpleNamespace(bin_fn=binfn, prefixes=prefixes, dir=d, x=x, y=y)


def _args(sb, **kw):
    return types.SimpleNamespace(bin_fn=sb.bin_fn, tensor_fn=None, var_fn=None, bed_fn=None, v2=False, v3=True, slim=True, **kw)


@contextlib.contextmanager
def _captured():
    logs = []

    class H(logging.Handler):
        def emit(self, rec):
            msg = rec.getMessage()
            if "time elapsed" not in msg:
                logs.append(msg)
    h = H(); root = logging.getLogger(); level = root.level
    root.addHandler(h); root.setLevel(logging.INFO)
    err = io.StringIO(); old = sys.stderr; sys.stderr = err
    try:
        yield logs, err
    finally:
        sys.stderr = old
        root.removeHandler(h); root.setLevel(level)


class _Spy(object):
    """counts the calls of the block decoder (utils_v2._unpack_into_one / unpack_arrays), of evaluateCounts and predict"""

    def __init__(self, monkeypatch):
        from clairvoyante_amd import model, utils_v2
        self.decodes, self.counted, self.predicted, self.resident = 0, [], 0, []
        one, many, ec, pr = utils_v2._unpack_into_one, utils_v2.unpack_arrays, model.Clairvoyante.evaluateCounts, \
            model.Clairvoyante.predict
        rfb = utils_v2.resident_from_blocks

        def spy_rfb(*a, **k):
            out = rfb(*a, **k)
            self.resident.append(isinstance(out[0], utils_v2.ResidentBlocks))
            return out
        monkeypatch.setattr(utils_v2, "resident_from_blocks", spy_rfb)

        def spy_one(*a, **k):
            self.decodes += 1
            return one(*a, **k)

        def spy_many(*a, **k):
            self.decodes += 1
            return many(*a, **k)

        def spy_ec(m, X, Y, counts=None):
            self.counted.append(int(X.shape[0]))
            return ec(m, X, Y, counts)

        def spy_pr(m, X):
            self.predicted += 1
            return pr(m, X)
        monkeypatch.setattr(utils_v2, "_unpack_into_one", spy_one)
        monkeypatch.setattr(utils_v2, "unpack_arrays", spy_many)
        monkeypatch.setattr(model.Clairvoyante, "evaluateCounts", spy_ec)
        monkeypatch.setattr(model.Clairvoyante, "predict", spy_pr)


@pytest.fixture(scope="module")
def host_lines(small_bin):
    """the report of both checkpoints through the host route: computed once, shared"""
    import os
    from clairvoyante_amd import evaluate
    old = os.environ.get("CV_EVAL")
    os.environ["CV_EVAL"] = "host"
    try:
        out = []
        for prefix in small_bin.prefixes:
            with _captured() as (logs, _):
                evaluate.Run(_args(small_bin, chkpnt_fn=prefix))
            out.append(logs)
    finally:
        if old is None:
            del os.environ["CV_EVAL"]
        else:
            os.environ["CV_EVAL"] = old
    # the host route's own lines are the report of the predictions (not a copy of what the device route printed)
    assert out[0][:4] == ["Loading model ...", "Loading the dataset ...", "Dataset size: %d" % N_BIN, "Testing on the dataset ..."]
    assert out[0][5].startswith("all/top1/top2/top1p/top2p: %d/" % N_BIN) and len(out[0]) == 4 + 17 and out[0] != out[1]
    return out


@pytest.mark.parametrize("mode", ["resident", "streamed", "default", "several_passes", "one_pass_exactly"])
def test_evaluate_run_device_lines_equal_the_host_lines(small_bin, host_lines, monkeypatch, mode):
    """the set resident (it is one pass: decoded ahead), streamed because it does not fit, and streamed because a
    caller that walks it once only decodes a set of ONE pass ahead -- on both sides of that threshold"""
    from clairvoyante_amd import evaluate, train, utils_v2
    if mode == "default":
        monkeypatch.delenv("CV_EVAL", raising=False)                    # a real model: the device route, unasked
    else:
        monkeypatch.setenv("CV_EVAL", "device")
    if mode == "streamed":
        monkeypatch.setattr(utils_v2, "TRAINSET_FREE_BYTES", 1 << 20)   # the set does not "fit": it stays in its blocks
    if mode in ("streamed", "several_passes"):
        monkeypatch.setattr(train, "EVAL_PASS", 512)                    # three passes and a ragged last one
    if mode == "one_pass_exactly":
        monkeypatch.setattr(train, "EVAL_PASS", N_BIN)
    spy = _Spy(monkeypatch)
    with _captured() as (logs, _):
        evaluate.Run(_args(small_bin, chkpnt_fn=small_bin.prefixes[0]))
    assert logs == host_lines[0]
    assert spy.predicted == 0                                           # no host predictions on this route
    many = mode in ("streamed", "several_passes")
    assert spy.counted == ([512, 512, 512, 164] if many else [N_BIN])
    assert spy.resident == ([] if many else [True])                     # (not even asked for when there are several passes)


def test_host_route_keeps_predicting_on_the_host(small_bin, host_lines, monkeypatch):
    from clairvoyante_amd import evaluate
    monkeypatch.setenv("CV_EVAL", "host")
    spy = _Spy(monkeypatch)
    with _captured() as (logs, _):
        evaluate.Run(_args(small_bin, chkpnt_fn=small_bin.prefixes[0]))
    assert logs == host_lines[0] and spy.counted == [] and spy.predicted >= 1


def test_evaluate_list_of_models_decodes_the_set_once(small_bin, host_lines, monkeypatch):
    from clairvoyante_amd import evaluateListOfModels
    monkeypatch.setenv("CV_EVAL", "device")
    lst = small_bin.dir / "models.txt"
    lst.write_text("".join(p + "\n" for p in small_bin.prefixes))
    spy = _Spy(monkeypatch)
    marks = []
    test = evaluateListOfModels.Test

    def marked(*a, **k):
        marks.append(spy.decodes)
        test(*a, **k)
        marks.append(spy.decodes)
    monkeypatch.setattr(evaluateListOfModels, "Test", marked)
    with _captured() as (logs, _):
        evaluateListOfModels.Run(_args(small_bin, chkpnt_list=str(lst)))
    # X and Y each in one decode step, before the first checkpoint; neither checkpoint adds one
    assert marks == [2, 2, 2, 2] and spy.predicted == 0 and spy.counted == [N_BIN, N_BIN] and spy.resident == [True]
    want = []
    for prefix, lines in zip(small_bin.prefixes, host_lines):
        want += ["Working on model: %s" % prefix] + lines[4:]
    assert logs == want


def test_caltraindevdiff_line_with_the_resident_set_equals_the_streamed_one(small_bin, monkeypatch):
    from clairvoyante_amd import calTrainDevDiff, clairvoyante_v3_slim, utils_v2
    lines, decodes = [], []
    for free in (None, 1 << 20):                                        # resident, then not
        with monkeypatch.context() as mp:
            mp.setattr(utils_v2, "TRAINSET_FREE_BYTES", free)
            spy = _Spy(mp)
            m = clairvoyante_v3_slim.Clairvoyante(); m.init()
            with _captured() as (_, err):
                calTrainDevDiff.CalcAll(_args(small_bin, chkpnt_fn=small_bin.prefixes), m, utils_v2)
            m.close()
            lines.append(err.getvalue()); decodes.append(spy.decodes)
    assert lines[0] == lines[1] and lines[0].count("\n") == 2 and lines[0].startswith(small_bin.prefixes[0] + "\t")
    assert decodes[0] == 2 and decodes[1] > 4                            # once for the whole list / per batch per checkpoint


def test_resident_from_blocks_holds_the_set_as_the_blocks_do(small_bin):
    import torch
    from clairvoyante_amd import utils_v2
    total, XC, YC, _ = utils_v2.LoadBin(small_bin.bin_fn, lazy=True)
    XR, YR = utils_v2.resident_from_blocks(total, XC, YC, torch.device("cuda", 0))
    assert isinstance(XR, utils_v2.ResidentBlocks) and isinstance(YR, utils_v2.ResidentBlocks)
    assert XR.t.dtype == torch.float32 and YR.t.dtype == torch.float64 and XR.t.is_cuda
    assert np.array_equal(XR.t.cpu().numpy(), small_bin.x) and np.array_equal(YR.t.cpu().numpy(), small_bin.y)
    xb, n, end = utils_v2.DecompressArray(XR, 1500, 512, total)
    assert n == 200 and end == 1 and np.array_equal(xb.cpu().numpy(), small_bin.x[1500:])
    assert utils_v2.resident_from_blocks(total, XR, YR)[0] is XR         # already there: handed back
