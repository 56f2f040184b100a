"""The evaluation report split into numbers and log lines (train.evaluation_counts_host / train.log_evaluation): the host
definition the device route is held to, and the pieces of that route that need no GPU."""
import logging

import numpy as np
import pytest

import eval_cases


def _split(out16):
    return out16[:, 0:4], out16[:, 4:6], out16[:, 6:10], out16[:, 10:16]


@pytest.mark.parametrize("ydtype", [np.float64, np.float32])
def test_counts_match_the_per_row_loop(ydtype):
    """4 000 random rows plus the crafted ones (the table rows, ties, all-equal rows, -0.0, all-zero and NaN labels)
    against the per-candidate loop"""
    from clairvoyante_amd import train
    ro, ry = eval_cases.random_rows(4000, seed=9, ydtype=ydtype)
    ao, ay = eval_cases.adversarial_rows(ydtype)
    out16, Y = np.concatenate([ro, ao]), np.concatenate([ry, ay])
    got = train.evaluation_counts_host(*_split(out16), Y)
    assert got.dtype == np.int64 and got.shape == (64,)
    assert np.array_equal(got, eval_cases.counts_per_row(out16, Y))
    assert got[0] == len(out16) and got[3] == 0 and not got[60:].any()
    # ... and over the crafted rows alone, where every rule decides
    assert np.array_equal(train.evaluation_counts_host(*_split(ao), ay), eval_cases.counts_per_row(ao, ay))


def test_table_rows_count_as_numpy_orders_them():
    """the four rows of the table: order of the base head and np.argmax, for every truth index"""
    from clairvoyante_amd import train
    for row, order, am in eval_cases.TABLE:
        r = np.array(row, dtype=np.float32)
        assert list(r.argsort()[::-1]) == order and list(np.argsort(r, kind="stable")[::-1]) == order
        assert int(np.argmax(r)) == am
        for truth in range(4):
            out16 = np.zeros((1, 16), dtype=np.float32); out16[0, 0:4] = r; out16[0, 6:10] = r
            Y = np.zeros((1, 16)); Y[0, truth] = 1; Y[0, 6 + truth] = 1
            c = train.evaluation_counts_host(*_split(out16), Y)
            assert (c[1], c[2]) == (int(truth == order[0]), int(truth in order[:2]))
            assert c[8 + truth * 4 + am] == 1 and c[8:24].sum() == 1


def test_float64_labels_are_not_rounded_to_a_tie():
    from clairvoyante_amd import train
    out16 = np.zeros((1, 16), dtype=np.float32); out16[0, 1] = 1
    Y = np.zeros((1, 16)); Y[0, 0:4] = [1, 1 + 2.0 ** -40, 0, 0]
    assert train.evaluation_counts_host(*_split(out16), Y)[1] == 1
    assert train.evaluation_counts_host(*_split(out16), Y.astype(np.float32))[1] == 0


# what EvaluateReport logged for the rows of _report_rows() before it was split
_LINES = ['Version 2 model, evaluation on base change:', 'all/top1/top2/top1p/top2p: 700/191/354/27.29/50.57',
          'Version 2 model, evaluation on Zygosity:', '162\t170', '183\t185',
          'Version 2 model, evaluation on variant type:', '42\t40\t46\t54', '47\t34\t57\t42', '52\t42\t38\t40', '51\t40\t39\t36',
          'Version 2 model, evaluation on indel length:', '19\t22\t18\t24\t15\t25', '27\t19\t10\t26\t14\t23',
          '14\t22\t19\t17\t23\t17', '18\t21\t21\t19\t20\t17', '17\t20\t15\t14\t22\t21', '14\t21\t27\t20\t21\t18']
_COUNTS = [700, 191, 354, 0, 162, 170, 183, 185, 42, 40, 46, 54, 47, 34, 57, 42, 52, 42, 38, 40, 51, 40, 39, 36,
           19, 22, 18, 24, 15, 25, 27, 19, 10, 26, 14, 23, 14, 22, 19, 17, 23, 17, 18, 21, 21, 19, 20, 17,
           17, 20, 15, 14, 22, 21, 14, 21, 27, 20, 21, 18, 0, 0, 0, 0]


def _report_rows():
    rng = np.random.RandomState(20)
    n = 700
    out = rng.rand(n, 16).astype(np.float32)
    Y = np.zeros((n, 16)); idx = np.arange(n)
    for lo, hi in eval_cases.HEADS:
        Y[idx, lo + rng.randint(0, hi - lo, n)] = 1
    return out, Y


def _logged(fn, *args):
    lines = []

    class H(logging.Handler):
        def emit(self, rec):
            lines.append(rec.getMessage())
    h = H(); root = logging.getLogger(); level = root.level
    root.addHandler(h); root.setLevel(logging.INFO)
    try:
        fn(*args)
    finally:
        root.removeHandler(h); root.setLevel(level)
    return lines


def test_log_lines_are_those_of_the_report_before_the_split():
    from clairvoyante_amd import train
    assert _logged(train.log_evaluation, np.array(_COUNTS, dtype=np.int64)) == _LINES
    assert _logged(train.log_evaluation, list(_COUNTS)) == _LINES
    out, Y = _report_rows()
    assert train.evaluation_counts_host(*_split(out), Y).tolist() == _COUNTS
    assert _logged(train.EvaluateReport, *_split(out), Y) == _LINES          # the two composed: same signature, same lines


class _Mock(object):
    def predict(self, X):
        return tuple(np.zeros((len(X), k), dtype=np.float32) for k in (4, 2, 4, 6))


class _AlmostReal(_Mock):
    accepts_device_batches = True

    def evaluateCounts(self, X, Y, counts=None):
        raise AssertionError("not reached")


def test_cv_eval_switch(monkeypatch):
    from clairvoyante_amd import train
    monkeypatch.delenv("CV_EVAL", raising=False)
    assert train.eval_route(_Mock()) == "host" and train.eval_route(_AlmostReal()) == "device"
    for v in ("host", "device"):
        monkeypatch.setenv("CV_EVAL", v)
        assert train.eval_route(_Mock()) == "host"              # a mock or foreign model: always the host's arithmetic
        assert train.eval_route(_AlmostReal()) == v
    for v in ("gpu", "Device", "1"):
        monkeypatch.setenv("CV_EVAL", v)
        for m in (_Mock(), _AlmostReal()):
            with pytest.raises(ValueError, match="CV_EVAL"):
                train.eval_route(m)
        with pytest.raises(ValueError, match="CV_EVAL"):
            train.PredictAndReport(_Mock(), None, 0, [], [])


def test_resident_from_blocks_without_a_gpu_returns_its_inputs(monkeypatch):
    from clairvoyante_amd import train, utils_v2
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    x = np.zeros((700, 33, 4, 4), dtype=np.float32); y = np.zeros((700, 16))
    XC = [utils_v2.pack_array(x[s:s + 500]) for s in range(0, 701, 500)]
    YC = [utils_v2.pack_array(y[s:s + 500]) for s in range(0, 701, 500)]
    got = utils_v2.resident_from_blocks(700, XC, YC, None)
    assert got[0] is XC and got[1] is YC
    # ... and the drivers' helper leaves the set of a mock model alone wherever it runs
    got = train.resident_dataset(_Mock(), utils_v2, 700, XC, YC)
    assert got[0] is XC and got[1] is YC


def test_mock_model_report_goes_the_host_way(monkeypatch):
    """PredictAndReport with a model object that is not ours: predictions on the host, the same lines as before"""
    from clairvoyante_amd import train, utils_v2
    monkeypatch.setenv("CV_EVAL", "device")
    out, Y = _report_rows()
    x = np.arange(700, dtype=np.float32).reshape(-1, 1)
    XC = [utils_v2.pack_array(x[s:s + 500]) for s in range(0, 701, 500)]
    YC = [utils_v2.pack_array(Y[s:s + 500]) for s in range(0, 701, 500)]

    class M(object):
        def predict(self, X):
            return _split(out[X[:, 0].astype(np.int64)])
    lines = [l for l in _logged(train.PredictAndReport, M(), utils_v2, 700, XC, YC) if "time elapsed" not in l]
    assert lines == _LINES
