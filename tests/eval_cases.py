"""Inputs and the per-candidate definition shared by the tests of the evaluation report's counters
(tests/test_eval_counts_host.py, tests/test_gpu_eval.py)."""
import numpy as np

HEADS = ((0, 4), (4, 6), (6, 10), (10, 16))
CELLS = [0, 1, 2] + list(range(4, 60))              # the 59 counters in use: candidates, top-1, top-2 and the 56 matrix cells
NAN = float("nan")

# base-head rows whose order / argmax were checked with numpy by hand: (row, argsort()[::-1], np.argmax)
TABLE = (
    ([.5, .5, .1, .5], [3, 1, 0, 2], 0),
    ([NAN, 1, NAN, 0], [2, 0, 1, 3], 0),
    ([0, -0., 0, 0], [3, 2, 1, 0], 0),
    ([1, NAN, .2, .3], [1, 0, 3, 2], 1),
)


def counts_per_row(out16, Y):
    """the report's 64 counters, one candidate at a time, as the reference's evaluation loop reads: the base head
    through argsort()[::-1] of the prediction, the other heads through np.argmax of truth and prediction"""
    c = np.zeros(64, dtype=np.int64)
    for o, y in zip(out16, Y):
        c[0] += 1
        order = o[0:4].argsort()[::-1]
        truth = np.argmax(y[0:4])
        if truth == order[0]:
            c[1] += 1; c[2] += 1
        elif truth == order[1]:
            c[2] += 1
        for (lo, hi), off in zip(HEADS[1:], (4, 8, 24)):
            c[off + np.argmax(y[lo:hi]) * (hi - lo) + np.argmax(o[lo:hi])] += 1
    return c


def random_rows(n, seed, ydtype=np.float64):
    """(out16 [n,16] fp32, Y [n,16] ydtype): one-hot labels and confident predictions, both classes drawn uniformly and
    independently per head -- every cell of every matrix is hit from about a thousand candidates on"""
    rng = np.random.RandomState(seed)
    out = (rng.rand(n, 16) * 0.5).astype(np.float32)
    Y = np.zeros((n, 16), dtype=ydtype)
    idx = np.arange(n)
    for lo, hi in HEADS:
        out[idx, lo + rng.randint(0, hi - lo, n)] = np.float32(0.9)
        Y[idx, lo + rng.randint(0, hi - lo, n)] = 1
    return out, Y


def _head_patterns(w):
    """prediction or label patterns of a head of width w that the tie rules decide: ties, all equal, +0 / -0, NaN first,
    NaN later, NaN everywhere, all zero"""
    tie = [.5] * w; tie[w // 2] = .1
    zeros = [0.] * w; zeros[min(1, w - 1)] = -0.
    nan_late = [1.] + [.2] * (w - 1); nan_late[w - 1] = NAN
    nan_two = [NAN] + [1.] * (w - 1); nan_two[w - 1] = NAN
    return [tie, [.25] * w, zeros, nan_late, nan_two, [NAN] * w, [0.] * w, [-0.] * w]


def adversarial_rows(ydtype=np.float64):
    """(out16 [k,16] fp32, Y [k,16] ydtype): the TABLE rows and the head patterns, in the predictions and in the labels,
    against each other and against plain one-hot rows; and a label row of two float64 values that round to one float"""
    outs, ys = [], []
    plain_o, plain_y = random_rows(8, seed=77, ydtype=np.float64)
    pats = [_head_patterns(hi - lo) for lo, hi in HEADS]
    base_rows = [r for r, _, _ in TABLE] + pats[0]
    for j, b in enumerate(base_rows):
        for truth in range(4):                       # every truth index against every crafted base row
            o = plain_o[j % 8].copy(); y = plain_y[truth].copy()
            o[0:4] = b
            y[0:4] = 0; y[truth] = 1
            for h in (1, 2, 3):
                lo, hi = HEADS[h]
                o[lo:hi] = pats[h][(j + truth) % len(pats[h])]
            outs.append(o); ys.append(y)
    for j in range(len(pats[3])):                    # crafted LABELS: against plain and against crafted predictions
        for crafted in (False, True):
            o = plain_o[j % 8].copy(); y = plain_y[(j + 3) % 8].copy()
            for h, (lo, hi) in enumerate(HEADS):
                y[lo:hi] = pats[h][j]
                if crafted:
                    o[lo:hi] = pats[h][(j + 1) % len(pats[h])]
            outs.append(o); ys.append(y)
    y = plain_y[0].copy(); y[0:4] = [1, 1 + 2.0 ** -40, 0, 0]; y[4:6] = [1, 1 + 2.0 ** -40]
    outs.append(plain_o[0].copy()); ys.append(y)
    return np.array(outs, dtype=np.float32), np.array(ys, dtype=np.float64).astype(ydtype)


def planted(n, seed, ydtype=np.float64):
    """random_rows with the adversarial rows written over row 0, the last row and both sides of every 64-lane and
    256-thread boundary that n has (cycling through them, so that every size sees a different mix)"""
    out, Y = random_rows(n, seed, ydtype)
    ao, ay = adversarial_rows(ydtype)
    spots = sorted(set(p for p in [0, n - 1, 63, 64, 127, 128, 255, 256, 511, 512, n - 65, n - 64, n - 257, n - 256]
                       if 0 <= p < n))
    for k, p in enumerate(spots):
        j = (k * 7 + seed) % len(ao)
        out[p] = ao[j]; Y[p] = ay[j]
    if n >= 2048:                                     # every adversarial row once, in a run across a workgroup boundary
        s = 1024 - len(ao) // 2
        out[s:s + len(ao)] = ao; Y[s:s + len(ay)] = ay
    return out, Y
