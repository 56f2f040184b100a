"""tests/adam_ref.py on the host: step32 (the fp32 restatement of csrc/cv_post.hip adam_one that the device is held to bit
for bit in tests/test_gpu_optimizer.py) is the intended formula -- it stays within a few roundings of the same formula
in float64 -- and the (hi, lo) float pair of the loss header carries a double to 2^-49."""
import numpy as np
import pytest

import adam_ref as R

N = 2 ** 20


@pytest.fixture(scope="module")
def state():
    return R.well_conditioned(N, seed=11)


def test_constants_are_the_fp32_differences():
    # 1 - 0.9f and 1 - 0.999f are exact in fp32 (Sterbenz), so the widened constants of step64 are the device's
    assert float(R.C1) == 1.0 - float(np.float32(0.9)) and float(R.C2) == 1.0 - float(np.float32(0.999))
    assert R.lr_t(1e-3, 1).dtype == np.float32
    # t = 1: lr * sqrt(0.001) / 0.1; a large t: lr_t -> lr
    assert abs(float(R.lr_t(1e-3, 1)) - 1e-3 * np.sqrt(0.001) / 0.1) <= 2.0 ** -24 * 1e-3
    assert R.lr_t(1e-3, 10 ** 6) == np.float32(1e-3) and R.lr_t(0.0, 5) == 0.0


@pytest.mark.parametrize("t", [1, 2, 1000, 100000])
def test_step32_stays_within_its_roundings_of_float64(state, t):
    w, m, v, g = state
    assert (np.sign(m) == np.sign(g)).all() and (v > 0).all()
    lrt = R.lr_t(1e-3, t)
    kern = np.zeros(N, dtype=bool); kern[::2] = True          # lambda 0: the class of an element makes no difference
    w1, m1, v1 = R.step32(w, m, v, g, kern, lrt, 0.0)
    assert w1.dtype == m1.dtype == v1.dtype == np.float32
    W, M, V, S = R.step64(w, m, v, g, kern, lrt, 0.0)
    assert np.array_equal(W, w.astype(np.float64) - S)
    u = R.U
    dm, dv, dw = R.distances(w1, m1, v1, (W, M, V, S))
    print("t=%d: step32 against float64, worst distances m %.2f u, v %.2f u, w %.2f u of the step" % (t, dm, dv, dw))
    assert (np.abs(m1 - M) <= R.BOUND_M * u * np.abs(M)).all()
    assert (np.abs(v1 - V) <= R.BOUND_V * u * V).all()
    assert (np.abs(w1 - W) <= u * np.abs(W) + R.BOUND_S * u * np.abs(S)).all()
    assert (w1 != w).mean() > 0.5                               # most steps are not lost in w's rounding


def test_lambda_term_goes_to_kernels_only():
    w = np.array([2.0, 2.0, -4.0, -4.0], np.float32)
    z = np.zeros(4, np.float32)
    kern = np.array([True, False, True, False])
    w1, m1, v1 = R.step32(w, z, z, z, kern, R.lr_t(1e-3, 1), 0.25)
    assert np.array_equal(m1, np.array([0.5, 0.0, -1.0, 0.0], np.float32) * R.C1)
    assert np.array_equal(v1, np.array([0.25, 0.0, 1.0, 0.0], np.float32) * R.C2)
    assert w1[1] == w[1] and w1[3] == w[3] and w1[0] < w[0] and w1[2] > w[2]
    W, M, V, S = R.step64(w, z, z, z, kern, R.lr_t(1e-3, 1), 0.25)
    assert np.array_equal(M, np.array([0.5, 0.0, -1.0, 0.0]) * float(R.C1)) and S[1] == 0.0 and S[3] == 0.0


def test_is_kernel_mask_alternates_from_the_offsets():
    offs = [0, 5, 7, 7, 10, 11]                                 # an empty variable in between
    assert R.is_kernel_mask(offs).tolist() == [True] * 5 + [False] * 2 + [False] * 3 + [True]


def test_header_pairs_carry_a_double():
    rng = np.random.RandomState(3)
    d = np.where(rng.rand(100000) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-15.0, 15.0, 100000)
    d = np.concatenate([d, [0.0, 12345.678901234567, -9876.54321012345, 1.0, 2.0 ** -20]])
    hi, lo = R.split_hi_lo(d)
    assert hi.dtype == lo.dtype == np.float32
    assert np.array_equal(hi, d.astype(np.float32))
    assert (np.abs(R.join(hi, lo) - d) <= 2.0 ** -49 * np.abs(d)).all()
    assert (np.abs(lo) <= 2.0 ** -24 * np.abs(hi)).all()         # lo lies below half a unit of hi
    assert (np.abs(hi.astype(np.float64) - d)[np.abs(d) > 0] > 0).mean() > 0.9     # ... and is needed: hi alone is not d
