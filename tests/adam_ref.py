"""Host reference of the optimizer step (csrc/cv_post.hip adam_one / apply_adam: TensorFlow 1's ApplyAdam on g + lambda*w
for kernels, g for biases) and of the (hi, lo) float pairs of the loss header (csrc/cv_train.hip t_loss_header).

step32 restates the device's arithmetic: one NumPy float32 operation per device operation, in the device's order.  The
library is compiled without contraction, fp32 division and square root are correctly rounded and denormals are kept,
so every operation is one IEEE-754 binary32 operation and the device must give step32's BITS.  step64 is the same
formula in float64 from the same fp32 inputs: what tests/test_adam_ref.py holds step32 to, and the device next to it.
NumPy only: nothing here needs the GPU or the library."""
import math

import numpy as np

F = np.float32
BETA1, BETA2, EPS = F(0.9), F(0.999), F(1e-8)
C1 = F(1) - BETA1          # 1 - beta1 and 1 - beta2 as the compiler folds them: fp32 differences of fp32 constants
C2 = F(1) - BETA2
U = 2.0 ** -24             # unit roundoff of binary32
# bounds of step32 (and of the device) against step64, in units of U, on well-conditioned inputs (well_conditioned):
# m1 is 3 roundings, v1 4, w1 about 9 of which the last is relative to w1 itself -- counted twice
BOUND_M, BOUND_V, BOUND_S = 8.0, 8.0, 16.0


def lr_t(lr, t):
    """float32 of double(float32(lr)) * sqrt(1 - 0.999**t) / (1 - 0.9**t), in double (apply_adam)"""
    return F(float(F(lr)) * math.sqrt(1.0 - 0.999 ** float(t)) / (1.0 - 0.9 ** float(t)))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def step32(w, m, v, g, is_kernel, lr_t, lam):
    """-> (w1, m1, v1), float32 arrays; every intermediate is rounded to float32"""
    w, m, v, g = _f32(w), _f32(m), _f32(v), _f32(g)
    lr_t, lam = F(lr_t), F(lam)
    with np.errstate(all="ignore"):
        gl = (g + (lam * w).astype(F)).astype(F)
        gi = np.where(is_kernel, gl, g).astype(F)
        m1 = (m + ((gi - m).astype(F) * C1).astype(F)).astype(F)
        v1 = (v + (((gi * gi).astype(F) - v).astype(F) * C2).astype(F)).astype(F)
        num = (m1 * lr_t).astype(F)
        den = (np.sqrt(v1).astype(F) + EPS).astype(F)
        w1 = (w - (num / den).astype(F)).astype(F)
    return w1, m1, v1


def step64(w, m, v, g, is_kernel, lr_t, lam):
    """-> (W, M, V, S), float64: the same formula from the same fp32 inputs, the fp32-rounded constants (1 - beta, eps,
    lr_t, lambda) widened; S is the step, W = w - S (returned as computed: w - W would lose a step below w's last
    float64 bit)"""
    w, m, v, g = (_f32(a).astype(np.float64) for a in (w, m, v, g))
    lr_t, lam, c1, c2, eps = float(F(lr_t)), float(F(lam)), float(C1), float(C2), float(EPS)
    with np.errstate(all="ignore"):
        gi = np.where(is_kernel, g + lam * w, g)
        M = m + (gi - m) * c1
        V = v + (gi * gi - v) * c2
        S = (M * lr_t) / (np.sqrt(V) + eps)
        W = w - S
    return W, M, V, S


def distances(w1, m1, v1, ref64):
    """worst distances of an fp32 result from step64's, in units of U: |m1 - M| / |M|, |v1 - V| / V and
    (|w1 - W| - U |W|) / |S| (what is left of w1's error after its own final rounding, relative to the step)"""
    W, M, V, S = ref64
    dm = np.abs(m1.astype(np.float64) - M) / np.abs(M)
    dv = np.abs(v1.astype(np.float64) - V) / V
    dw = (np.abs(w1.astype(np.float64) - W) - U * np.abs(W)) / np.abs(S)
    return float(dm.max() / U), float(dv.max() / U), float(dw.max() / U)


def well_conditioned(n, seed):
    """(w, m, v, g) on which the float64 bounds apply: sign(m) == sign(g) (no cancellation in m1), v > 0, |g| and |m|
    log-uniform in 1e-12 .. 1e6, v in 1e-24 .. 1e12 (no under- or overflow of g*g), w ~ 0.1 N(0, 1); to be used with lambda 0"""
    rng = np.random.RandomState(seed)
    sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    g = (sign * 10.0 ** rng.uniform(-12.0, 6.0, n)).astype(F)
    m = (sign * 10.0 ** rng.uniform(-12.0, 6.0, n)).astype(F)
    v = (10.0 ** rng.uniform(-24.0, 12.0, n)).astype(F)
    w = (0.1 * rng.standard_normal(n)).astype(F)
    return w, m, v, g


def is_kernel_mask(offsets):
    """bool per element of the flat buffer from the CV_NUM_PARAMS + 1 offsets of cv_param_buffer: the variables
    alternate kernel, bias -- an even variable index is a kernel"""
    offsets = [int(o) for o in offsets]
    mask = np.zeros(offsets[-1], dtype=bool)
    for p in range(0, len(offsets) - 1, 2):
        mask[offsets[p]:offsets[p + 1]] = True
    return mask


def split_hi_lo(d):
    """a double as the header's float pair: hi = float32(d), lo = float32(d - double(hi))"""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(all="ignore"):
        hi = d.astype(F)
        lo = (d - hi.astype(np.float64)).astype(F)
    return hi, lo


def join(hi, lo):
    """the double a reader of the header sees: double(hi) + double(lo)"""
    return np.asarray(hi, dtype=F).astype(np.float64) + np.asarray(lo, dtype=F).astype(np.float64)
