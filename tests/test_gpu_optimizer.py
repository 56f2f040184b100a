"""The optimizer step and the loss bookkeeping around it, directly on the flat buffers, against tests/adam_ref.py:

* adam_kernel (csrc/cv_post.hip) gives the BITS of adam_ref.step32 on states that mix typical values with the edges of
  the formula (cancellation in m1, eps deciding the step, g*g under- and overflowing, denormals, signed zeros, Inf, NaN),
  at small and large t, with and without the lambda term, one step and five chained ones; next to it the float64 formula
  under the bounds of tests/test_adam_ref.py;
* which elements get the lambda term: per tensor, at every tensor boundary inside a 16-byte quadruple, in the scalar tail;
* which bucket the step reads; cv_apply_adam_accumulate = cv_apply_adam + cv_loss_accumulate;
* the loss header as (hi, lo) pairs: the accumulator keeps the doubles (a float-only sum fails), the L2 term is divided by
  the rank count, the header a step writes agrees with the losses the host reads and with sum(w^2) in float64, and the L2
  term has the same bits whatever schedule the L2 kernel ran on.

Everything goes through the C ABI (m._lib / m._h); only the header tests of the last group run passes."""
import ctypes
import math

import numpy as np
import pytest

import adam_ref as R
import common

pytestmark = pytest.mark.gpu

HDR = 16                                    # CV_GRAD_HEADER: floats in front of the flat gradient
F = np.float32


# ---- plumbing -----------------------------------------------------------------------------------------------------

class _Model:
    """a model of one topology plus what the tests need of its flat buffers"""

    def __init__(self, arch):
        from clairvoyante_amd import _lib, clairvoyante_v3, clairvoyante_v3_slim
        self.arch = arch
        self.m = clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()
        self.lib, self.h, self.check = self.m._lib, self.m._h, _lib.check
        ptr = ctypes.c_void_p(); cnt = ctypes.c_int64(); offs = (ctypes.c_int64 * (_lib.NUM_PARAMS + 1))()
        self.check(self.lib.cv_param_buffer(self.h, ctypes.byref(ptr), ctypes.byref(cnt), offs))
        self.offs = [int(o) for o in offs]
        self.n = int(cnt.value)
        self.names = list(self.m._shapes)               # table order (cv_param_info)
        assert self.offs[0] == 0 and self.offs[-1] == self.n == self.m.numParameters and len(self.names) == _lib.NUM_PARAMS
        assert all(("kernel" in nm) == (p % 2 == 0) for p, nm in enumerate(self.names))
        self.kern = R.is_kernel_mask(self.offs)
        total = ctypes.c_int64(); hdr = ctypes.c_int64()
        self.check(self.lib.cv_grad_bucket_info(self.h, ctypes.byref(total), ctypes.byref(hdr), None))
        assert hdr.value == HDR and total.value == self.n + HDR
    
    def put(self, which, a):
        import torch
        a = np.ascontiguousarray(a, dtype=np.float32)
        assert a.shape == (self.n,)
        t = torch.from_numpy(a).cuda()
        self.check(self.lib.cv_flat_copy(self.h, which, ctypes.c_void_p(t.data_ptr()), 1, None))
        torch.cuda.synchronize()

    def get(self, which):
        import torch
        t = torch.empty(self.n, dtype=torch.float32, device="cuda")
        self.check(self.lib.cv_flat_copy(self.h, which, ctypes.c_void_p(t.data_ptr()), 0, None))
        torch.cuda.synchronize()
        return t.cpu().numpy()

    def put_state(self, w, m, v, g=None):
        self.put(0, w); self.put(2, m); self.put(3, v)
        if g is not None:
            self.put(1, g)

    def state(self):
        return self.get(0), self.get(2), self.get(3)

    def adam(self, lr, lam, t, accumulate=False):
        import torch
        fn = self.lib.cv_apply_adam_accumulate if accumulate else self.lib.cv_apply_adam
        self.check(fn(self.h, ctypes.c_float(lr), ctypes.c_float(lam), t, None))
        torch.cuda.synchronize()

    def bucket(self):
        import torch
        return torch.zeros(self.n + HDR, dtype=torch.float32, device="cuda")

    def bind(self, t):
        self.check(self.lib.cv_bind_grad_bucket(self.h, None if t is None else ctypes.c_void_p(t.data_ptr()),
                                                0 if t is None else t.numel()))

    def read_acc(self, reset):
        losses = (ctypes.c_double * 6)(); steps = ctypes.c_int64()
        self.check(self.lib.cv_loss_read(self.h, losses, ctypes.byref(steps), reset, None))
        return list(losses), int(steps.value)

    def accumulate(self):
        import torch
        self.check(self.lib.cv_loss_accumulate(self.h, None))
        torch.cuda.synchronize()

    def where(self, i):
        p = int(np.searchsorted(self.offs, i, side="right")) - 1
        return "%s + %d (flat %d of %d)" % (self.names[p], i - self.offs[p], i, self.n)


@pytest.fixture(scope="module", params=["full", "slim"])
def mdl(request):
    md = _Model(request.param)
    yield md
    md.bind(None)
    md.m.close()


CLASSES = ("typical, m and g of one sign", "typical, m and g of opposite signs", "g = -9 m: m1 cancels", "g = m = v = 0",
           "|g| ~ 1e-9, v ~ 1e-18: eps decides the step", "g = +-1e-30: g*g underflows", "denormal g, m, v", "+-0 in g, m, v",
           "g = +-1e20 / +-3e38: g*g overflows", "g = +-Inf / NaN")
ZERO, OVERFLOW, NONFINITE = 3, 8, 9


def mixed_state(n, seed, finite_only=False):
    """(w, m, v, g, cls): every element of one class of CLASSES, drawn per element; the non-finite class in 48 elements"""
    rng = np.random.RandomState(seed)
    cls = rng.randint(0, 9, n)
    if not finite_only:
        cls[rng.choice(n, 48, replace=False)] = NONFINITE
    s = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    s2 = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    mag = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, n)
    w = (0.1 * rng.standard_normal(n)).astype(F)
    g = (s * mag(-6, -1)).astype(F)
    m = (s * mag(-6, -1)).astype(F)
    v = mag(-12, -2).astype(F)
    k = cls == 1
    m[k] = -m[k]
    k = cls == 2                      # -9 m, a few units in the last place around it
    g[k] = (-9.0 * m[k].astype(np.float64) * (1.0 + rng.uniform(-3e-7, 3e-7, n)[k])).astype(F)
    k = cls == ZERO
    g[k] = 0; m[k] = 0; v[k] = 0
    k = cls == 4
    g[k] = (s * rng.uniform(0.5, 2.0, n) * 1e-9)[k].astype(F)
    m[k] = (s2 * rng.uniform(0.5, 2.0, n) * 1e-9)[k].astype(F)
    v[k] = (rng.uniform(0.25, 4.0, n) * 1e-18)[k].astype(F)
    k = cls == 5
    g[k] = (s * 1e-30)[k].astype(F)
    m[k] = (s2 * mag(-32, -28))[k].astype(F)
    v[k] = rng.choice(np.array([0.0, 1e-40, 1e-30, 1e-20], F), n)[k]
    k = cls == 6                      # denormals through their bit patterns, any mantissa
    sign = (rng.randint(0, 2, (2, n)).astype(np.uint32) << np.uint32(31))
    den = rng.randint(1, 0x800000, (3, n)).astype(np.uint32)
    g[k] = (den[0] | sign[0]).view(F)[k]; m[k] = (den[1] | sign[1]).view(F)[k]; v[k] = den[2].view(F)[k]
    k = cls == 7
    z = np.array([0.0, -0.0], F)
    g[k] = rng.choice(z, n)[k]; m[k] = rng.choice(z, n)[k]; v[k] = rng.choice(z, n)[k]
    w[k] = np.where(rng.rand(n) < 0.5, rng.choice(z, n), w)[k]
    k = cls == OVERFLOW
    g[k] = rng.choice(np.array([1e20, -1e20, 3e38, -3e38], F), n)[k]
    k = cls == NONFINITE
    g[k] = rng.choice(np.array([np.inf, -np.inf, np.nan], F), n)[k]
    assert all((cls == c).any() for c in range(9)) and (finite_only or (cls == NONFINITE).sum() == 48)
    assert np.isfinite(w).all() and np.isfinite(m).all() and np.isfinite(v).all() and (v[cls != 7] >= 0).all()
    return w, m, v, g, cls


def assert_bits(md, what, got, want, cls=None):
    ok = common.same_bits(got, want)
    if ok.all():
        return
    bad = np.flatnonzero(~ok)
    i = int(bad[0])
    by_class = "" if cls is None else "; failing classes: %s" % sorted({CLASSES[c] for c in np.unique(cls[bad])})
    raise AssertionError("%s: %d of %d elements differ from the reference; first at %s%s: device %r (0x%08x), reference %r (0x%08x)%s"
                         % (what, bad.size, got.size, md.where(i), "" if cls is None else ", class '%s'" % CLASSES[cls[i]],
                            got[i], got.view(np.uint32)[i], want[i], want.view(np.uint32)[i], by_class))


_STATES = {}


def _mixed(md, seed=21, finite_only=False):
    key = (md.n, seed, finite_only)
    if key not in _STATES:
        _STATES[key] = mixed_state(md.n, seed, finite_only)
    return _STATES[key]


def _lambda():
    from clairvoyante_amd import param
    return float(param.l2RegularizationLambda)


# ---- a. one step, bit for bit --------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [1, 2, 7, 1000, 10 ** 6])
@pytest.mark.parametrize("lr,lam", [(1e-3, 0.0), (1e-3, None), (0.0, 0.5)], ids=["lambda0", "lambda", "lr0"])
def test_one_step_has_the_bits_of_step32(mdl, t, lr, lam):
    lam = _lambda() if lam is None else lam
    w, m, v, g, cls = _mixed(mdl)
    mdl.put_state(w, m, v, g)
    mdl.adam(lr, lam, t)
    w1, m1, v1 = mdl.state()
    g1 = mdl.get(1)
    rw, rm, rv = R.step32(w, m, v, g, mdl.kern, R.lr_t(lr, t), lam)
    assert_bits(mdl, "m", m1, rm, cls); assert_bits(mdl, "v", v1, rv, cls); assert_bits(mdl, "w", w1, rw, cls)
    assert_bits(mdl, "gradient (must be left alone)", g1, g, cls)
    # what the classes are there for, stated on the device's output
    fin = cls != NONFINITE
    assert not np.isnan(w1[fin]).any() and not np.isnan(m1[fin]).any() and not np.isnan(v1[fin]).any()
    assert np.isnan(w1[cls == NONFINITE]).all()
    k = cls == OVERFLOW
    assert np.isposinf(v1[k]).all() and np.isfinite(m1[k]).all() and np.array_equal(w1[k].view(np.uint32), w[k].view(np.uint32))
    k = (cls == ZERO) & (~mdl.kern | (lam == 0.0))
    assert np.array_equal(w1[k].view(np.uint32), w[k].view(np.uint32)) and not m1[k].any() and not v1[k].any()
    if lr == 0.0:
        assert (w1[fin] == w[fin]).all()                          # no step ...
        zw, zm, zv = R.step32(w, m, v, g, mdl.kern, 0.0, 0.0)     # ... while the slots take the lambda term: kernels only
        typical = (cls <= 1)
        assert (m1 != zm)[typical & mdl.kern].mean() > 0.9 and (v1 != zv)[typical & mdl.kern].mean() > 0.9
        assert common.same_bits(m1, zm)[~mdl.kern].all() and common.same_bits(v1, zv)[~mdl.kern].all()
    else:
        assert (w1 != w)[cls <= 1].mean() > 0.9


@pytest.mark.parametrize("t", [1, 1000])
def test_one_step_stays_within_the_float64_bounds(mdl, t):
    """the float64 leg: on well-conditioned inputs (m and g of one sign, v > 0, lambda 0) the device lies within the
    bounds tests/test_adam_ref.py holds step32 to -- were device and step32 ever to disagree, this says who left the formula"""
    w, m, v, g = R.well_conditioned(mdl.n, seed=31)
    mdl.put_state(w, m, v, g)
    lrt = R.lr_t(1e-3, t)
    mdl.adam(1e-3, 0.0, t)
    w1, m1, v1 = mdl.state()
    W, M, V, S = R.step64(w, m, v, g, mdl.kern, lrt, 0.0)
    dm, dv, dw = R.distances(w1, m1, v1, (W, M, V, S))
    print("\n%s t=%d: device against float64, worst distances m %.2f u, v %.2f u, w %.2f u of the step" % (mdl.arch, t, dm, dv, dw))
    u = R.U
    assert (np.abs(m1 - M) <= R.BOUND_M * u * np.abs(M)).all()
    assert (np.abs(v1 - V) <= R.BOUND_V * u * V).all()
    assert (np.abs(w1 - W) <= u * np.abs(W) + R.BOUND_S * u * np.abs(S)).all()
    rw, rm, rv = R.step32(w, m, v, g, mdl.kern, lrt, 0.0)
    assert_bits(mdl, "m", m1, rm); assert_bits(mdl, "v", v1, rv); assert_bits(mdl, "w", w1, rw)


# ---- b. which elements get lambda ----------------------------------------------------------------------------------

def test_lambda_term_reaches_kernels_only_element_by_element(mdl):
    n, offs = mdl.n, mdl.offs
    zero = np.zeros(n, F)
    mdl.put_state(np.ones(n, F), zero, zero, zero)
    mdl.adam(1e-3, 0.25, 1)
    w1, m1, v1 = mdl.state()
    km, kv = F(0.25) * R.C1, F(0.0625) * R.C2                    # exact products: gi = 0.25 on a kernel, 0 on a bias
    want = lambda i: (km, kv) if mdl.kern[i] else (F(0), F(0))

    def check(i, why):
        wm, wv = want(i)
        assert m1[i] == wm and v1[i] == wv and (w1[i] < 1 if mdl.kern[i] else w1[i] == 1), \
            "%s: %s: m1 %r v1 %r w1 %r, a %s" % (why, mdl.where(i), m1[i], v1[i], w1[i], "kernel" if mdl.kern[i] else "bias")
    for p, name in enumerate(mdl.names):
        lo, hi = offs[p], offs[p + 1]
        assert hi > lo
        check(lo, "first element"); check(hi - 1, "last element")
        assert (m1[lo:hi] == want(lo)[0]).all() and (v1[lo:hi] == want(lo)[1]).all(), name
        assert ((w1[lo:hi] < 1) if p % 2 == 0 else (w1[lo:hi] == 1)).all(), name
    # the kernel works on quadruples of the flat buffer and decides per element: every quadruple a tensor boundary cuts
    straddling = sorted({b // 4 for b in offs[1:-1] if b % 4})
    for q in straddling:
        for i in range(4 * q, min(4 * q + 4, n)):
            check(i, "quadruple %d holds a tensor boundary" % q)
    # ... and the elements behind the last whole quadruple, which a scalar loop updates
    for i in range(n - n % 4, n):
        check(i, "scalar tail")
    if mdl.arch == "slim":                                        # (18-float fc5/bias, heads of 4, 2, 4, 6: both must occur here)
        assert straddling and n % 4 != 0, (straddling, n)
        assert any(len({bool(mdl.kern[i]) for i in range(4 * q, min(4 * q + 4, n))}) == 2 for q in straddling)


# ---- c. five chained steps ------------------------------------------------------------------------------------------

def test_five_chained_steps_have_the_bits_of_step32(mdl):
    lam = _lambda()
    w, m, v, _g, cls = _mixed(mdl)
    mdl.put_state(w, m, v)
    rng = np.random.RandomState(44)
    for t in range(1, 6):
        # a fresh gradient; slots and weights stay on the device.  (An overflowed v is Inf for good and NaN one step later:
        # only 2 % of the overflowing gradients are kept, so that most of the buffer stays on finite values to the end.)
        g, gcls = (np.roll(a, 7919 * t) for a in _mixed(mdl)[3:5])   # (rolled: every class of gradient meets every class of slot)
        tame = (gcls >= OVERFLOW) & (rng.rand(mdl.n) > 0.02)
        g[tame] = (np.where(rng.rand(mdl.n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, -1.0, mdl.n)).astype(F)[tame]
        mdl.put(1, g)
        mdl.adam(1e-3, lam, t)
        w, m, v = R.step32(w, m, v, g, mdl.kern, R.lr_t(1e-3, t), lam)
        w1, m1, v1 = mdl.state()
        assert_bits(mdl, "step %d: m" % t, m1, m); assert_bits(mdl, "step %d: v" % t, v1, v); assert_bits(mdl, "step %d: w" % t, w1, w)
    assert np.isfinite(w).mean() > 0.9 and np.isnan(w).any()


# ---- d. the bucket the step reads -----------------------------------------------------------------------------------

def test_the_step_reads_the_bound_bucket(mdl):
    import torch
    lam = _lambda()
    w, m, v, _g, _cls = _mixed(mdl, finite_only=True)
    A, B, C = (np.roll(_g, 7919 * k) for k in range(3))
    assert not np.array_equal(A, B) and not np.array_equal(B, C)
    want = {k: R.step32(w, m, v, G, mdl.kern, R.lr_t(1e-3, 3), lam) for k, G in (("A", A), ("B", B), ("C", C))}
    ta, tc = mdl.bucket(), mdl.bucket()
    tc[HDR:] = torch.from_numpy(C).cuda()

    def step_is(k, why):
        mdl.put_state(w, m, v)
        mdl.adam(1e-3, lam, 3)
        for name, got, ref in zip("wmv", mdl.state(), want[k]):
            assert_bits(mdl, "%s: %s after a step that must read gradient %s" % (why, name, k), got, ref)
    try:
        mdl.bind(ta)
        mdl.put(1, A)                                              # which = 1 is the BOUND bucket's gradient
        assert np.array_equal(ta[HDR:].cpu().numpy().view(np.uint32), A.view(np.uint32)) and not ta[:HDR].any()
        mdl.bind(None)
        mdl.put(1, B)                                              # ... and now the library's own
        assert np.array_equal(ta[HDR:].cpu().numpy().view(np.uint32), A.view(np.uint32))
        mdl.bind(ta)
        step_is("A", "caller's bucket bound")
        mdl.bind(None)
        step_is("B", "unbound")
        mdl.bind(tc)
        step_is("C", "a second bucket bound")
        mdl.bind(None)
        step_is("B", "unbound again")
    finally:
        mdl.bind(None)


# ---- e. cv_apply_adam_accumulate and the accumulator ---------------------------------------------------------------

def _header(doubles5, count=1.0):
    """16 header floats from the five losses as doubles: (hi, lo) pairs, the rank count, zeros"""
    h = np.zeros(HDR, F)
    hi, lo = R.split_hi_lo(np.asarray(doubles5, np.float64))
    h[0:10:2] = hi; h[1:10:2] = lo; h[10] = count
    return h


def test_accumulating_step_is_the_plain_step_plus_the_header(mdl):
    import torch
    lam = _lambda()
    w, m, v, g, _cls = _mixed(mdl, finite_only=True)
    d = [12345.678901234567, 0.5 + 2.0 ** -30, -9876.54321012345, 0.0, 77.000000123456789]
    hdr = _header(d)
    assert all(abs(float(hdr[2 * k + 1])) < 2.0 ** -24 * abs(float(hdr[2 * k])) and hdr[2 * k + 1] != 0 for k in (0, 1, 2, 4))
    b = mdl.bucket()
    try:
        mdl.bind(b)
        b[:HDR] = torch.from_numpy(hdr).cuda(); mdl.put(1, g)
        before = b.cpu().numpy()
        mdl.read_acc(1)
        mdl.put_state(w, m, v); mdl.adam(1e-3, lam, 4)
        plain = mdl.state()
        assert mdl.read_acc(0) == ([0.0] * 6, 0)                  # cv_apply_adam leaves the accumulator alone
        mdl.put_state(w, m, v); mdl.adam(1e-3, lam, 4, accumulate=True)
        for name, got, ref in zip("wmv", mdl.state(), plain):
            assert_bits(mdl, name + " after cv_apply_adam_accumulate against cv_apply_adam", got, ref)
        for name, got, ref in zip("wmv", plain, R.step32(w, m, v, g, mdl.kern, R.lr_t(1e-3, 4), lam)):
            assert_bits(mdl, name, got, ref)
        assert np.array_equal(b.cpu().numpy().view(np.uint32), before.view(np.uint32))      # header and gradient untouched
        j = R.join(hdr[0:10:2], hdr[1:10:2])
        losses, steps = mdl.read_acc(0)
        assert steps == 1 and losses[:5] == [float(x) for x in j] and losses[5] == (((j[0] + j[1]) + j[2]) + j[3]) + j[4]
        assert all(abs(a - e) <= 2.0 ** -47 * abs(e) for a, e in zip(losses[:5], d))
        mdl.adam(1e-3, lam, 5)                                    # a plain step in between adds nothing
        assert mdl.read_acc(0) == (losses, 1)                     # reset = 0 keeps it ...
        assert mdl.read_acc(1) == (losses, 1)
        assert mdl.read_acc(0) == ([0.0] * 6, 0)                  # ... reset = 1 zeroed it
    finally:
        mdl.bind(None)


@pytest.mark.parametrize("path", ["cv_apply_adam_accumulate", "cv_loss_accumulate"])
def test_accumulator_keeps_the_doubles_over_fifty_steps(mdl, path):
    """Fifty headers whose lo halves matter: the accumulated sums equal the math.fsum of the joined doubles to K 2^-52 (K
    double additions, and the terms nearly all of one sign).  Adding the hi halves alone, or adding in fp32, is off by ~1e-8."""
    import torch
    K = 50
    w, m, v, g, _cls = _mixed(mdl, finite_only=True)
    base = np.array([12345.678901234567, 2345.6789012345678, 345.67890123456789, 45.678901234567891, 5.6789012345678912])
    doubles = [base * (1.0 + 0.01 * k) + 0.123456789012345 * k for k in range(K)]
    doubles[7] = -0.3 * base                                       # a negative header and a zero one
    doubles[13] = np.zeros(5)
    headers = [_header(d) for d in doubles]
    joined = np.array([R.join(h[0:10:2], h[1:10:2]) for h in headers])            # [K, 5]
    want = [math.fsum(joined[:, j]) for j in range(5)]
    hi_only = [math.fsum(float(h[2 * j]) for h in headers) for j in range(5)]
    assert all(abs(hi_only[j] - want[j]) > 100 * K * 2.0 ** -52 * abs(want[j]) for j in range(5))   # the lo halves are needed
    b = mdl.bucket()
    try:
        mdl.bind(b)
        mdl.put_state(w, m, v, g)
        mdl.read_acc(1)
        for k, h in enumerate(headers):
            b[:HDR] = torch.from_numpy(h).cuda()
            if path == "cv_loss_accumulate":
                mdl.accumulate()
            else:
                mdl.adam(1e-3, 0.0, k + 1, accumulate=True)
        losses, steps = mdl.read_acc(0)
        assert steps == K
        for j in range(5):
            assert abs(losses[j] - want[j]) <= K * 2.0 ** -52 * abs(want[j]), (j, losses[j], want[j], hi_only[j])
        assert losses[5] == (((losses[0] + losses[1]) + losses[2]) + losses[3]) + losses[4]
        # the same additions in the same order, stated exactly
        acc = np.zeros(5)
        for row in joined:
            acc = acc + row
        assert losses[:5] == [float(x) for x in acc]
        assert mdl.read_acc(1) == (losses, K) and mdl.read_acc(0) == ([0.0] * 6, 0)
    finally:
        mdl.bind(None)


# ---- f. the rank count ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["cv_apply_adam_accumulate", "cv_loss_accumulate"])
@pytest.mark.parametrize("count,div", [(0.0, 1.0), (0.4, 1.0), (1.0, 1.0), (2.0, 2.0), (4.0, 4.0)])
def test_l2_term_is_divided_by_the_rank_count(mdl, path, count, div):
    import torch
    d = [12345.678901234567, 2345.6789012345678, -345.67890123456789, 45.678901234567891, 5.6789012345678912]
    hdr = _header(d, count=count)
    j = R.join(hdr[0:10:2], hdr[1:10:2])
    b = mdl.bucket()
    try:
        mdl.bind(b)
        b[:HDR] = torch.from_numpy(hdr).cuda()
        mdl.read_acc(1)
        if path == "cv_loss_accumulate":
            mdl.accumulate()
        else:
            w, m, v, g, _cls = _mixed(mdl, finite_only=True)
            mdl.put_state(w, m, v, g)
            mdl.adam(1e-3, 0.0, 1, accumulate=True)
        losses, steps = mdl.read_acc(1)
        assert steps == 1
        assert losses[:4] == [float(x) for x in j[:4]]            # the data losses are sums over the ranks: never divided
        assert losses[4] == float(j[4]) / div, (losses[4], float(j[4]), div)
    finally:
        mdl.bind(None)


# ---- g. the header a step writes ------------------------------------------------------------------------------------

def _grad(md, x, y, n, lam):
    import torch
    losses = (ctypes.c_double * 6)()
    md.check(md.lib.cv_grad(md.h, ctypes.c_void_p(x.data_ptr()) if n else None, ctypes.c_void_p(y.data_ptr()) if n else None, n,
                            ctypes.c_float(0.0), ctypes.c_float(lam), ctypes.c_uint64(5), ctypes.c_uint64(1), losses, None))
    torch.cuda.synchronize()
    return list(losses)


def _batch(n, seed=61):
    from clairvoyante_amd import synth
    xt, cls, rf, alt, il = synth.make_candidates(max(n, 1), seed=seed, device="cuda", return_class=True)
    return xt[:n].contiguous(), synth.make_labels(cls, rf, alt, il)[:n].contiguous()


def _l2_float64(md, lam):
    """lambda * sum(w^2) / 2 over the nine kernels in float64 (math.fsum: the correctly rounded sum), lambda as the fp32 it is"""
    w = md.get(0).astype(np.float64)
    return float(F(lam)) * 0.5 * math.fsum((w[md.kern] ** 2).tolist())


def _check_header(md, hdr, losses, n):
    for k in range(5):
        d = losses[k]
        assert hdr[2 * k] == F(d), (k, hdr[2 * k], d)
        assert abs(float(R.join(hdr[2 * k], hdr[2 * k + 1])) - d) <= 2.0 ** -47 * abs(d), (k, hdr[2 * k], hdr[2 * k + 1], d)
    assert hdr[10] == 1.0 and not hdr[11:].any() and np.array_equal(hdr[11:].view(np.uint32), np.zeros(5, np.uint32))
    assert losses[5] == losses[0] + losses[1] + losses[2] + losses[3] + losses[4]
    if n == 0:
        assert losses[:4] == [0.0] * 4
    else:
        assert all(np.isfinite(l) and l > 0 for l in losses[:4])


def test_header_of_a_step_carries_the_losses_and_the_float64_l2_term(mdl):
    import torch
    lam = _lambda()
    mdl.m.setParameters(common.bench_params(None, mdl.arch))
    x, y = _batch(16)
    b = mdl.bucket()
    try:
        mdl.bind(b)
        b[:HDR] = float("nan")
        losses = _grad(mdl, x, y, 16, lam)
        hdr = b[:HDR].cpu().numpy()
        _check_header(mdl, hdr, losses, 16)
        want = _l2_float64(mdl, lam)
        got = float(R.join(hdr[8], hdr[9]))
        print("\n%s: L2 term %.17g, float64 %.17g, relative distance %.3g" % (mdl.arch, got, want, abs(got - want) / want))
        assert want > 0 and abs(got - want) <= 2.0 ** -30 * want
        assert bool(torch.isfinite(b[HDR:]).all()) and float(b[HDR:].abs().max()) > 0
    finally:
        mdl.bind(None)


def test_l2_term_is_squared_and_added_in_float64(mdl):
    """every kernel element the same c whose fp32 square is 0.27 units of the last place away from c*c: the rounding of
    every term points the same way, so squares taken in fp32 (or an fp32 sum) miss 2^-30, which random weights would
    let average out.  The exact sum is count * c*c, c*c exact in float64."""
    import torch
    lam = _lambda()
    c = F(0.001)
    exact = float(c) * float(c)
    assert abs(float(c * c) - exact) > 2.0 ** -28 * exact          # an fp32 product is visibly off at 2^-30
    mdl.put(0, np.where(mdl.kern, c, F(0)))
    x, y = _batch(16)
    b = mdl.bucket()
    try:
        mdl.bind(b)
        b[:HDR] = float("nan")
        losses = _grad(mdl, x, y, 16, lam)
        hdr = b[:HDR].cpu().numpy()
        _check_header(mdl, hdr, losses, 16)
        want = _l2_float64(mdl, lam)
        assert abs(want - float(F(lam)) * 0.5 * int(mdl.kern.sum()) * exact) <= 2.0 ** -50 * want
        got = float(R.join(hdr[8], hdr[9]))
        assert abs(got - want) <= 2.0 ** -30 * want, (got, want, abs(got - want) / want)
    finally:
        mdl.bind(None)


def test_l2_term_has_the_same_bits_on_every_schedule(mdl):
    """n = 0 (an empty rank: the L2 kernel at the end of the step), 16 and 8 192 (launched behind the first layer, on the
    side stream), 8 208 (513 groups: next to the forward pass): the division by the rank count after an all-reduce assumes
    that all of them write the same (hi, lo) pair"""
    import torch
    lam = _lambda()
    mdl.m.setParameters(common.bench_params(None, mdl.arch))
    x, y = _batch(8208)
    b = mdl.bucket()
    pairs = {}
    try:
        mdl.bind(b)
        for n in (0, 16, 8192, 8208):
            b[:HDR] = float("nan")
            losses = _grad(mdl, x[:n], y[:n], n, lam)
            hdr = b[:HDR].cpu().numpy()
            _check_header(mdl, hdr, losses, n)
            pairs[n] = hdr[8:10].view(np.uint32).tolist()
            if n == 0:
                assert not b[HDR:].any()                          # an empty rank contributes a zero gradient
        assert len({tuple(p) for p in pairs.values()}) == 1, pairs
        assert np.isfinite(np.array(pairs[0], np.uint32).view(F)).all() and pairs[0][0] != 0
    finally:
        mdl.bind(None)
