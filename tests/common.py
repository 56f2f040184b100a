"""Shared helpers of the parity tests (seeded weights + inputs, comparison metrics)."""
import numpy as np

HEADS = ((0, 4), (4, 6), (6, 10), (10, 16))
DEFAULT_VARIANT = 2031     # cv_create's default kernel selection (include/clairvoyante_amd.h, option "variant")


def bench_params(oracle, arch, seed=1):
    """The seeded weight set of the bench line and the parity tests (clairvoyante_amd/synth.py: needs nothing from
    oracle/; the first argument is kept for the call sites that pass the oracle module)."""
    from clairvoyante_amd import synth
    return synth.bench_params(arch, seed=seed)

# Forced launch shapes of the inference pass (tests/test_gpu_parity.py, tests/test_gpu_adversarial.py): each setting is
# applied on top of the defaults, which restore what the library chooses by size
FORCED_LAUNCH_SETTINGS = [{"infer_flat": 0}, {"infer_flat": 2}, {"infer_fc4_one_groups": 65536}, {"infer_fc4_one_groups": 0},
                          {"slim_waves": 4}, {"slim_waves": 8}, {"slim_small_groups": 65536}, {"slim_small_groups": 0},
                          {"infer_slab_groups": 0}, {"infer_slab_groups": 65536}, {"dense_rag": -1, "infer_slab_groups": 65536}]
FORCED_LAUNCH_SETTINGS += [{"dense_rag": s, "infer_slab_groups": 65536, "infer_flat": 2 if s % 2 else 0} for s in range(4, 15)]
FORCED_LAUNCH_DEFAULTS = {"infer_flat": 1, "infer_fc4_one_groups": 80, "slim_waves": 0, "slim_small_groups": -1,
                          "infer_slab_groups": -1, "dense_rag": 0}
# ... and the small-pass kernel sets
SMALL_PASS_SETTINGS = ({"dbg0": 5}, {"dbg0": 6}, {"dbg1": 4}, {"infer_fc4_one_groups": 0}, {"infer_fc4_one_groups": 65536},
                       {"slim_small_groups": 0}, {"slim_small_groups": 65536})
SMALL_PASS_DEFAULTS = {"dbg0": 0, "dbg1": 0, "infer_fc4_one_groups": 80, "slim_small_groups": -1}


def inputs(n, seed=5, stress=0):
    from clairvoyante_amd import synth
    x = synth.make_candidates(n, seed=seed).numpy()
    if stress:
        x = np.concatenate([x, synth.make_stress(stress, seed=seed).numpy() * np.float32(0.25)])
    return np.ascontiguousarray(x, dtype=np.float32)


def argmax_match(a, b):
    """per-head fraction of identical argmax (np.argmax semantics) between two [n,16] arrays"""
    return [float(np.mean(np.argmax(a[:, lo:hi], 1) == np.argmax(b[:, lo:hi], 1))) for lo, hi in HEADS]


def bitwise_frac(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.uint32)
    return float(np.mean(a == b))


# ---- adversarial regime (tests/test_gpu_adversarial.py): built on the CPU, so that the oracle and the device read the
# same bits

# the special values, as bit patterns: quiet NaN, negative NaN, signalling NaN, +-Inf, +-1e30, 3.4e38
SPECIAL_BITS = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7f800000, 0xff800000,
                         0x7149f2ca, 0xf149f2ca, 0x7f7fc99e], dtype=np.uint32)
DENORMALS = np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45], dtype=np.float32)


def adversarial_inputs(n, seed=7, specials=True):
    """[n,33,4,4] fp32: synthetic pileups, each transform on its own seeded share of the candidates -- scaled by 10^u
    (u uniform in [-3, 3]); whole position ranges zeroed, and ~10 % of the candidates zeroed outright; ~5 % of the
    elements -0.0; denormals (+-1e-40, +-1.4e-45); with `specials`, one special value (SPECIAL_BITS) at 1-4 positions of
    ~2 % of the candidates, written through the bit pattern so that a signalling NaN stays one."""
    from clairvoyante_amd import synth
    x = np.ascontiguousarray(synth.make_candidates(n, seed=seed).numpy(), dtype=np.float32)
    rng = np.random.RandomState(seed)
    share = rng.randint(0, 4, size=n)                  # 0: as drawn, 1: scaled, 2: zeroed ranges + -0.0, 3: denormals
    flat = x.reshape(n, -1)
    scaled = share == 1
    flat[scaled] *= (10.0 ** rng.uniform(-3.0, 3.0, size=int(scaled.sum()))).astype(np.float32)[:, None]
    for i in np.flatnonzero(share == 2):
        lo = rng.randint(0, 33); hi = rng.randint(lo + 1, 34)
        x[i, lo:hi] = 0.0
        neg = rng.rand(33 * 16) < 0.05
        flat[i, neg] = np.float32(-0.0)
    for i in np.flatnonzero(share == 3):
        k = rng.rand(33 * 16) < 0.05
        flat[i, k] = DENORMALS[rng.randint(0, 4, size=int(k.sum()))]
    flat[rng.rand(n) < 0.1] = 0.0
    if specials:
        bits = flat.view(np.uint32)
        for i in np.flatnonzero(rng.rand(n) < 0.02):
            bits[i, rng.randint(0, 33 * 16, size=rng.randint(1, 5))] = SPECIAL_BITS[rng.randint(0, len(SPECIAL_BITS))]
    return x


def adversarial_batch(n, kind, seed=7):
    """A finite training batch (x, y) of one adversarial kind: 'small' (inputs scaled by 1e-3), 'large' (by 30),
    'sparse' (position ranges zeroed, -0.0 sprinkled, ~10 % of the candidates all zero), 'denormal' (as 'sparse', with
    denormals sprinkled too: pre-activations in (-2^-25, 0) inside zeroed ranges)."""
    from clairvoyante_amd import synth
    xt, cls, rf, alt, il = synth.make_candidates(n, seed=seed, return_class=True)
    x = np.ascontiguousarray(xt.numpy(), dtype=np.float32)
    y = np.ascontiguousarray(synth.make_labels(cls, rf, alt, il).numpy(), dtype=np.float32)
    rng = np.random.RandomState(seed)
    if kind == "small":
        x *= np.float32(1e-3)
    elif kind == "large":
        x *= np.float32(30.0)
    elif kind in ("sparse", "denormal"):
        flat = x.reshape(n, -1)
        for i in range(n):
            lo = rng.randint(0, 33); hi = rng.randint(lo + 1, 34)
            x[i, lo:hi] = 0.0
        flat[rng.rand(*flat.shape) < 0.05] = np.float32(-0.0)
        k = rng.rand(*flat.shape) < 0.05
        if kind == "denormal":
            flat[k] = DENORMALS[rng.randint(0, 4, size=int(k.sum()))]
        flat[rng.rand(n) < 0.1] = 0.0
    else:
        raise ValueError(kind)
    assert np.isfinite(x).all()
    return x, y


def adversarial_params(arch, kind, seed=1):
    """'bench': bench_params; 'zero_bias': bench_params with every bias exactly 0; 'init': the reference initialiser
    (oracle.init_params: zero biases, conv1 unscaled -- the heads saturate on count data)."""
    if kind == "bench":
        return bench_params(None, arch, seed=seed)
    if kind == "zero_bias":
        return {k: (np.zeros_like(v) if k.endswith("bias") else v) for k, v in bench_params(None, arch, seed=seed).items()}
    if kind == "init":
        from oracle import cv_oracle
        return cv_oracle.init_params(arch, seed=seed)
    raise ValueError(kind)


def same_bits(a, b):
    """elementwise: identical fp32 bits, or both NaN (any payload, either sign)"""
    a = np.ascontiguousarray(a, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- the decision checker: callVar.py:58-87 restated per row (tests/test_gpu_adversarial.py, tests/test_host_golden.py) -----------------------------------------------------

def _descending(v):
    """indices of v in the order of np.sort(v)[::-1] / v.argsort()[::-1]: NaN above every number; equal values (NaN and
    NaN, +0 and -0) the higher index first"""
    return sorted(range(len(v)), key=lambda k: (v[k] != v[k], v[k] if v[k] == v[k] else 0.0, k), reverse=True)


def _argmax(v):
    """np.argmax: the first NaN, else the first maximum"""
    best = 0
    for k in range(len(v)):
        if v[k] != v[k]:
            return k
        if v[k] > v[best]:
            best = k
    return best


def decide(o16, x):
    """one candidate: o16 [16] fp32 network outputs, x [33,4,4] fp32 -> ([type, zygosity, length, base1, base2],
    [p1, p2, dp] fp32): the arg-maxes, the products of the best and second-best probability of each softmax head taken
    left to right in fp32, the two best bases, and dp as the builtin sum of fp32 values"""
    f = np.float32
    base, zyg, typ, ln = o16[0:4], o16[4:6], o16[6:10], o16[10:16]
    st, sz, sl = ([h[k] for k in _descending(h.tolist())] for h in (typ, zyg, ln))
    ob = _descending(base.tolist())
    with np.errstate(all="ignore"):
        p1 = (f(st[0]) * f(sz[0])) * f(sl[0])
        p2 = (f(st[1]) * f(sz[1])) * f(sl[1])
        F = 16
        dp = (((sum(x[F, :, 0]) + sum(x[F + 1, :, 1])) + sum(x[F + 1, :, 2])) + sum(x[F, :, 3]))
    return [_argmax(typ.tolist()), _argmax(zyg.tolist()), _argmax(ln.tolist()), ob[0], ob[1]], \
        np.array([p1, p2, dp], dtype=np.float32)


def decide_all(out16, x):
    calls = np.empty((out16.shape[0], 5), np.int32)
    quals = np.empty((out16.shape[0], 3), np.float32)
    for i in range(out16.shape[0]):
        calls[i], quals[i] = decide(out16[i], x[i])
    return calls, quals


def crafted_rows(n=10000, seed=3):
    """[n,16] fp32 head outputs written by hand: per head, values drawn at random or exact ties of 2-4 entries at 1.0,
    0.5 and 0.0, ties between +0 and -0, denormals, +-Inf, NaN in one entry or in all of them (several NaN patterns)"""
    rng = np.random.RandomState(seed)
    nan_bits = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fc01234], np.uint32)
    o = np.empty((n, 16), np.float32)
    bits = o.view(np.uint32)
    for i in range(n):
        for lo, hi in HEADS:
            w = hi - lo
            o[i, lo:hi] = rng.uniform(0.0, 1.0, w).astype(np.float32)
            mode = rng.randint(0, 9)
            pick = rng.permutation(w)
            if mode in (1, 2, 3):           # exact ties at 1.0 / 0.5 / 0.0 of 2-4 entries, the others below
                tie = (1.0, 0.5, 0.0)[mode - 1]
                o[i, lo:hi] = (tie - rng.uniform(0.01, 1.0, w)).astype(np.float32)
                o[i, lo + pick[:min(w, rng.randint(2, 5))]] = tie
            elif mode == 4:                 # +0 / -0
                o[i, lo:hi] = np.where(rng.rand(w) < 0.5, np.float32(0.0), np.float32(-0.0))
            elif mode == 5:                 # denormals, among zeros
                o[i, lo:hi] = rng.choice(np.array([1e-40, 1.4e-45, -1.4e-45, 0.0, -0.0, 1e-40], np.float32), w)
            elif mode == 6:                 # +-Inf in 1..w entries
                k = rng.randint(1, w + 1)
                o[i, lo + pick[:k]] = rng.choice(np.array([np.inf, -np.inf], np.float32), k)
            elif mode == 7:                 # NaN in one entry
                bits[i, lo + pick[0]] = nan_bits[rng.randint(0, 4)]
            elif mode == 8:                 # NaN in every entry
                bits[i, lo:hi] = nan_bits[rng.randint(0, 4, w)]
    return o
