"""Planted candidates: batches in which every candidate but a chosen few is EMPTY (tests/test_planted_ref.py on the
CPU, tests/test_gpu_planted.py on the device).

With every bias exactly 0 and dropout off, a candidate whose pileup is all zeros has zero activations in every layer:
its contribution to each of the nine */kernel gradients is exactly +-0, its loss parts are the constants
[1, ln 2, ln 4, ln 6, 0] for a one-hot label, and its bias gradients are one fixed vector.  So in a batch of n empty
candidates with K real ones planted at chosen positions the kernel gradients are those of the planted candidates
alone, whatever n is: the tolerance of a comparison is relative to THEIR gradient, and one planted candidate lost,
counted twice or multiplied with a neighbour's gradient is an error of the order of the whole tensor -- which a dense
random batch of the same size hides below its rounding allowance (one candidate carries 1/n of such a sum).

The references are the oracle's own sums in double, one candidate at a time (oracle.loss_grad(..., f64=True), lambda
0, the zero-bias bench weights), computed once per process.
"""
import functools
import math

import numpy as np

import common

M = 64                         # pool members
# synth seed of the pool.  What a planted batch can tell apart is set by its WEAKEST member (a candidate the heads are
# sure of has head gradients a hundred times below its neighbours'): of the seeds 1..11 this one has the strongest
# weakest member on both topologies (margin() of all 64 at 1e-4: 50 x slim, 64 x full; seed 5: 1.0 x slim)
POOL_SEED = 11
HOT = (0, 5, 6, 10)            # the empty candidates' label: one entry of each head
EMPTY_PARTS = np.array([1.0, math.log(2.0), math.log(4.0), math.log(6.0), 0.0])      # loss1..loss4, lossL2
EMPTY_LOSS = float(EMPTY_PARTS.sum())                                                # 4.871201010907891
MARGIN_MIN = 10.0              # the share of the weakest planted candidate over the allowed distance, at least

KERNELS = ("conv1/kernel", "conv2/kernel", "conv3/kernel", "fc4/kernel", "fc5/kernel", "YBaseChangeSigmoid/kernel",
           "YZygosityFC/kernel", "YVarTypeFC/kernel", "YIndelLengthFC/kernel")
# each element of these is ONE product of a planted candidate plus zeros: no summation order can move it
ONE_PRODUCT = KERNELS[3:]


def y0():
    y = np.zeros(16, np.float32)
    y[list(HOT)] = 1.0
    return y


@functools.lru_cache(maxsize=None)
def candidates(m=M, seed=POOL_SEED):
    """the pool's pileups and labels: ([m,33,4,4], [m,16]) fp32, read-only"""
    from clairvoyante_amd import synth
    xt, cls, rf, alt, il = synth.make_candidates(m, seed=seed, return_class=True)
    x = np.ascontiguousarray(xt.numpy(), dtype=np.float32)
    y = np.ascontiguousarray(synth.make_labels(cls, rf, alt, il).numpy(), dtype=np.float32)
    assert (np.abs(x).reshape(m, -1).max(axis=1) > 0).all()          # no pool member is empty itself
    x.setflags(write=False); y.setflags(write=False)
    return x, y


class Pool(object):
    """arch, P (zero-bias bench weights), x / y (candidates()), g[name]: [m, ...] float64 per-member gradients,
    parts: [m, 5] float64 loss parts; g_empty[name] / parts_empty: the same of one empty candidate labelled y0()"""


@functools.lru_cache(maxsize=None)
def pool(arch, m=M, seed=POOL_SEED):
    from oracle import cv_oracle as O
    O.build()
    pl = Pool()
    pl.arch, pl.m = arch, m
    pl.P = common.adversarial_params(arch, "zero_bias")
    pl.x, pl.y = candidates(m, seed)
    shapes = O.param_shapes(arch)
    pl.g = {name: np.empty((m,) + tuple(shapes[name]), np.float64) for name in O.PARAM_NAMES}
    pl.parts = np.empty((m, 5), np.float64)
    for i in range(m):
        _, parts, g = O.loss_grad(arch, pl.P, pl.x[i:i + 1], pl.y[i:i + 1], lam=0.0, f64=True)
        pl.parts[i] = parts
        for name in O.PARAM_NAMES:
            pl.g[name][i] = g[name]
    _, parts, g = O.loss_grad(arch, pl.P, np.zeros((1, 33, 4, 4), np.float32), y0()[None], lam=0.0, f64=True)
    pl.g_empty, pl.parts_empty = g, np.array(parts)
    # the largest entry of every member's gradient, per tensor (margin())
    pl.gmax = {name: np.abs(pl.g[name]).reshape(m, -1).max(axis=1) for name in O.PARAM_NAMES}
    return pl


def members_for(count, seed, m=M):
    """`count` pool members for planted positions in ascending order: seeded permutations of the pool one after the
    other, so that neighbours differ and every member is used as often as any other (+-1)"""
    rng = np.random.RandomState(1000003 * (seed + 1))
    out = []
    while len(out) < count:
        perm = rng.permutation(m).tolist()
        if out and m > 1 and perm[0] == out[-1]:
            perm.append(perm.pop(0))
        out += perm
    return out[:count]


def batch(n, positions, members, device="cpu", m=M, seed=POOL_SEED):
    """-> (x [n,33,4,4], y [n,16]) torch fp32 on `device`: x all zeros and every label y0(), pool member members[k]
    (pileup and label) written at positions[k]"""
    import torch
    xs, ys = candidates(m, seed)
    positions = [int(p) for p in positions]
    assert len(positions) == len(members) and len(set(positions)) == len(positions)
    assert all(0 <= p < n for p in positions)
    x = torch.zeros((n, 33, 4, 4), dtype=torch.float32, device=device)
    y = torch.from_numpy(y0()).to(device)[None].repeat(n, 1).contiguous()
    if positions:
        idx = torch.tensor(positions, dtype=torch.int64, device=device)
        mem = np.asarray(members, dtype=np.int64)
        x[idx] = torch.from_numpy(np.ascontiguousarray(xs[mem])).to(device)
        y[idx] = torch.from_numpy(np.ascontiguousarray(ys[mem])).to(device)
    return x, y


def expected(pl, n, members):
    """-> (grads {name: float64}, parts [5] float64) of a batch of n candidates with `members` planted: kernels
    sum_k g[members[k]]; biases the same sum + (n - K) g_empty; loss parts the same sum + (n - K) EMPTY_PARTS"""
    cnt = np.bincount(np.asarray(members, dtype=np.int64), minlength=pl.m).astype(np.float64)
    K = len(members)
    grads = {}
    for name, g in pl.g.items():
        acc = np.zeros(g.shape[1:], np.float64)
        for i in np.flatnonzero(cnt):
            acc += cnt[i] * g[i]
        if name.endswith("bias"):
            acc += (n - K) * pl.g_empty[name]
        grads[name] = acc
    parts = cnt @ pl.parts + (n - K) * EMPTY_PARTS
    return grads, parts


def margin(arch, members, tol, abs_tol=1e-7):
    """Over the nine kernel tensors, the smallest ratio of (largest entry of the weakest planted member's gradient) to
    the distance a comparison allows, tol * (largest entry of the expected tensor) + abs_tol: how far the loss of ONE
    planted candidate stands above the rounding allowance."""
    pl = pool(arch)
    cnt = np.bincount(np.asarray(members, dtype=np.int64), minlength=pl.m).astype(np.float64)
    used = np.flatnonzero(cnt)
    worst = np.inf
    for name in KERNELS:
        g = pl.g[name]
        acc = np.zeros(g.shape[1:], np.float64)
        for i in used:
            acc += cnt[i] * g[i]
        worst = min(worst, float(pl.gmax[name][used].min()) / (tol * float(np.abs(acc).max()) + abs_tol))
    return worst


# ---- the cases of tests/test_gpu_planted.py (the margin of every one is asserted on the CPU, tests/test_planted_ref.py)

# the smallest ragged batch on the far side of each launch-shape line of the step: 2, 25, 49, 81, 129, 141, 161, 257, 401,
# 513, 1 025 and 2 049 groups of 16 candidates (16 387 and 32 771 are 1 025 and 2 049 groups with three candidates in
# the last one), and two slices of 32 784 + 32 753 candidates
SIZES = (17, 385, 769, 1281, 2049, 2241, 2561, 4097, 6401, 8193, 16387, 32771, 65537)
PLAIN_MAX = 2561               # option impl 0 (the one-thread-per-output kernels) up to here
PATHS = {"chain": {"train_ksplit": 0}, "default": {}, "plain": {"impl": 0}}


def ksplit_runs(arch, n, path):
    """whether this step's fc4 forward runs as eight k ranges: tests/test_gpu_train_parity.py, compare_step -- slim at
    every size, full up to 400 groups; never with option train_ksplit 0, nor on the plain kernels (a single chain)"""
    if path != "default":
        return False
    return arch == "slim" or (n + 15) // 16 <= 400


def kernel_tol(arch, n, path):
    """tests/test_gpu_train_parity.py's bound of a kernel gradient against the oracle, of the tensor's largest entry
    (+ 1e-7): 2e-5 as a single chain, 1e-4 where the k-split fc4 forward runs.  (Its sqrt(n / 10 000) growth belongs
    to sums over n candidates; a planted batch's kernel gradients are sums over the K planted ones.)"""
    return 1e-4 if ksplit_runs(arch, n, path) else 2e-5


def bias_tol(n):
    return 2e-5 * max(1.0, math.sqrt(n / 10000.0))


def single_positions(n):
    """Test 1: 0, 15, 16, 31; first and last candidate of the last full group; n - 1, n - 2; at 65 537 the candidates
    around the slice boundary and the lone candidate of the last group; then seeded positions until every one of the 16
    offsets inside a group occurs, at least 12 of them (the sizes are 16 k + 1 or 16 k + 3: the boundary positions hold
    three offsets at most, so up to 14 are drawn)."""
    full = n // 16
    pos = [0, 15, 16, 31, 16 * (full - 1), 16 * full - 1, n - 1, n - 2]
    if n == 65537:
        pos += [32783, 32784, 32785, 65536]
    pos = [p for p in dict.fromkeys(pos) if 0 <= p < n]
    rng = np.random.RandomState(n)
    G = (n + 15) // 16
    missing = [o for o in range(16) if o not in set(p % 16 for p in pos)]
    offs = missing + rng.randint(0, 16, size=max(0, 12 - len(missing))).tolist()
    for o in offs:
        for _ in range(1000):
            p = 16 * int(rng.randint(0, G)) + o
            if p < n and p not in pos:
                pos.append(p)
                break
    assert set(p % 16 for p in pos) == set(range(16))
    return pos


def single_members(arch, n, count):
    """Test 1: three pool members per size, dealt round robin, so that every member sits at several positions"""
    rng = np.random.RandomState(7 * n + (1 if arch == "slim" else 0))
    three = rng.choice(M, size=3, replace=False).tolist()
    return [three[k % 3] for k in range(count)]


# Test 2: how many candidates a run plants, per (topology, tolerance): the largest count (a multiple of 8) at which
# margin() is >= MARGIN_MIN for each member sequence the runs use (members_for seeds 0..2), from the oracle alone;
# tests/test_planted_ref.py asserts it for every run.  As a single chain the margin reaches 10 only near 1 600 (slim) and
# 2 000 (full) planted: capped at 1 024, where a run of the sizes below still leaves empty candidates between planted ones.
# Measured margins (weakest member's share over the allowed distance; the limit is a head kernel, YZygosityFC or
# YVarTypeFC, in every column):
#   planted   full 2e-5   slim 2e-5   full 1e-4   slim 1e-4
#       64       322 x       252 x        64 x        50 x
#      256        80 x        63 x        16 x        12.6 x
#      320        64 x        50 x        12.9 x      10.0 x
#      408        50 x        40 x        10.1 x       7.9 x
#    1 024        20 x        15.7 x        4.0 x       3.1 x
K_PLANTED = {
    ("full", 2e-5): 1024,
    ("slim", 2e-5): 1024,
    ("full", 1e-4): 408,
    ("slim", 1e-4): 320,
}
STRIDED_SIZES = (17, 385, 1281, 2561, 6401)


def strided_runs(arch, n, path):
    """Test 2: the positions 0..n-1 dealt into R = ceil(n / K) strided runs, run r = every p = r (mod R): together they
    plant at every position once, and each run touches every range.  -> [(positions, members)]"""
    K = K_PLANTED[(arch, kernel_tol(arch, n, path))]
    R = (n + K - 1) // K
    runs = []
    for r in range(R):
        pos = list(range(r, n, R))
        runs.append((pos, members_for(len(pos), seed=r % 3)))
    return runs


WINDOW_SIZES = (16387, 32771, 65537)


def windows(n):
    """Test 3: every position of the first 48, of the last 48 and, at 65 537, of the 64 around the slice boundary"""
    w = [("first48", list(range(48))), ("last48", list(range(n - 48, n)))]
    if n == 65537:
        w.append(("slice64", list(range(32784 - 32, 32784 + 32))))
    return [(name, pos, members_for(len(pos), seed=3 + k)) for k, (name, pos) in enumerate(w)]


# 225 = 15 groups: the convolution weight gradients launch 56 waves per output fragment and sum 49 tiles; 257 = 17 groups
# (added: the line `per = ceil(G / splits)` of the dense weight gradients -- slim's fc4 has 15 candidate ranges of two
# groups, the last six of them start past the last group); 65 537: the first layer launches 1 024 workgroups and sums 683
# tiles in the first slice
OWN_NOTHING_SIZES = (225, 257, 65537)


def group_plants(n):
    """Test 4: only the first group planted, then only the last one (a single candidate at these sizes)"""
    G = (n + 15) // 16
    out = []
    for k, (name, pos) in enumerate((("first_group", list(range(16))), ("last_group", list(range(16 * (G - 1), n))))):
        out.append((name, pos, members_for(len(pos), seed=10 + k)))
    return out
