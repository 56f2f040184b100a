"""The planted-candidate construction (tests/planted_cases.py) on the CPU, with the oracle alone: an empty candidate is
silent in every kernel gradient, its losses are the closed form, a mixed batch is the sum expected() says -- and every
case tests/test_gpu_planted.py runs keeps the loss of ONE planted candidate at least ten times above the distance its
comparison allows, so that the device test cannot pass with a candidate lost, doubled or mispaired."""
import numpy as np
import pytest

import planted_cases as pc

ARCHS = ("full", "slim")


@pytest.mark.parametrize("arch", ARCHS)
def test_an_empty_candidate_is_silent_in_every_kernel_gradient(oracle, arch):
    pl = pc.pool(arch)
    for name in pc.KERNELS:
        assert not pl.g_empty[name].any(), name                      # exactly +-0
    for name in oracle.PARAM_NAMES:
        if name.endswith("bias"):
            assert np.abs(pl.g_empty[name]).max() > 0, name          # ... while every bias hears it
    for i in range(pl.m):                                            # and no pool member is silent anywhere
        assert all(pl.gmax[name][i] > 0 for name in pc.KERNELS), i


@pytest.mark.parametrize("arch", ARCHS)
def test_an_empty_candidates_losses_are_the_closed_form(oracle, arch):
    pl = pc.pool(arch)
    assert np.abs(pl.parts_empty - pc.EMPTY_PARTS).max() <= 1e-15, pl.parts_empty
    assert abs(pc.EMPTY_LOSS - 4.871201010907891) <= 1e-15
    # any one-hot label, and several empty candidates at once (the sum, in double)
    y = np.zeros((7, 16), np.float32)
    rng = np.random.RandomState(3)
    for i in range(7):
        y[i, [rng.randint(0, 4), 4 + rng.randint(0, 2), 6 + rng.randint(0, 4), 10 + rng.randint(0, 6)]] = 1.0
    _, parts, g = oracle.loss_grad(arch, pl.P, np.zeros((7, 33, 4, 4), np.float32), y, lam=0.0, f64=True)
    assert np.abs(np.array(parts) - 7 * pc.EMPTY_PARTS).max() <= 7e-15, parts
    assert not any(g[name].any() for name in pc.KERNELS)


@pytest.mark.parametrize("arch", ARCHS)
def test_a_mixed_batch_is_the_sum_of_its_planted_candidates(oracle, arch):
    pl = pc.pool(arch)
    n = 200
    pos = sorted(np.random.RandomState(8).choice(n, size=20, replace=False).tolist()) + [0, n - 1]
    pos = list(dict.fromkeys(pos))
    mem = pc.members_for(len(pos), seed=5)
    x, y = pc.batch(n, pos, mem)
    loss, parts, g = oracle.loss_grad(arch, pl.P, x.numpy(), y.numpy(), lam=0.0, f64=True)
    want, wparts = pc.expected(pl, n, mem)
    for name in oracle.PARAM_NAMES:
        assert np.abs(g[name] - want[name]).max() <= 1e-12 * np.abs(want[name]).max(), name
    assert np.abs(np.array(parts) - wparts).max() <= 1e-12 * np.abs(wparts).max()
    assert abs(loss - (pl.parts[mem].sum() + (n - len(pos)) * pc.EMPTY_LOSS)) <= 1e-12 * loss
    # the float gradients the device tests' neighbours compare with are these doubles, rounded
    _, _, g32 = oracle.loss_grad(arch, pl.P, x.numpy(), y.numpy(), lam=0.0)
    for name in oracle.PARAM_NAMES:
        assert np.array_equal(g32[name], g[name].astype(np.float32)), name


def test_batches_and_positions_are_what_the_cases_say():
    xs, ys = pc.candidates()
    x, y = pc.batch(50, [3, 49], [7, 9])
    x, y = x.numpy(), y.numpy()
    assert np.array_equal(x[3], xs[7]) and np.array_equal(x[49], xs[9]) and np.array_equal(y[49], ys[9])
    rest = np.ones(50, bool); rest[[3, 49]] = False
    assert not x[rest].any() and (y[rest] == pc.y0()).all()
    for n in pc.SIZES:
        pos = pc.single_positions(n)
        full = n // 16
        for p in (0, 15, 16, 16 * (full - 1), 16 * full - 1, n - 1, n - 2):
            assert p in pos, (n, p)
        assert n < 32 or 31 in pos
        assert len(pos) == len(set(pos)) and all(0 <= p < n for p in pos)
        assert set(p % 16 for p in pos) == set(range(16))
        assert len(pos) >= min(n, 12 + 7)                             # (17: every position there is)
        mem = pc.single_members("full", n, len(pos))
        assert min(mem.count(v) for v in set(mem)) >= 2              # position invariance has pairs to compare
    assert all(p in pc.single_positions(65537) for p in (32783, 32784, 32785, 65536))
    for n in pc.STRIDED_SIZES:
        for arch in ARCHS:
            for path in ("chain", "default"):
                runs = pc.strided_runs(arch, n, path)
                K = pc.K_PLANTED[(arch, pc.kernel_tol(arch, n, path))]
                assert sorted(p for pos, _ in runs for p in pos) == list(range(n))       # every position exactly once
                assert all(len(pos) <= K for pos, _ in runs)
                assert all(a != b for _, mem in runs for a, b in zip(mem, mem[1:]))     # neighbours differ
    assert [len(pos) for _, pos, _ in pc.windows(65537)] == [48, 48, 64]
    assert pc.windows(65537)[2][1][32] == 32784
    assert [pos for _, pos, _ in pc.group_plants(225)] == [list(range(16)), [224]]
    assert [pos for _, pos, _ in pc.group_plants(257)] == [list(range(16)), [256]]
    assert [pos for _, pos, _ in pc.group_plants(65537)] == [list(range(16)), [65536]]


@pytest.mark.parametrize("arch", ARCHS)
def test_every_device_case_keeps_one_candidate_ten_times_above_its_tolerance(oracle, arch):
    """margin() >= 10 for the members of every run of tests/test_gpu_planted.py under the tolerance that run is held to;
    and the counts of K_PLANTED are the largest that do (the next multiple of 8 fails, or the cap is reached)."""
    seen = {}

    def check(members, tol, what):
        key = (tuple(members), tol)
        if key not in seen:
            seen[key] = pc.margin(arch, members, tol)
        assert seen[key] >= pc.MARGIN_MIN, (what, tol, len(members), seen[key])
        return seen[key]

    for n in pc.SIZES:                                                           # test 1: one planted candidate
        for path in pc.PATHS:
            for mbr in set(pc.single_members(arch, n, 30)):
                check([mbr], pc.kernel_tol(arch, n, path), ("single", n, path))
    low = {}
    for n in pc.STRIDED_SIZES:                                                   # test 2
        for path in ("chain", "default"):
            tol = pc.kernel_tol(arch, n, path)
            for pos, mem in pc.strided_runs(arch, n, path):
                mg = check(mem, tol, ("strided", n, path))
                low[tol] = min(low.get(tol, np.inf), mg)
    for n in pc.WINDOW_SIZES:                                                    # test 3
        for path in ("chain", "default"):
            for name, pos, mem in pc.windows(n):
                check(mem, pc.kernel_tol(arch, n, path), (name, n, path))
    for n in pc.OWN_NOTHING_SIZES:                                               # test 4
        for path in ("chain", "default"):
            for name, pos, mem in pc.group_plants(n):
                check(mem, pc.kernel_tol(arch, n, path), (name, n, path))
    for tol in (2e-5, 1e-4):
        K = pc.K_PLANTED[(arch, tol)]
        mg = [pc.margin(arch, pc.members_for(K, seed), tol) for seed in range(3)]
        assert min(mg) >= pc.MARGIN_MIN, (tol, K, mg)
        over = [pc.margin(arch, pc.members_for(K + 8, seed), tol) for seed in range(3)]
        assert K == 1024 or min(over) < pc.MARGIN_MIN, (tol, K, over)
        print("planted margin %s tol %.0e: K = %d -> %.1f x (K + 8: %.1f x); lowest over the strided runs %.1f x"
              % (arch, tol, K, min(mg), min(over), low.get(tol, float("nan"))))
