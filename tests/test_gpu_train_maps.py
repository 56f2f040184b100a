"""The training step's maps against the ORACLE candidate by candidate (cv_get_activation 11..13 / 21..23 against
oracle.backward_maps, the per-candidate backward of cvo_loss_grad).

The weight gradients (tests/test_gpu_train_parity.py) are sums over the batch: a wrong value in one candidate's map
disappears in them.  Here each sampled candidate's maps are compared on their own, one step per case with the
reference's dropout rate and lambda, the oracle fed the device's keep mask (layer 6):
- pooled maps (11..13) bit for bit, signed zeros included: the training forward runs the canonical chain on every path;
- pre-activation gradients (21..23) within 1e-5 of the oracle's largest magnitude in that candidate's layer map (both
  sides fp32, in different summation orders through three data-gradient layers);
- where fc4's forward runs as eight k ranges (slim always, full up to 400 groups) within 5e-5: that order moves the
  dropout output by up to ~1e-5 of its size (6e-6 at slim n=83 candidate 68), and every head gradient and map with it
  (1.6e-5 there, 6e-7 with the single chain).  A candidate may exceed that only when a SELU pre-activation at or
  behind fc4 lies within the reordering's reach of 0 (|pre_j| <= 1e-5 * sum_k |in_k W_kj| in fc4, fc5 or a SELU
  head): selu' jumps between 1.051 and 1.758 there and the whole backward pass of the candidate with it.  At most one
  such candidate per 1 000 sampled.  (Full n=640 candidate 413: fc5 unit 121 at 5.2e-8, 2.5e-9 of its sum of
  magnitudes, lands below 0 on the device's k-range d4: the maps 11 % off, conv1/kernel 3e-4 in
  test_gpu_train_parity.py.)
Sizes cover every training kernel-set class and launch shape named in test_gpu_train_parity.py, and ragged last groups;
candidates: the first 64, every candidate of the last group, a seeded sample of up to 512 others.

Measured on the MI355X (worst per-candidate distance, relative to the candidate's largest entry in the layer): default
path full 9.9e-6 (k ranges; 1.0e-6 above 400 groups), slim 1.6e-5, and one explained exception in 3 923 sampled full
candidates (413 at n=640, above); train_ksplit 0: full 1.4e-6, slim 1.8e-6; impl 0: full 1.3e-6, slim 2.2e-6; full with
dbg4 = 4, layer 21 included: 1.2e-6; adversarial batches: at most 1.9e-6.  Pooled maps: the oracle's bits in every
case.  The whole file: 11 s.
"""
import numpy as np
import pytest

import common
from test_gpu_train_parity import _data, _model

pytestmark = pytest.mark.gpu

SIZES = (1, 17, 83, 320, 640, 1250, 2561, 6401, 10000, 40010)
BOUND = 1e-5          # per candidate and layer, of the oracle's largest magnitude in that map
BOUND_KSPLIT = 5e-5   # ... where fc4's forward runs as k ranges
NEAR_ZERO = 1e-5      # a SELU pre-activation this close to 0, relative to its sum of magnitudes, explains a selu' flip


def _cands(n, seed):
    """the first 64, the whole last group, up to 512 seeded others; sorted"""
    head = np.arange(min(n, 64))
    last = np.arange((n - 1) // 16 * 16, n)
    rest = np.setdiff1d(np.arange(n), np.union1d(head, last))
    pick = np.random.RandomState(seed).choice(rest, size=min(512, rest.size), replace=False) if rest.size else rest
    return np.unique(np.concatenate([head, last, pick])).astype(np.int64)


def _step(arch, P, x, y, options, rate, lam):
    m = _model(arch); m.setParameters(P)
    for k, v in (options or {}).items():
        m.setOption(k, v)
    m.dropoutRateFC4Val = rate; m.setL2RegularizationLambda(lam); m.setLearningRate(1e-3)
    m._dropout_seed = 4242
    m.train(x, y)
    return m


def _rows(m, layer, n, idx_dev):
    """layer of the last pass, only the sampled candidates leave the device (layer 23 at 40 010 is 0.8 GB)"""
    return m.getActivation(layer, n).index_select(0, idx_dev).cpu().numpy()


def _near_zero(P, ref, j):
    """(min |pre| / sum_k |in_k W_k|, layer) over the SELU units of fc4, fc5 and the three SELU heads of sampled
    candidate j, from the oracle's record (float64)"""
    best = (np.inf, None)
    for layer, inp, pre, w in (("fc4", "pool3", "fc4pre", "fc4/kernel"), ("fc5", "d4", "fc5pre", "fc5/kernel"),
                               ("zygosity", "fc5", "hpre1", "YZygosityFC/kernel"),
                               ("type", "fc5", "hpre2", "YVarTypeFC/kernel"),
                               ("length", "fc5", "hpre3", "YIndelLengthFC/kernel")):
        mag = np.abs(ref[inp][j].astype(np.float64).ravel()) @ np.abs(P[w].astype(np.float64))
        r = np.abs(ref[pre][j].astype(np.float64)) / np.maximum(mag, 1e-300)
        k = int(np.argmin(r))
        if r[k] < best[0]:
            best = (float(r[k]), "%s unit %d" % (layer, k))
    return best


def check_maps(oracle, arch, P, m, x, y, n, rate, what, seed=0, explain=False, grads=(1, 2, 3)):
    """Compare the sampled candidates' maps of model m's last training pass with the oracle.  grads: the gradient
    layers that must be there (the others must raise); explain: fc4 ran as k ranges (its bound and exception rule).  Returns
    (worst distance of the candidates within the bound, [(candidate, layer, distance, near-zero ratio)] exceptions, number
    of candidates sampled)."""
    import torch
    from clairvoyante_amd import _lib
    idx = _cands(n, seed)
    idx_dev = torch.from_numpy(idx).cuda()
    keep = (_rows(m, 6, n, idx_dev) != 0).astype(np.float32)
    ref = oracle.backward_maps(arch, P, x[idx], y[idx], mask4=keep, rate4=rate)
    for l in (1, 2, 3):
        got = _rows(m, 10 + l, n, idx_dev)
        same = common.same_bits(got, ref["pool%d" % l]).reshape(idx.size, -1).all(1)
        assert same.all(), "%s: pooled map %d differs from the oracle's bits for candidates %s" % (
            what, l, idx[~same][:8].tolist())
    worst, flagged = 0.0, {}
    for l in (1, 2, 3):
        if l not in grads:
            with pytest.raises(_lib.CvError):
                m.getActivation(20 + l, n)
            continue
        got = _rows(m, 20 + l, n, idx_dev)
        want = ref["gpre%d" % l]
        err = np.abs(got.astype(np.float64) - want).reshape(idx.size, -1).max(1)
        scale = np.abs(want.astype(np.float64)).reshape(idx.size, -1).max(1)
        assert np.isfinite(err).all(), (what, l)
        rel = err / np.maximum(scale, 1e-300)
        bad = err > (BOUND_KSPLIT if explain else BOUND) * scale
        for j in np.flatnonzero(bad):
            flagged.setdefault(int(j), []).append((l, float(rel[j])))
        if (~bad).any():
            worst = max(worst, float(rel[~bad].max()))
    exceptions = []
    for j, hits in sorted(flagged.items()):
        ratio, where = _near_zero(P, ref, j)
        for l, r in hits:
            line = "%s: candidate %d, layer %d: %.2e of its largest entry; nearest SELU pre-activation to 0: %s, %.2e" % (
                what, idx[j], 20 + l, r, where, ratio)
            print("EXCEPTION " + line)
            assert explain and ratio <= NEAR_ZERO, line
            exceptions.append((int(idx[j]), 20 + l, r, ratio))
    return worst, exceptions, idx.size


def _report(tag, results):
    """print the worst distance within the bound and the exceptions of a path; returns (exception candidates, sampled)"""
    worst = max(r[0] for r in results)
    sampled = sum(r[2] for r in results)
    cands = sum(len({e[0] for e in r[1]}) for r in results)
    print("train maps %s: worst %.2e over %d sampled candidates, %d explained exceptions %s" % (
        tag, worst, sampled, cands, ["cand %d L%d %.1e ratio %.1e" % e for r in results for e in r[1]]))
    return cands, sampled


@pytest.mark.parametrize("arch", ["full", "slim"])
@pytest.mark.parametrize("path", ["default", "train_ksplit0", "impl0"])
def test_training_maps_match_the_oracle_per_candidate(oracle, arch, path):
    """One step per size on the path; the default path carries the k-split bound and exception rule where fc4 runs as k ranges
    (counted over the whole path: at most one per 1 000 sampled candidates)"""
    from clairvoyante_amd import param
    rate, lam = param.dropoutRateFC4, param.l2RegularizationLambda
    P = common.bench_params(oracle, arch)
    options = {"default": {}, "train_ksplit0": {"train_ksplit": 0}, "impl0": {"impl": 0}}[path]
    results = []
    for n in SIZES:
        if path == "impl0" and n > 2561:
            continue
        x, y = _data(n, seed=9)
        m = _step(arch, P, x, y, options, rate, lam)
        ksplit = path == "default" and (arch == "slim" or (n + 15) // 16 <= 400)
        # the full topology's tile path fuses conv1's unpool into its weight gradient: layer 21 is never written
        grads = (2, 3) if (arch == "full" and path != "impl0") else (1, 2, 3)
        results.append(check_maps(oracle, arch, P, m, x, y, n, rate, "%s %s n=%d" % (arch, path, n), seed=n,
                                  explain=ksplit, grads=grads))
        m.close()
    cands, sampled = _report("%s %s" % (arch, path), results)
    assert cands <= max(1, sampled // 1000), (cands, sampled)


@pytest.mark.parametrize("n,options", [(83, {"dbg4": 4, "train_ksplit": 0}), (10000, {"dbg4": 4})])
def test_full_conv1_gradient_map_when_materialised(oracle, n, options):
    """dbg4 = 4 runs conv1's unpool as its own pass (the row-segment form at 83, the streaming one at 10 000):
    layer 21 is then written and held to the oracle with the others"""
    from clairvoyante_amd import param
    rate, lam = param.dropoutRateFC4, param.l2RegularizationLambda
    P = common.bench_params(oracle, "full")
    x, y = _data(n, seed=9)
    m = _step("full", P, x, y, options, rate, lam)
    r = check_maps(oracle, "full", P, m, x, y, n, rate, "full dbg4=4 n=%d" % n, seed=n)
    m.close()
    _report("full dbg4=4 n=%d" % n, [r])


@pytest.mark.parametrize("arch", ["full", "slim"])
@pytest.mark.parametrize("batch,weights", [("sparse", "init"), ("denormal", "init"), ("large", "zero_bias")])
def test_training_maps_on_adversarial_batches(oracle, arch, batch, weights):
    """common.adversarial_batch -- where the routing and -0 bugs were: zeroed ranges, -0.0, denormals, all-zero
    candidates (exact ties in pooling windows, pre-activations of +-0 and in (-2^-25, 0)), and large counts on zero
    biases.  Single-chain fc4 (train_ksplit 0) and the plain kernels (impl 0); the bit-exact and per-candidate rules
    with no exception."""
    from clairvoyante_amd import param
    rate, lam = param.dropoutRateFC4, param.l2RegularizationLambda
    P = common.adversarial_params(arch, weights)
    results = []
    for n in (37, 1250, 10000):
        x, y = common.adversarial_batch(n, batch, seed=11)
        for options in ({"train_ksplit": 0}, {"impl": 0}):
            m = _step(arch, P, x, y, options, rate, lam)
            grads = (2, 3) if (arch == "full" and "impl" not in options) else (1, 2, 3)
            results.append(check_maps(oracle, arch, P, m, x, y, n, rate, "%s %s/%s n=%d %s" % (
                arch, batch, weights, n, options), seed=n, grads=grads))
            m.close()
    _report("%s %s/%s" % (arch, batch, weights), results)


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_map_export_contract(oracle, arch):
    """Every layer code gives the oracle's values or an error: after getLoss the pooled maps are there and the
    gradients are not; n beyond the pass raises; after a step of several slices (70 001 candidates) 11..13 and 21..23
    raise with and without keep_activations, while 6 / 7 cover the whole batch with it; a single-slice step after that
    brings the maps back."""
    import torch
    from clairvoyante_amd import _lib, param
    rate, lam = param.dropoutRateFC4, param.l2RegularizationLambda
    P = common.bench_params(oracle, arch)
    maps = (11, 12, 13, 21, 22, 23)
    n = 83
    x, y = _data(n, seed=9)
    m = _model(arch); m.setParameters(P)
    m.getLoss(x, y)
    idx = np.arange(n); idx_dev = torch.from_numpy(idx).cuda()
    fa = oracle.forward_all(arch, P, x)
    for l in (1, 2, 3):
        assert common.same_bits(_rows(m, 10 + l, n, idx_dev), fa["pool%d" % l]).all(), l
        with pytest.raises(_lib.CvError):
            m.getActivation(20 + l, n)
    for layer in maps:
        with pytest.raises(_lib.CvError):
            m.getActivation(layer, n + 1)

    N = 70001
    xb, yb = _data(N, seed=21)
    m.dropoutRateFC4Val = rate; m.setL2RegularizationLambda(lam); m.setLearningRate(1e-3); m._dropout_seed = 4242
    for keep in (0, 1):
        m.setOption("keep_activations", keep)
        Pn = _params_now(m, oracle, arch)          # (the weights this step runs on)
        m.train(xb, yb)
        for layer in maps:
            for k in (1, N):
                with pytest.raises(_lib.CvError):
                    m.getActivation(layer, k)
    # keep_activations: the dropout maps of both slices; the rows at either end against the oracle's forward
    sel = np.concatenate([np.arange(32), np.arange(N - 32, N)])
    sel_dev = torch.from_numpy(sel).cuda()
    amask = _rows(m, 6, N, sel_dev)
    d4 = _rows(m, 7, N, sel_dev)
    fa = oracle.forward_all(arch, Pn, xb[sel], mask4=(amask != 0).astype(np.float32), rate4=rate)
    assert np.abs(d4 - fa["d4"]).max() <= 5e-6 * max(1.0, float(np.abs(fa["d4"]).max()))
    del amask, d4, fa

    # a single-slice step after the multi-slice one (fc4 as one chain): the maps are back and are the oracle's
    m.setOption("keep_activations", 0); m.setOption("train_ksplit", 0)
    n2 = 1250
    x2, y2 = _data(n2, seed=22)
    Pn = _params_now(m, oracle, arch)
    m.train(x2, y2)
    grads = (2, 3) if arch == "full" else (1, 2, 3)
    r = check_maps(oracle, arch, Pn, m, x2, y2, n2, rate, "%s after a multi-slice step" % arch, seed=n2, grads=grads)
    assert not r[1], r[1]
    for layer in maps:
        with pytest.raises(_lib.CvError):
            m.getActivation(layer, n2 + 1)
    m.close()


def _params_now(m, oracle, arch):
    """the model's current weights (after optimizer steps) as the oracle's parameter dict"""
    from test_gpu_train_parity import _flat, _split
    return {k: np.ascontiguousarray(v, dtype=np.float32)
            for k, v in _split(_flat(m, 0), oracle, m.paramShapes()).items()}
