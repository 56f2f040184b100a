"""The float64 formulation of tests/dropout5_ref.py (fc4 and fc5 alpha-dropout) at fc5 rate 0 against the oracle
(oracle/cv_oracle.c cvo_loss_grad), with and without a fc4 keep mask: the bounds tests/test_oracle.py holds the oracle
and tests/torch_ref.py to.  What makes it the reference of the fc5 dropout tests (tests/test_gpu_dropout5.py)."""
import numpy as np
import pytest
import torch

import common
import dropout5_ref


def _batch(n, seed=4):
    from clairvoyante_amd import synth
    xt, cls, rf, alt, il = synth.make_candidates(n, seed=seed, return_class=True)
    return xt.numpy(), synth.make_labels(cls, rf, alt, il).numpy()


@pytest.mark.parametrize("arch", ["full", "slim"])
@pytest.mark.parametrize("with_mask4", [False, True])
@pytest.mark.parametrize("mask5_ones", [False, True])
def test_rate0_formulation_matches_oracle(oracle, arch, with_mask4, mask5_ones):
    n, lam = 24, 1e-3
    x, y = _batch(n)
    P = common.bench_params(oracle, arch)
    mask4 = None
    if with_mask4:
        mask4 = (np.random.RandomState(0).uniform(size=(n, P["fc4/bias"].size)) < 0.5).astype(np.float32)
    # rate 0 with an all-keep mask is the identity (a = 1, b = 0): the same as no fc5 dropout
    mask5 = np.ones((n, P["fc5/bias"].size), np.float32) if mask5_ones else None
    loss, parts, grads = oracle.loss_grad(arch, P, x, y, lam=lam, mask4=mask4, rate4=0.5 if with_mask4 else 0.0)
    r = dropout5_ref.loss_grad(arch, P, x, y, lam, mask4=mask4, rate4=0.5 if with_mask4 else 0.0, mask5=mask5, rate5=0.0)
    assert abs(r["loss"] - loss) <= 1e-5 * abs(loss)
    for a, b in zip(parts, r["parts"]):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (a, b)
    assert set(grads) == set(r["grads"]) and len(grads) == 18
    for k, g in r["grads"].items():
        assert np.abs(grads[k] - g).max() <= 2e-4 * max(1e-6, np.abs(g).max()), k


def test_alpha_dropout_keeps_mean_and_variance():
    """selu.py:34-69: with the affine pair (a, b) a standard-normal input keeps mean 0 and variance 1"""
    rng = np.random.RandomState(1)
    h = torch.tensor(rng.standard_normal(400000))
    for rate in (0.1, 0.3, 0.5):
        keep = torch.tensor((rng.uniform(size=h.shape) >= rate).astype(np.float64))
        d = dropout5_ref.alpha_dropout(h, keep, rate)
        assert abs(float(d.mean())) < 0.01 and abs(float(d.var()) - 1.0) < 0.01, rate
