"""front2_tm (conv1 + pool1 + conv2 + pool2 of the full topology) makes every first-layer row once per group: the two
waves of a group split the layer by width column and carry the pooling window's last four rows from chunk to chunk.
Tiny passes normally take the small-pass kernel set, so infer_small_groups 0 sends them through front2_tm here: whole
groups (infer_flat 0; 49 candidates leave a spare half workgroup) and flat ranges of 6 pooled rows (infer_flat 2: 26 = 4 x 6
+ 2, so ranges start mid-group and span two groups -- re-priming of the carried window, first rows above 0, partial last
chunks).  Outputs and the pool2 map must be the oracle's bits."""
import ctypes

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

N = 100


@pytest.fixture(scope="module")
def setup(oracle):
    from clairvoyante_amd import clairvoyante_v3
    P = common.bench_params(oracle, "full")
    m = clairvoyante_v3.Clairvoyante()
    m.setParameters(P)
    x = common.inputs(N)
    tail = x.copy()
    tail[:, 29:] = np.float32(-1000.0)       # the last windows' maxima then depend on which rows a window really holds
    cases = [(xi, oracle.forward_all("full", P, xi)) for xi in (x, tail)]
    yield m, cases
    m.close()


def _stage_kernel(m, stage):
    from clairvoyante_amd import _lib
    kn = ctypes.c_char_p()
    _lib.check(m._lib.cv_kernel_name(m._h, stage, ctypes.byref(kn)))
    return kn.value.decode() if kn.value else None


@pytest.mark.parametrize("flat", [0, 2])
@pytest.mark.parametrize("n", [1, 16, 17, 33, 49, 100])
def test_front2_rows_made_once_give_the_oracle_bits(setup, n, flat):
    import torch
    m, cases = setup
    try:
        m.setOption("impl", 1)
        m.setOption("variant", common.DEFAULT_VARIANT)
        m.setOption("keep_activations", 1)
        m.setOption("infer_small_groups", 0)
        m.setOption("infer_flat", flat)
        for x, ref in cases:
            got = m.predict_device(torch.from_numpy(x[:n]).cuda()).cpu().numpy()
            assert _stage_kernel(m, 1) == ("front2_tm<6, true>" if flat else "front2_tm<6, false>")
            want = np.ascontiguousarray(ref["out"][:n])
            assert got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            p2 = np.ascontiguousarray(m.getActivation(2, n).cpu().numpy().reshape(n, -1))
            w2 = np.ascontiguousarray(ref["pool2"][:n].reshape(n, -1), dtype=np.float32)
            assert p2.shape == w2.shape
            assert np.array_equal(p2.view(np.uint32), w2.view(np.uint32))
    finally:
        m.setOption("infer_small_groups", 256)
        m.setOption("infer_flat", 1)
        m.setOption("keep_activations", 0)
