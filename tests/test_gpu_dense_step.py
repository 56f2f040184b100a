"""GPU tests of the k step of the fused fc4 + fc5 + heads kernel (dense_tm<21, 8, 3, 2>; run with -m gpu on an MI355X).

The kernel carries the first weight fragments of a k step across the barrier in registers and stages its four-slot
ring three steps ahead.  The 288 steps of a pass wrap that ring 72 times whatever the pass holds, so a wrong slot, a
write into a slot that is still being read or a counted wait that leaves the wrong pieces in flight shows at the
smallest pass; the candidate counts walk the edges of the kernel's work split (16 candidates per group, two groups per
wave, eight waves per workgroup).  The fused form is forced at these sizes the way tests/test_gpu_layers.py forces it.
Every value is compared with the oracle as uint32: out16, the fc4 and fc5 maps, and the logits of cv_forward_logits
against cvo_selu_scalar(hpre) + float32(1e-10)."""
import ctypes

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

FUSED = {"infer_fc4_small_groups": 0, "infer_slab_groups": 0}
BACK = {"infer_fc4_small_groups": 288, "infer_slab_groups": -1}
KERNEL = "dense_tm<21, 8, 3, 2>"
# one group / a second group that is mostly padding rows; one wave's two groups / the next wave with a single real
# group; the last wave of a workgroup / a full workgroup / a second workgroup with one real candidate; 1 000
NS = (1, 16, 17, 32, 33, 241, 256, 257, 1000)


def _stage3(m):
    from clairvoyante_amd import _lib
    kn = ctypes.c_char_p()
    _lib.check(m._lib.cv_kernel_name(m._h, 3, ctypes.byref(kn)))
    return kn.value.decode() if kn.value else None


def _same(got, want, what):
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def _logits(oracle, ref):
    selu = np.vectorize(oracle.lib().cvo_selu_scalar, otypes=[np.float32])
    pre = np.concatenate([ref["hpre1"], ref["hpre2"], ref["hpre3"]], axis=1).astype(np.float32)
    lg = (selu(pre) + np.float32(1e-10)).astype(np.float32)
    return np.concatenate([ref["out"][:, :4], lg], axis=1)


@pytest.fixture(scope="module")
def world(oracle):
    """model with the fused form forced, 1 000 inputs, the oracle's intermediates and logits (computed once)"""
    from clairvoyante_amd import clairvoyante_v3
    P = common.bench_params(oracle, "full")
    x = common.inputs(976, stress=24)
    ref = oracle.forward_all("full", P, x)
    m = clairvoyante_v3.Clairvoyante()
    m.setParameters(P)
    for k, v in FUSED.items():
        m.setOption(k, v)
    yield m, P, x, ref, _logits(oracle, ref)
    for k, v in BACK.items():
        m.setOption(k, v)
    m.close()


@pytest.mark.parametrize("n", NS)
def test_outputs_and_fc_maps_equal_the_oracle(world, n):
    m, _P, x, ref, _lg = world
    got = m.layers(x[:n], ["fc4", "fc5", "YBaseChangeSigmoid", "YZygositySoftmax", "YVarTypeSoftmax", "YIndelLengthSoftmax"])
    assert _stage3(m) == KERNEL
    out16 = np.concatenate([got[k] for k in ("YBaseChangeSigmoid", "YZygositySoftmax", "YVarTypeSoftmax", "YIndelLengthSoftmax")], axis=1)
    _same(out16, ref["out"][:n], "out16 n=%d" % n)
    _same(got["fc4"], ref["fc4"][:n], "fc4 n=%d" % n)
    _same(got["fc5"], ref["fc5"][:n], "fc5 n=%d" % n)


@pytest.mark.parametrize("n", NS)
def test_outputs_without_kept_maps_equal_the_oracle(world, n):
    """the pass as predict runs it (keep_activations = 0: the first group's fc4 fragments never leave the registers)"""
    import torch
    m, _P, x, ref, _lg = world
    got = m.predict_device(torch.from_numpy(x[:n]).cuda()).cpu().numpy()
    assert _stage3(m) == KERNEL
    _same(got, ref["out"][:n], "out16 n=%d" % n)


@pytest.mark.parametrize("n", NS)
def test_logits_equal_the_oracle(world, n):
    import torch
    m, _P, x, _ref, lg = world
    got = m.embeddings_device(torch.from_numpy(x[:n]).cuda()).cpu().numpy()
    assert _stage3(m) == KERNEL[:-1] + ", true>"
    _same(got, lg[:n], "logits n=%d" % n)


def test_stress_pass_of_8192_equals_the_oracle(oracle, world):
    """32 workgroups, uniform integers in [-250, 250]: the worst magnitudes the layers see"""
    from clairvoyante_amd import synth
    m, P, _x, _ref, _lg = world
    x = np.ascontiguousarray(synth.make_stress(8192).numpy(), dtype=np.float32)
    ref = oracle.forward_all("full", P, x)
    got = m.layers(x, ["fc4", "fc5", "YBaseChangeSigmoid", "YZygositySoftmax", "YVarTypeSoftmax", "YIndelLengthSoftmax"])
    assert _stage3(m) == KERNEL
    out16 = np.concatenate([got[k] for k in ("YBaseChangeSigmoid", "YZygositySoftmax", "YVarTypeSoftmax", "YIndelLengthSoftmax")], axis=1)
    _same(out16, ref["out"], "out16 stress")
    _same(got["fc4"], ref["fc4"], "fc4 stress")
    _same(got["fc5"], ref["fc5"], "fc5 stress")
