"""The training step held to PLANTED candidates (tests/planted_cases.py): a batch of n empty candidates
with a few real ones at chosen positions, zero biases, no dropout, lambda 0, learning rate 0.  Every kernel gradient
must be that of the planted candidates alone, so the comparison is relative to THEIR gradient at any n -- a candidate
lost at a range boundary, counted twice across the slices, clamped away in a ragged group or multiplied with its
neighbour's gradient is an error of the order of the tensor, where the dense random batches of
tests/test_gpu_train_parity.py allow 2e-5 .. 1e-4 of a sum over n and one candidate carries 1/n of it.

The bounds are that file's: a kernel gradient within 2e-5 of the expected tensor's largest entry + 1e-7 as a single
chain, 1e-4 where the fc4 forward runs as eight k ranges (planted_cases.kernel_tol); bias gradients, which do sum over
all n candidates, within 2e-5 * max(1, sqrt(n / 10 000)); losses and getLoss within 1e-5.  tests/test_planted_ref.py
asserts on the CPU that in every case below the weakest planted candidate's gradient is at least ten times the allowed
distance.

Measured on an MI355X (worst over all cases of a test, distance over the expected tensor's largest entry): see DESIGN 4.7.
"""
import ctypes

import numpy as np
import pytest

import planted_cases as pc

pytestmark = pytest.mark.gpu

LOSS_KEYS = ("loss1", "loss2", "loss3", "loss4", "lossL2")
ARCHS = ("full", "slim")


def _model(arch, path):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    m = clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()
    m.setParameters(pc.pool(arch).P)
    for k, v in pc.PATHS[path].items():
        m.setOption(k, v)
    m.dropoutRateFC4Val = 0.0; m.dropoutRateFC5Val = 0.0
    m.setL2RegularizationLambda(0.0); m.setLearningRate(0.0)
    m._dropout_seed = 4242
    return m


def _flat(m, which):
    import torch
    from clairvoyante_amd import _lib
    t = torch.empty(m.numParameters, device="cuda")
    _lib.check(m._lib.cv_flat_copy(m._h, which, ctypes.c_void_p(t.data_ptr()), 0, None))
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _split(flat, oracle, shapes):
    out, off = {}, 0
    for name in oracle.PARAM_NAMES:
        sz = int(np.prod(shapes[name]))
        out[name] = flat[off:off + sz].reshape(shapes[name]); off += sz
    assert off == flat.size
    return out


class Case(object):
    """One model for all the steps of a case; check() runs one planted batch through getLoss and train and holds the
    result to expected(); done() asserts that the weights have not moved and reports the worst distances."""

    def __init__(self, oracle, arch, n, path):
        self.oracle, self.arch, self.n, self.path = oracle, arch, n, path
        self.pl = pc.pool(arch)
        self.m = _model(arch, path)
        self.shapes = self.m.paramShapes()
        self.tol = pc.kernel_tol(arch, n, path)
        self.worst = {}
        self.want = {}

    def _expected(self, members):
        key = tuple(members)
        if key not in self.want:
            if len(self.want) > 4:
                self.want.clear()
            self.want[key] = pc.expected(self.pl, self.n, members)
        return self.want[key]

    def _note(self, name, err):
        self.worst[name] = max(self.worst.get(name, 0.0), err)

    def check(self, positions, members, what, kernels_only=False):
        n, m = self.n, self.m
        x, y = pc.batch(n, positions, members, device="cuda")
        want, wparts = self._expected(members)
        wloss = float(wparts.sum())
        if not kernels_only:
            l_eval = float(m.getLoss(x, y))
            self._note("getLoss", abs(l_eval - wloss) / abs(wloss))
        loss, summ = m.train(x, y)
        g = _split(_flat(m, 1), self.oracle, self.shapes)
        ctx = (self.arch, n, self.path, what)
        for name in pc.KERNELS:                                                   # (a)
            d = float(np.abs(g[name] - want[name]).max()); big = float(np.abs(want[name]).max())
            self._note(name, d / big)
            assert d <= self.tol * big + 1e-7, ctx + (name, d / big)
        if kernels_only:
            return g
        for name in self.oracle.PARAM_NAMES:                                      # (b)
            if name.endswith("bias"):
                d = float(np.abs(g[name] - want[name]).max()); big = float(np.abs(want[name]).max())
                self._note(name, d / big)
                assert d <= pc.bias_tol(n) * big, ctx + (name, d / big)
        self._note("loss", abs(float(loss) - wloss) / abs(wloss))
        for k, ref in zip(LOSS_KEYS, wparts):
            self._note(k, abs(summ[k] - ref) / max(1.0, abs(ref)))
            assert self.worst[k] <= 1e-5, ctx + (k, summ[k], ref)
        assert self.worst["loss"] <= 1e-5, ctx + (float(loss), wloss)
        assert self.worst["getLoss"] <= 1e-5, ctx + (l_eval, wloss)
        return g

    def done(self, label):
        w = _flat(self.m, 0)
        P = np.concatenate([np.asarray(self.pl.P[name], np.float32).ravel() for name in self.oracle.PARAM_NAMES])
        assert np.array_equal(w, P), "the weights moved under learning rate 0"
        self.m.close()
        print("planted %s %s n=%d %s (tol %.0e): %s" % (label, self.arch, self.n, self.path, self.tol,
              " ".join("%s=%.1e" % (k.replace("/kernel", "/k").replace("/bias", "/b"), v) for k, v in self.worst.items())))


def _single_cases():
    for n in pc.SIZES:
        for path in ("chain", "default", "plain"):
            if path != "plain" or n <= pc.PLAIN_MAX:
                yield n, path


@pytest.mark.parametrize("n,path", list(_single_cases()))
@pytest.mark.parametrize("arch", ARCHS)
def test_one_planted_candidate_at_every_kind_of_position(oracle, arch, n, path):
    """Test 1.  One candidate planted at 0, 15, 16, 31, the ends of the last full group, n - 2, n - 1, both sides of the
    slice boundary (65 537) and seeded positions covering all 16 offsets of a group, each in a step of its own: (a)
    kernels, (b) biases and losses -- and (c) position invariance: the fc4, fc5 and head kernel gradients of the same
    pool member at any two positions of one size and option set are the same floats (+0 == -0): each element is one
    product plus zeros.  Convolution kernels sum over the rows of a candidate and are held to (a)."""
    c = Case(oracle, arch, n, path)
    positions = pc.single_positions(n)
    members = pc.single_members(arch, n, len(positions))
    first = {}
    moved = []
    for p, mbr in zip(positions, members):
        g = c.check([p], [mbr], "position %d member %d" % (p, mbr))
        if mbr not in first:
            first[mbr] = (p, {name: g[name].copy() for name in pc.ONE_PRODUCT})
            continue
        p0, g0 = first[mbr]
        for name in pc.ONE_PRODUCT:
            if not np.array_equal(g[name], g0[name]):
                moved.append((name, mbr, p0, p, float(np.abs(g[name] - g0[name]).max() / np.abs(g0[name]).max())))
    c.done("single")
    assert not moved, "a candidate's gradient depends on where it sits in the batch: %s" % (moved[:8],)


@pytest.mark.parametrize("path", ["chain", "default"])
@pytest.mark.parametrize("n", pc.STRIDED_SIZES)
@pytest.mark.parametrize("arch", ARCHS)
def test_every_position_is_counted_exactly_once(oracle, arch, n, path):
    """Test 2.  The positions 0..n-1 in R = ceil(n / K) strided runs (run r plants every p = r mod R): together they
    plant every position once, each run touches every range.  K = planted_cases.K_PLANTED: the largest count at which
    the weakest planted candidate stays ten times above the allowed distance."""
    c = Case(oracle, arch, n, path)
    for r, (pos, mem) in enumerate(pc.strided_runs(arch, n, path)):
        c.check(pos, mem, "run %d of stride" % r)
    c.done("strided")


@pytest.mark.parametrize("path", ["chain", "default"])
@pytest.mark.parametrize("n", pc.WINDOW_SIZES)
@pytest.mark.parametrize("arch", ARCHS)
def test_windows_at_the_large_sizes(oracle, arch, n, path):
    """Test 3.  1 025 and 2 049 groups and two slices: every position of the first 48, the last 48 and the 64 around the
    slice boundary planted, one step per window."""
    c = Case(oracle, arch, n, path)
    for name, pos, mem in pc.windows(n):
        c.check(pos, mem, name)
    c.done("windows")


@pytest.mark.parametrize("path", ["chain", "default"])
@pytest.mark.parametrize("n", pc.OWN_NOTHING_SIZES)
@pytest.mark.parametrize("arch", ARCHS)
def test_ranges_that_own_nothing_add_nothing(oracle, arch, n, path):
    """Test 4.  15 groups (fewer groups than candidate ranges: ranges past the last group) and two slices of 2 049 and
    2 048 groups (the first layer launches more workgroups than it sums tiles): only the first group planted, then only the
    last one -- the launched-but-unused ranges and tiles must contribute zero."""
    c = Case(oracle, arch, n, path)
    for name, pos, mem in pc.group_plants(n):
        c.check(pos, mem, name, kernels_only=True)
    c.done("own-nothing")
