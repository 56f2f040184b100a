"""GPU tests of the inspection entries (run with -m gpu on an MI355X): cv_forward_logits and cv_forward_conv_map through
the model object (embeddings / embeddings_device / layers) and the getEmbedding command line, against
oracle.forward_all -- bit for bit, like the rest of the forward pass.

Logits: columns 0..3 are the oracle's sigmoid, columns 4..15 cvo_selu_scalar(hpre) + float32(1e-10) taken elementwise
in float32.  Conv maps: the oracle's act1..act3 (SELU before pooling)."""
import ctypes
import os

import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_DEFAULTS = {"impl": 1, "variant": common.DEFAULT_VARIANT, "chunk": 65536, "infer_fc4_small_groups": 288,
                   "infer_slab_groups": -1, "slim_small_groups": -1, "slim_waves": 0}
# every kernel form that computes the heads, forced the way tests/test_gpu_parity.py forces forms:
# (topology, options, the stage that computes the heads, its kernel in a cv_forward pass)
FORMS = [
    ("full", {"impl": 0}, None, None),                                                               # heads_kernel<false>
    ("full", {"variant": 493}, 5, "heads_kernel"),                                                   # heads_kernel<true> behind the tile layers
    ("full", {"variant": 495}, 5, "heads_tm"),
    ("full", {}, 4, "infer_tail_tm<21, 11>"),
    ("full", {"variant": 2031 & ~128}, 4, "dense_tm<11, 4, 2, 1>"),
    ("full", {"infer_fc4_small_groups": 0, "infer_slab_groups": 0}, 3, "dense_tm<21, 8, 3, 2>"),
    ("slim", {"impl": 0}, None, None),
    ("slim", {"variant": 493}, 5, "heads_kernel"),
    ("slim", {"variant": 495}, 5, "heads_tm"),
    ("slim", {"slim_small_groups": 65536}, 4, "dense_tm<2, 4, 2, 1>"),
    ("slim", {"slim_small_groups": 0, "variant": 1007}, 4, "dense_tm<2, 4, 2, 1>"),
    ("slim", {"slim_small_groups": 0, "slim_waves": 8}, 2, "conv3fc4_slim<8>"),
    ("slim", {"slim_small_groups": 0, "slim_waves": 4}, 2, "conv3fc4_slim<4>"),
]
NS = (1, 15, 16, 17, 1000)


def _model(arch):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    return clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()


def _logits(oracle, ref):
    """[n,16]: the oracle's sigmoid, then selu(hpre) + 1e-10 of the three other heads, each step in float32"""
    selu = np.vectorize(oracle.lib().cvo_selu_scalar, otypes=[np.float32])
    pre = np.concatenate([ref["hpre1"], ref["hpre2"], ref["hpre3"]], axis=1).astype(np.float32)
    with np.errstate(invalid="ignore"):                    # (NaN pre-activations of the adversarial inputs stay NaN)
        lg = (selu(pre) + np.float32(1e-10)).astype(np.float32)
    return np.concatenate([ref["out"][:, :4], lg], axis=1)


@pytest.fixture(scope="module")
def world(oracle):
    """per topology: model, weights, 1 000 inputs, the oracle's intermediates and the logits from them (computed once)"""
    w = {}
    for arch in ("full", "slim"):
        P = common.bench_params(oracle, arch)
        m = _model(arch)
        m.setParameters(P)
        x = common.inputs(976, stress=24)
        ref = oracle.forward_all(arch, P, x)
        w[arch] = (m, P, x, ref, _logits(oracle, ref))
    yield w
    for m, *_ in w.values():
        m.close()


def _set(m, opts):
    for k, v in OPTION_DEFAULTS.items():
        m.setOption(k, opts.get(k, v))


def _names(m):
    from clairvoyante_amd import _lib
    out = []
    for s in range(6):
        kn = ctypes.c_char_p()
        _lib.check(m._lib.cv_kernel_name(m._h, s, ctypes.byref(kn)))
        out.append(kn.value.decode() if kn.value else None)
    return out


def _with_argument(name):
    """the kernel's name with the logits template argument"""
    return name[:-1] + ", true>" if name.endswith(">") else name + "<true>"


def _all_same(got, want, what):
    ok = common.same_bits(got, want)
    assert ok.all(), "%s: %d of %d values differ, first at %s" % (what, int((~ok).sum()), ok.size, np.argwhere(~ok)[0])


@pytest.mark.parametrize("form", range(len(FORMS)), ids=["%s-%s" % (f[0], f[3] or "impl0") + "-%d" % i for i, f in enumerate(FORMS)])
def test_logits_of_every_head_form_equal_the_oracle(world, form):
    import torch
    arch, opts, stage, kernel = FORMS[form]
    m, _P, x, _ref, want = world[arch]
    xd = torch.from_numpy(x).cuda()
    try:
        _set(m, opts)
        for n, chunk in [(n, 65536) for n in NS] + [(600, 256)]:
            m.setOption("chunk", chunk)
            soft = m.predict_device(xd[:n]).cpu().numpy()
            fwd = _names(m)
            got = m.embeddings_device(xd[:n]).cpu().numpy()
            lgn = _names(m)
            assert got.shape == (n, 16)
            _all_same(got, want[:n], "%s n=%d chunk=%d" % (kernel, n, chunk))
            _all_same(got[:, :4], soft[:, :4], "base sigmoid against cv_forward, n=%d" % n)
            if stage is None:
                assert fwd == lgn == [None] * 6               # the plain kernels report no names
                continue
            # the same form per stage; the one that computes the heads shows the new argument
            assert fwd[stage] == kernel, (n, fwd)
            assert lgn == [(_with_argument(k) if s == stage else k) for s, k in enumerate(fwd)], (n, fwd, lgn)
    finally:
        _set(m, {})


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_embeddings_of_a_host_batch_are_the_four_heads_side_by_side(world, arch):
    m, _P, x, _ref, want = world[arch]
    e = m.embeddings(x)
    assert [a.shape for a in e] == [(1000, 4), (1000, 2), (1000, 4), (1000, 6)]
    _all_same(np.concatenate(e, axis=1), want, "embeddings")
    assert [a.shape for a in m.embeddings(x[:0])] == [(0, 4), (0, 2), (0, 4), (0, 6)]


@pytest.mark.parametrize("impl", [1, 0])
@pytest.mark.parametrize("arch", ["full", "slim"])
def test_conv_maps_before_pooling_equal_the_oracle(world, arch, impl):
    import torch
    m, _P, x, ref, _lg = world[arch]
    try:
        _set(m, {"impl": impl})
        for n, chunk in ((1, 65536), (17, 65536), (600, 256)):
            m.setOption("chunk", chunk)
            got = m.layers(x[:n], ["conv1", "conv2", "conv3"])
            for l in (1, 2, 3):
                want = ref["act%d" % l][:n]
                assert got["conv%d" % l].shape == want.shape
                _all_same(got["conv%d" % l], want, "conv%d impl=%d n=%d" % (l, impl, n))
        if arch == "slim":            # no pooling: the maps are the pass's own (unfused layers, so that all three exist)
            _set(m, {"impl": impl, "variant": 1006 & ~256, "slim_small_groups": 0})
            got = m.layers(x[:600], ["conv1", "conv2", "conv3"])
            m.predict_device(torch.from_numpy(x[:600]).cuda())
            for l in (1, 2, 3):
                _all_same(got["conv%d" % l], m.getActivation(l, 600).cpu().numpy(), "slim conv%d against cv_get_activation" % l)
    finally:
        _set(m, {})


@pytest.mark.parametrize("layer", [0, 4])
def test_conv_map_of_a_layer_outside_1_to_3_is_an_error(world, layer):
    import torch
    from clairvoyante_amd import _lib
    m, _P, x, _ref, _lg = world["full"]
    xd = torch.from_numpy(x[:16]).cuda()
    dst = torch.empty((16, 33, 4, 48), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.CvError, match="not in 1..3"):
        _lib.check(m._lib.cv_forward_conv_map(m._h, ctypes.c_void_p(xd.data_ptr()), 16, layer,
                                              ctypes.c_void_p(dst.data_ptr()), None))


@pytest.mark.parametrize("kind", ["specials", "small", "large", "sparse", "denormal", "zero_bias"])
@pytest.mark.parametrize("arch", ["full", "slim"])
def test_adversarial_inputs_logits_and_maps(oracle, arch, kind):
    """NaN, +-Inf, -0.0, denormals, zero biases at n = 256: bitwise where finite, NaN where the oracle has NaN (same_bits)"""
    n = 256
    if kind == "specials":
        x = common.adversarial_inputs(n)
    elif kind == "zero_bias":
        x = common.adversarial_batch(n, "sparse")[0]
    else:
        x = common.adversarial_batch(n, kind)[0]
    P = common.adversarial_params(arch, "zero_bias" if kind == "zero_bias" else "bench")
    ref = oracle.forward_all(arch, P, x)
    want = _logits(oracle, ref)
    if kind == "specials":
        assert np.isnan(want).any() and np.isfinite(want).any()
    m = _model(arch)
    try:
        m.setParameters(P)
        for impl in (1, 0):
            m.setOption("impl", impl)
            _all_same(np.concatenate(m.embeddings(x), axis=1), want, "logits %s impl=%d" % (kind, impl))
            got = m.layers(x, ["conv1", "conv2", "conv3"])
            for l in (1, 2, 3):
                _all_same(got["conv%d" % l], ref["act%d" % l], "conv%d %s impl=%d" % (l, kind, impl))
    finally:
        m.close()


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_predict_and_a_training_step_are_not_disturbed(oracle, arch):
    from clairvoyante_amd import synth
    P = common.bench_params(oracle, arch)
    xt, cls, rf, alt, il = synth.make_candidates(300, seed=11, return_class=True)
    x = np.ascontiguousarray(xt.numpy(), dtype=np.float32)
    y = np.ascontiguousarray(synth.make_labels(cls, rf, alt, il).numpy(), dtype=np.float32)
    weights = []
    for touch in (False, True):
        m = _model(arch)
        try:
            m.setParameters(P)
            m._dropout_seed = 12345
            before = np.concatenate(m.predict(x), axis=1)
            if touch:
                m.embeddings(x)
                m.layers(x, ["conv2", "fc4", "embedding3"])
                after = np.concatenate(m.predict(x), axis=1)
                assert common.same_bits(before, after).all()
            m.train(x, y)
            weights.append(m.getParameters())
        finally:
            m.close()
    for name in weights[0]:
        assert common.same_bits(weights[0][name], weights[1][name]).all(), name


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_layers_names_shapes_and_values(world, arch):
    from clairvoyante_amd import _lib
    m, _P, x, ref, lg = world[arch]
    n = 40
    names = list(m.LAYER_NAMES)
    keep = ctypes.c_int64()
    _lib.check(m._lib.cv_get_option(m._h, b"keep_activations", ctypes.byref(keep)))
    got = m.layers(x[:n], names)
    assert list(got) == names
    a = m._arch
    hc = (33, 33 - (a.pool[0] - 1), 33 - (a.pool[0] - 1) - (a.pool[1] - 1))
    shapes = {"conv1": (n, hc[0], 4, a.cout[0]), "conv2": (n, hc[1], 4, a.cout[1]), "conv3": (n, hc[2], 4, a.cout[2]),
              "fc4": (n, a.fc4), "fc5": (n, a.fc5), "YBaseChangeSigmoid": (n, 4), "YZygositySoftmax": (n, 2),
              "YVarTypeSoftmax": (n, 4), "YIndelLengthSoftmax": (n, 6), "embedding1": (n, 4), "embedding2": (n, 2),
              "embedding3": (n, 4), "embedding4": (n, 6)}
    assert {k: v.shape for k, v in got.items()} == shapes
    for k, r in (("conv1", "act1"), ("conv2", "act2"), ("conv3", "act3"), ("fc4", "fc4"), ("fc5", "fc5")):
        _all_same(got[k], ref[r][:n].reshape(shapes[k]), k)
    outs = np.concatenate([got[k] for k in names[5:9]], axis=1)
    _all_same(outs, ref["out"][:n], "outputs")
    _all_same(np.concatenate([got[k] for k in names[9:]], axis=1), lg[:n], "embeddings")
    after = ctypes.c_int64()
    _lib.check(m._lib.cv_get_option(m._h, b"keep_activations", ctypes.byref(after)))
    assert after.value == keep.value == 0                       # the option is put back
    assert list(m.layers(x[:n], ["fc5"])) == ["fc5"]
    with pytest.raises(KeyError, match="conv4"):
        m.layers(x[:n], ["conv1", "conv4"])


def test_layers_fc_maps_span_several_chunks(world):
    m, _P, x, ref, _lg = world["full"]
    try:
        m.setOption("chunk", 256)
        got = m.layers(x[:600], ["fc4", "fc5"])
        _all_same(got["fc4"], ref["fc4"][:600], "fc4")
        _all_same(got["fc5"], ref["fc5"][:600], "fc5")
    finally:
        _set(m, {})


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_get_embedding_command_line_on_the_mini_set(oracle, arch, tmp_path, monkeypatch):
    from clairvoyante_amd import getEmbedding, tf_checkpoint, utils_v2
    P = common.adversarial_params(arch, "init", seed=3)
    m = _model(arch)
    try:
        m.setParameters(P)
        ck = str(tmp_path / "model")
        m.saveParameters(ck)
        binfn = os.path.join(ROOT, "tests", "golden", "mini.bin")
        total, XC, _YC, _posC = utils_v2.LoadBin(binfn)
        count = min(50, total)
        olog = str(tmp_path / "olog")
        monkeypatch.setattr("sys.argv", ["getEmbedding.py", "--bin_fn", binfn, "--chkpnt_fn", ck, "--olog_dir", olog,
                                         "--count", str(count)] + (["--slim"] if arch == "slim" else []))
        getEmbedding.main()
        got = tf_checkpoint.read_bundle(os.path.join(olog, "model.ckpt-1"))
        assert sorted(got) == sorted(getEmbedding.VARIABLES)
        X, _n, _e = utils_v2.DecompressArray(XC, 0, count, total)
        emb = m.embeddings(X)
        want = _logits(oracle, oracle.forward_all(arch, P, X))
        for name, e, (lo, hi) in zip(getEmbedding.VARIABLES, emb, common.HEADS):
            assert got[name].dtype == np.float32 and got[name].shape == (count, hi - lo)
            _all_same(got[name], e, name + " against m.embeddings")
            _all_same(got[name], want[:, lo:hi], name + " against the oracle")
    finally:
        m.close()
