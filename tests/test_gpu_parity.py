"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI,
against the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): argmax-exact on all four heads, |dp| <= 1e-4 on the
probabilities.  The kernels reproduce the oracle's canonical fmaf order, so the tests
assert a much tighter 2e-6 and report the bitwise-equal fraction.
"""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

TOL = 2e-6


def _model(arch):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    return clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()


@pytest.fixture(scope="module", params=["full", "slim"])
def setup(request, oracle):
    arch = request.param
    P = common.bench_params(oracle, arch)
    m = _model(arch)
    m.setParameters(P)
    m.setOption("keep_activations", 1)       # the tests below read the fc4 / fc5 maps also behind the fused tails
    x = common.inputs(1000, stress=24)
    ref = oracle.forward_all(arch, P, x)
    yield arch, P, m, x, ref
    m.close()


@pytest.mark.parametrize("impl", [1, 0])
def test_outputs_match_oracle(setup, impl):
    arch, P, m, x, ref = setup
    m.setOption("impl", impl)
    base, z, t, l = m.predict(x)
    got = np.concatenate([base, z, t, l], axis=1)
    assert got.shape == ref["out"].shape
    assert np.isfinite(got).all()
    assert np.abs(got - ref["out"]).max() <= TOL
    assert common.argmax_match(got, ref["out"]) == [1.0, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("impl,variant", [(1, 1007), (1, 1006), (1, 495), (1, 239), (1, 111), (1, 47), (1, 6), (1, 0), (0, 47)])
def test_intermediates_match_oracle(setup, impl, variant):
    import torch
    arch, P, m, x, ref = setup
    m.setOption("impl", impl)
    m.setOption("variant", variant)
    n = x.shape[0]
    m.predict_device(torch.from_numpy(x).cuda())
    m.setOption("variant", common.DEFAULT_VARIANT)
    for layer, name in ((1, "pool1"), (2, "pool2"), (3, "pool3"), (4, "fc4"), (5, "fc5")):
        if layer == 1 and impl == 1 and (variant & 1):
            continue      # with the first layer fused into the conv2 kernel pool1 never reaches HBM (round 6: also in the
                          # small passes of the full topology, where conv2's position parts make their own first-layer rows;
                          # variant 1006 = the small-pass set with the first layer as its own kernel)
        if layer == 3 and impl == 1 and (variant & 256) and arch == "slim":
            continue      # slim conv3 + fc4 as one kernel: the conv3 map never exists in memory
        a = m.getActivation(layer, n).cpu().numpy().reshape(n, -1)
        b = ref[name].reshape(n, -1)
        scale = max(1.0, float(np.abs(b).max()))
        assert np.abs(a - b).max() <= 1e-5 * scale, name


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33, 1000])
def test_ragged_batch_sizes(setup, n):
    arch, P, m, x, ref = setup
    m.setOption("impl", 1)
    base, z, t, l = m.predict(x[:n])
    assert base.shape == (n, 4) and z.shape == (n, 2) and t.shape == (n, 4) and l.shape == (n, 6)
    if n:
        got = np.concatenate([base, z, t, l], axis=1)
        assert np.abs(got - ref["out"][:n]).max() <= TOL


def test_chunking_is_invisible(setup):
    """results do not depend on the internal pass size"""
    arch, P, m, x, ref = setup
    m.setOption("impl", 1)
    m.setOption("chunk", 256)
    a = np.concatenate(m.predict(x), axis=1)
    m.setOption("chunk", 32768)
    b = np.concatenate(m.predict(x), axis=1)
    assert np.array_equal(a, b)


def test_plain_and_tile_kernels_agree_bitwise(setup):
    arch, P, m, x, ref = setup
    m.setOption("impl", 0)
    a = np.concatenate(m.predict(x), axis=1)
    m.setOption("impl", 1)
    for variant in (0, 1, 2, 4, 7, 8, 15, 47, 111, 65, 239, 128, 495, 256, 1007, 512, 879, 1519, 2031):       # every kernel variant computes the same bits
        m.setOption("variant", variant)
        b = np.concatenate(m.predict(x), axis=1)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), variant
    m.setOption("variant", common.DEFAULT_VARIANT)
    assert np.array_equal(a.view(np.uint32), ref["out"].view(np.uint32))     # ... the oracle's bits


def test_large_pass_kernels_equal_small_pass_kernels(setup):
    """A pass of more than 3 400 groups runs fc4 with all 21 output tiles per workgroup, smaller passes in
    three output slabs: both must give the same bits (the small-pass bits are the oracle's, see above)."""
    import torch
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    n = 60010                                # 3 751 groups: odd, so one wave of the two-groups-per-wave fc4 is half empty
    xd = synth.make_candidates(n, seed=77, device="cuda")
    m.setOption("impl", 1)
    m.setOption("chunk", 8192)
    small = m.predict_device(xd).cpu().numpy()
    for variant in (1519, 2031, 1007, 495, 239, 111, 47, 15, 11):        # fc5 + heads on fc4's tail / two groups per wave / one group per wave with 8 or 4 waves per workgroup
        m.setOption("variant", variant)
        m.setOption("chunk", 65536)
        big = m.predict_device(xd).cpu().numpy()
        assert np.array_equal(small.view(np.uint32), big.view(np.uint32)), variant
        if arch == "full" and variant in (1519, 495):      # fc4 / fc5 maps of the whole pass: written by the fused tail or by their own kernels
            acts = [m.getActivation(layer, n).cpu().numpy() for layer in (4, 5)]
            if variant == 1519:
                tail_acts = acts
            else:
                assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(tail_acts, acts))
    m.setOption("variant", common.DEFAULT_VARIANT)
    m.setOption("chunk", 65536)
    head = m.predict(xd[:256].cpu().numpy())
    assert np.array_equal(np.concatenate(head, axis=1), small[:256])


def test_passes_either_side_of_every_size_line_give_the_same_bits(setup):
    """cv_forward picks its kernels by the number of groups of the pass (options infer_small_groups 256,
    infer_fc4_small_groups 288, infer_slab_groups 3 400): a pass one group either side of each line must give the bits of
    the same candidates run in chunks of 2 048 (128 groups: the small-pass kernels throughout, the oracle's bits)"""
    import torch
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("variant", common.DEFAULT_VARIANT)
    xd = synth.make_candidates(54417, seed=79, device="cuda")
    m.setOption("chunk", 2048)
    want = m.predict_device(xd).cpu().numpy()
    m.setOption("chunk", 65536)
    # (round 6: up to 80 groups fc4 runs as one wave per (group, output fragment) -- option infer_fc4_one_groups; the position
    # parts of the small-pass convolutions are 8 / 4 / 2 by the number of groups; slim: the small-pass set by estimate)
    for n in (1, 17, 100, 250, 770, 1000, 1280, 1297, 1600, 2560, 2577, 4096, 4113, 4608, 4625, 8960, 8977, 32768, 32785, 54400, 54417):
        got = m.predict_device(xd[:n].contiguous()).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), n
    for key, value in (("infer_small_groups", 160), ("infer_fc4_small_groups", 256), ("infer_slab_groups", 2048)):
        m.setOption(key, value)                  # the lines of rounds 1-4
    for n in (2577, 4113, 32785):
        got = m.predict_device(xd[:n].contiguous()).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), n
    for key, value in (("infer_small_groups", 256), ("infer_fc4_small_groups", 288), ("infer_slab_groups", -1)):
        m.setOption(key, value)


LADDER = (1000, 1600, 2000, 2560, 2576, 3200, 4096, 4112, 5120, 6400, 8192, 10000, 12288, 16384, 24576, 32768, 32784,
          40000, 49152, 54417)


def test_every_size_of_the_ladder_gives_the_bits_of_small_chunks(setup):
    """Round 6: the launch shape of every per-group kernel is a function of the pass size (ragged fc4 slabs, flat
    (group, row) ranges of the convolutions, 4- or 8-wave slim workgroups, the fused tail by estimate).  Every size of
    the size-sweep ladder (tools/gpu_infer_stage_ladder.py) must give, bit for bit, what the same candidates give in
    chunks of 2 048 (the small-pass kernels throughout = the oracle's bits, tests above)."""
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("variant", common.DEFAULT_VARIANT)
    xd = synth.make_candidates(54417, seed=79, device="cuda")
    m.setOption("chunk", 2048)
    want = m.predict_device(xd).cpu().numpy()
    m.setOption("chunk", 65536)
    for n in LADDER:
        got = m.predict_device(xd[:n].contiguous()).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), n


def test_random_pass_sizes_give_the_bits_of_small_chunks(setup):
    """Round 6 made every launch shape a function of the pass size (position parts, flat ranges, ragged slabs, kernel forms
    and the slim kernel set by estimate): 64 seeded sizes, log-uniform over 1 .. 70 000 candidates -- ragged last groups,
    sizes next to nothing in particular -- must each give, bit for bit, what the same candidates give in chunks of 2 048
    (the small-pass kernels throughout = the oracle's bits, tests above), and a second call of the same size the same."""
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("variant", common.DEFAULT_VARIANT)
    rng = np.random.RandomState(20260)
    sizes = sorted(set(int(v) for v in np.exp(rng.uniform(0.0, np.log(70000.0), 64)).astype(np.int64)) | {1, 70000})
    xd = synth.make_candidates(70000, seed=91, device="cuda")
    m.setOption("chunk", 2048)
    want = m.predict_device(xd).cpu().numpy()
    m.setOption("chunk", 65536)
    for n in sizes:
        got = m.predict_device(xd[:n].contiguous()).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32)), n
        again = m.predict_device(xd[:n].contiguous()).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), n


@pytest.mark.parametrize("n", [4107, 12283, 32779])
def test_forced_launch_shapes_give_the_same_bits(setup, n):
    """the shapes the estimates choose between, each forced at sizes where it is NOT the default (ragged last group):
    every fc4 slab shape s = 4 .. 14 and the round-5 slab kernel (option dense_rag), whole groups / flat ranges for the
    convolutions (infer_flat 0 / 2), 4- / 8-wave slim workgroups (slim_waves), the slim topology's small-pass kernel set at
    every size / never (slim_small_groups), the slab form / the fused tail by a fixed line (infer_slab_groups)"""
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("variant", common.DEFAULT_VARIANT); m.setOption("chunk", 65536)
    xd = synth.make_candidates(n, seed=83, device="cuda")
    want = m.predict_device(xd).cpu().numpy()
    settings, defaults = common.FORCED_LAUNCH_SETTINGS, common.FORCED_LAUNCH_DEFAULTS
    try:
        for st in settings:
            for k, v in defaults.items():
                m.setOption(k, v)
            for k, v in st.items():
                m.setOption(k, v)
            got = m.predict_device(xd).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), st
    finally:
        for k, v in defaults.items():
            m.setOption(k, v)


@pytest.mark.parametrize("n", [100, 777, 1000, 1530, 4000])
def test_small_pass_shapes_give_the_same_bits(setup, n):
    """the small-pass kernel sets (round 6), each choice forced the other way at sizes either side of its line: the first
    layer inside conv2's position parts or as its own kernel (dbg0 6 / 5; default: fused up to 96 groups), fc4 as one wave
    per (group, fragment) or per (group, slab of 3) (infer_fc4_one_groups; default up to 80 groups; from 49 groups two groups
    per wave, dbg1 4: one), the slim topology's
    unfused set or its fused pair (slim_small_groups) -- same bits as the default"""
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("variant", common.DEFAULT_VARIANT); m.setOption("chunk", 65536)
    xd = synth.make_candidates(n, seed=89, device="cuda")
    want = m.predict_device(xd).cpu().numpy()
    defaults = common.SMALL_PASS_DEFAULTS
    try:
        for st in common.SMALL_PASS_SETTINGS:
            for k, v in defaults.items():
                m.setOption(k, v)
            for k, v in st.items():
                m.setOption(k, v)
            got = m.predict_device(xd).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), st
    finally:
        for k, v in defaults.items():
            m.setOption(k, v)


@pytest.mark.parametrize("n", [24576, 40003, 70001, 140000])
def test_predict_of_a_large_host_batch_in_overlapped_parts_gives_the_same_bits(setup, n):
    """predict(numpy) sends batches of >= 24 576 candidates to the device in parts (copy of part k + 1 under the kernels of
    part k, outputs back per part: model._predict_host_parts); the four arrays must be what one pass over the
    device-resident batch gives, bit for bit -- also when called twice in a row and from a worker thread (predictNoRT,
    callVar.py:197-204)"""
    import threading
    import torch
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("variant", common.DEFAULT_VARIANT); m.setOption("chunk", 65536)
    xd = synth.make_candidates(n, seed=91, device="cuda")
    want = m.predict_device(xd).cpu().numpy()
    xh = xd.cpu().numpy()
    for _ in range(2):
        got = np.concatenate(m.predict(xh), axis=1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    t = threading.Thread(target=m.predictNoRT, args=(xh,))
    t.start(); t.join()
    got = np.concatenate([m.predictBaseRTVal, m.predictZygosityRTVal, m.predictVarTypeRTVal, m.predictIndelLengthRTVal], axis=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not xh.flags.writeable or np.array_equal(xh, xd.cpu().numpy())       # the caller's array is never written


def test_fused_tail_back_to_back_calls_with_changing_outputs(setup):
    """fc5 + heads ride on the tail of the large-pass fc4 kernel (variant bit 10) and take the number of candidates and the
    output pointer per call: several large passes enqueued back to back, each with its own output tensor and size, no
    synchronisation in between -- every one must equal the separate-kernel result"""
    import torch
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("chunk", 65536)
    sizes = (60010, 55000, 65536, 60010)
    xs = [synth.make_candidates(n, seed=90 + i, device="cuda") for i, n in enumerate(sizes)]
    m.setOption("variant", 495)
    want = [m.predict_device(xd).cpu().numpy() for xd in xs]
    m.setOption("variant", common.DEFAULT_VARIANT)
    outs = [torch.full((n, 16), -1.0, device="cuda") for n in sizes]
    for xd, o in zip(xs, outs):
        m.predict_device(xd, o)
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert np.array_equal(o.cpu().numpy().view(np.uint32), w.view(np.uint32))


def test_candidates_are_independent_at_scale(setup):
    """size-independent property on 300 000 candidates: a candidate's 16 outputs do not depend on which other candidates
    share its pass, group of 16 or lane -- predicting a permuted batch gives the permuted outputs, bit for bit; and the
    softmax heads sum to 1"""
    import torch
    from clairvoyante_amd import synth
    arch, P, m, x, ref = setup
    m.setOption("impl", 1); m.setOption("variant", common.DEFAULT_VARIANT); m.setOption("chunk", 65536)
    n = 300000
    xd = synth.make_candidates(n, seed=123, device="cuda")
    out = m.predict_device(xd)
    perm = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    outp = m.predict_device(xd[perm].contiguous())
    assert torch.equal(outp, out[perm])
    o = out.cpu().numpy()
    assert np.isfinite(o).all() and (o >= 0).all() and (o <= 1).all()
    for lo, hi in ((4, 6), (6, 10), (10, 16)):
        assert np.abs(o[:, lo:hi].sum(axis=1) - 1).max() <= 2e-6


@pytest.mark.gpu
def test_device_selu_sweep_equals_the_oracle_sweep_and_is_monotone(oracle):
    """all 2 139 095 041 negative floats through the shipped binary's SELU: no monotonicity violation, and the same
    checksum of output bits as the oracle's sweep (i.e. device and oracle SELU agree on EVERY negative input)"""
    import ctypes
    from clairvoyante_amd import _lib
    lib = _lib.load()
    viol = ctypes.c_uint64(); chk = ctypes.c_uint64()
    _lib.check(lib.cv_selu_sweep(0, 0x80000000, 0xff800000, ctypes.byref(viol), ctypes.byref(chk)))
    o_viol, o_chk = oracle.selu_sweep()
    assert viol.value == 0 and o_viol == 0
    assert chk.value == o_chk
    # a small window too (different split of the range into runs)
    _lib.check(lib.cv_selu_sweep(0, 0xbe000000, 0xbe100000, ctypes.byref(viol), ctypes.byref(chk)))
    assert (viol.value, chk.value) == oracle.selu_sweep(0xbe000000, 0xbe100000)


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_hip_path_matches_committed_float64_fixture_directly(oracle, arch):
    """The independent check without the C oracle in the loop: the HIP path on tests/golden/forward_*.npz (inputs x,
    seeded weights) against the committed float64 outputs of the torch formulation (tests/golden/make_golden_forward.py;
    clairvoyante_v3.py:54-138): 16 outputs <= 1e-5 (north_star bar 1e-4), argmax-exact wherever the float64 margin
    exceeds 1e-5, pool3 and fc5 intermediates <= 2e-5 relative.  `oracle` only supplies the weight initialiser."""
    import os
    import torch
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_%s.npz" % arch))
    P = common.bench_params(oracle, arch, seed=int(d["seed"]))
    m = _model(arch)
    try:
        m.setParameters(P)
        m.setOption("keep_activations", 1)
        x = d["x"].astype(np.float32)
        n = x.shape[0]
        for variant in (common.DEFAULT_VARIANT, 0):       # pass-size default kernels, and the unfused set that keeps pool3
            m.setOption("variant", variant)
            got = m.predict_device(torch.from_numpy(x).cuda()).cpu().numpy()
            out64 = d["out64"]
            assert np.abs(got.astype(np.float64) - out64).max() <= 1e-5
            for lo, hi in common.HEADS:
                srt = np.sort(out64[:, lo:hi], 1)
                clear = (srt[:, -1] - srt[:, -2]) > 1e-5
                assert np.array_equal(np.argmax(got[clear, lo:hi], 1), np.argmax(out64[clear, lo:hi], 1))
            fc5 = m.getActivation(5, n).cpu().numpy()
            assert np.abs(fc5 - d["fc5_64"]).max() <= 2e-5 * max(1.0, np.abs(d["fc5_64"]).max())
        k = d["pool3_64"].shape[0]
        pool3 = m.getActivation(3, n).cpu().numpy()[:k]          # variant 0: conv3's map is in HBM for both topologies
        assert np.abs(pool3 - d["pool3_64"]).max() <= 2e-5 * np.abs(d["pool3_64"]).max()
    finally:
        m.close()


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_fused_tail_writes_no_maps_unless_asked(oracle, arch):
    """with fc5 and the heads on the tail of the fc4 kernel the fc4 / fc5 maps have no reader but cv_get_activation: by
    default they are not written (option keep_activations 0) and asking for them says so; the 16 outputs are the same
    bits either way"""
    import torch
    from clairvoyante_amd import _lib, synth
    n = 60010
    xd = synth.make_candidates(n, seed=78, device="cuda")
    m = _model(arch); m.setParameters(common.bench_params(oracle, arch))
    try:
        lean = m.predict_device(xd).cpu().numpy()
        with pytest.raises(_lib.CvError, match="keep_activations"):
            m.getActivation(5, n)
        m.getActivation(2, n)                                     # maps of the layers in front are untouched by the option
        m.setOption("keep_activations", 1)
        kept = m.predict_device(xd).cpu().numpy()
        assert np.array_equal(lean.view(np.uint32), kept.view(np.uint32))
        fc5 = m.getActivation(5, n).cpu().numpy()
        want = oracle.forward_all(arch, common.bench_params(oracle, arch), xd[:512].cpu().numpy())
        assert np.array_equal(fc5[:512].view(np.uint32), want["fc5"].view(np.uint32))
        assert np.array_equal(lean[:512].view(np.uint32), want["out"].view(np.uint32))
        small = m.predict_device(xd[:1000].contiguous())           # a pass on separate kernels always leaves its maps
        m.setOption("keep_activations", 0)
        small = m.predict_device(xd[:1000].contiguous())
        if arch == "full":
            m.getActivation(4, 1000)
    finally:
        m.close()


@pytest.mark.parametrize("flat_heads", [False, True])
@pytest.mark.parametrize("arch", ["full", "slim"])
def test_argmax_agrees_with_a_second_fp32_library_outside_the_float64_margin_set(oracle, arch, flat_heads):
    """north_star asks for 100 % per-head argmax agreement with TF-CPU; TensorFlow cannot run here, and its Eigen
    summation order is not the oracle's ascending-k chain anyway.  What can be shown: the float64 formulation bounds the
    set of candidates on which two correct fp32 implementations may order the two best classes differently (top-2
    margin < 1e-5 on a head), and OUTSIDE that set the HIP path agrees per head with float64 and with stock torch CPU
    ops (oneDNN: another library's summation order) on every candidate -- also with head weights shrunk until a large
    part of the candidates IS inside the set (flat_heads), where the two fp32 orders do differ.  bench.py reports the
    same quantities over its 262 144 timed candidates (parity.margin_below_1e-5_frac, cpu_baseline_torch.*)."""
    import torch
    import bench
    import torch_ref
    P = dict(common.bench_params(oracle, arch))
    if flat_heads:
        for k in list(P):                                   # logits within ~1e-5 of each other: most candidates near a tie
            if k.startswith("Y"):
                P[k] = (P[k] * np.float32(3e-5 if k.endswith("kernel") else 0.0)).astype(np.float32)
    x = common.inputs(8192, seed=11, stress=2048)
    m = _model(arch)
    try:
        m.setParameters(P)
        got = m.predict_device(torch.from_numpy(x).cuda()).cpu().numpy()
    finally:
        m.close()
    with torch.no_grad():
        other = torch_ref.forward(arch, P, x, dtype=torch.float32)["out"].numpy()
    s = bench.order_sensitivity(got, bench.float64_outputs(arch, P, x, None, chunk=4096)[:len(x)], other)
    assert s["n"] == len(x) and s["max_abs_dprob_vs_float64"] <= 1e-5
    assert s["argmax_match_vs_float64_where_margin_ge_1e-5"] == [1.0, 1.0, 1.0, 1.0]
    assert s["other_argmax_match_where_margin_ge_1e-5"] == [1.0, 1.0, 1.0, 1.0]
    if flat_heads:
        assert s["margin_below_1e-5_frac"] > 0.3           # the set is far from empty here: the test has teeth
    else:
        assert s["margin_below_1e-5_frac"] < 0.01
