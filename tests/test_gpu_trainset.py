"""The labelled training set built on the GPU (utils_v2.GetTrainingSetDevice, csrc/cv_trainset.hip) against the host loop
it replaces and against the reference's own arrays: bits of X, Y and the keys, no tolerance.  Every test asserts the
route it took and the number of lines the device parser left to the host, so that neither a silent fall-back nor a
dropped line can pass."""
import ctypes
import gzip
import os
import random
import types

import numpy as np
import pytest

import trainset_cases as cases
import textparse_cases as tc

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("trainset"))
    return {case: cases.write_case(d, case) for case in cases.CASES}


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(t.shape[0], tc.NV).view(np.uint32)


def _check_set(ts, want, planted):
    total, nblocks, X, Y, keys = want
    assert ts.route == "device", ts.reason
    assert ts.host_lines == planted
    assert ts.total == total and tuple(ts.X.shape) == (total, 33, 4, 4) and tuple(ts.Y.shape) == (total, 16)
    assert ts.X.is_cuda and ts.Y.is_cuda
    assert np.array_equal(_bits(ts.X), X)
    assert np.array_equal(ts.Y.cpu().numpy().astype(np.float64), Y)
    assert ts.keys() == keys
    got = cases.arrays_of(ts.blocks())
    assert got[:2] == (total, nblocks)
    assert np.array_equal(got[2], X) and np.array_equal(got[3], Y) and got[4] == keys


def test_reference_pin(monkeypatch):
    """tests/golden/trainarray_*: 1 015 kept rows in 3 blocks, written by the reference itself"""
    from clairvoyante_amd import utils_v2
    d = np.load(os.path.join(G, "trainarray.npz"))
    fns = [os.path.join(G, n) for n in ("trainarray_tensor.txt.gz", "trainarray_var.txt.gz", "trainarray.bed.gz")]
    total = int(d["total"])
    want = (total, int(d["nblocks"]), np.ascontiguousarray(d["X"]).reshape(total, -1).view(np.uint32), d["Y"], [str(s) for s in d["pos"]])
    assert d["Y"].dtype == np.float64
    planted = cases.host_lines_of(gzip.open(fns[0], "rb").read())
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    assert utils_v2.trains_on_device(fns[0])
    random.seed(1234)
    got = cases.arrays_of(utils_v2.GetTrainingArray(*fns))
    assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]
    random.seed(1234)
    _check_set(utils_v2.GetTrainingSetDevice(*fns, num=256), want, planted)


@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("case", cases.CASES)
def test_case_files_equal_the_host_loop(files, case, shuffle, fmt):
    from clairvoyante_amd import utils_v2
    f = files[case]
    want = cases.host_result(f, case, shuffle)
    assert want[0] == {"k1000": 1000, "k0": 0, "k499": 499}.get(case, want[0])
    assert want[1] == want[0] // 500 + 1
    num = max(f["rows"] // 6, 16)                               # at least 5 slabs: runs and duplicates straddle their edges
    before = utils_v2.text_line_counts["host"]
    random.seed(cases.SEED)
    ts = utils_v2.GetTrainingSetDevice(f[fmt], f["var"], f["bed"], shuffle, num=num)
    _check_set(ts, want, f["planted"])
    assert utils_v2.text_line_counts["host"] - before == f["planted"] and ts.batches >= 5
    if case == "full" and not shuffle:
        assert keys_sorted(ts.keys()) and len(set(ts.keys())) == ts.total > 600


def keys_sorted(keys):
    return keys == sorted(keys)


def test_one_slab_at_the_abi_level(files):
    """cv_trainset_tokens / _join / _finish over the rows the parser left of one 300-line slab, against a numpy / dict
    restatement of the loop: pos, centre, run flags, keep, truth index, src, Y"""
    import torch
    from clairvoyante_amd import _lib, utils_v2
    lib = _lib.load()
    f = files["full"]
    lines = open(f["plain"], "rb").read().split(b"\n")[330:630]          # chr1 -> chr10, two tab lines, an N centre, a key twice
    text = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    dev = utils_v2._TextSlabDevice("cuda:0", 320)
    try:
        up = dev.upload(text)
        job = dev.parse(up, 0)
        info, status, meta = dev.collect(job)
    finally:
        dev.close()
    assert int(info[1]) == 300 and int(info[3]) == cases.host_lines_of(text.tobytes()) == 2
    keep = np.flatnonzero(status == tc.ROW)
    toks = [lines[i].split(b" ")[:3] for i in keep]
    n = len(keep)
    assert 280 < n < 300
    tree, Ytruth = utils_v2._read_bed_truth(f["var"], f["bed"])
    names, t = utils_v2._trainset_tables(tree, Ytruth, True)
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = lambda x: ctypes.c_void_p(x.data_ptr()) if x.numel() else None
    idx = D(keep.astype(np.int64))
    pos = torch.empty(n, dtype=torch.int64, device="cuda"); run = torch.empty(n, dtype=torch.int32, device="cuda")
    digits, centre, flags = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(3))
    need = ctypes.c_int64()
    _lib.check(lib.cv_trainset_tokens_workspace(n, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.cv_trainset_tokens(ctypes.c_void_p(job["text_ptr"]), ctypes.c_void_p(job["meta_ptr"]), P(idx), n, P(pos), P(digits),
                                      P(centre), P(flags), P(run), P(ws), need.value, st))
    want_pos = np.array([int(tk[1]) for tk in toks])
    want_start = np.array([i == 0 or toks[i][0] != toks[i - 1][0] for i in range(n)])
    assert np.array_equal(pos.cpu().numpy(), want_pos)
    assert np.array_equal(digits.cpu().numpy(), [len(tk[1]) for tk in toks])
    assert np.array_equal(centre.cpu().numpy(), ["ACGT".index(chr(tk[2][16]).upper()) for tk in toks])
    assert np.array_equal(flags.cpu().numpy(), want_start.astype(np.uint8))          # RUN_START only: no bad token
    assert np.array_equal(run.cpu().numpy(), np.cumsum(want_start) - 1) and want_start.sum() == 2
    ids = {nm: i for i, nm in enumerate(names)}
    run_ctg = np.array([ids[toks[i][0]] for i in np.flatnonzero(want_start)], dtype=np.int32)
    tab = {k: D(v) for k, v in t.items()}
    ctg = torch.empty(n, dtype=torch.int32, device="cuda"); truth = torch.empty(n, dtype=torch.int32, device="cuda")
    kp = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(lib.cv_trainset_join(n, P(run), P(D(run_ctg)), len(run_ctg), P(pos), len(names), 1, P(tab["bed_off"]), P(tab["bed_begin"]),
                                    P(tab["bed_emax"]), P(tab["truth_off"]), P(tab["truth_pos"]), P(ctg), P(kp), P(truth), st))
    want_keep = np.array([bool(tree[tk[0].decode()].hit(int(tk[1]))) for tk in toks])
    key_of = lambda tk: tk[0].decode() + ":" + tk[1].decode()
    tkeys = ["%s:%d" % (names[c].decode(), p) for c in range(len(names))
             for p in t["truth_pos"][t["truth_off"][c]:t["truth_off"][c + 1]]]
    want_truth = np.array([tkeys.index(key_of(tk)) if key_of(tk) in Ytruth else -1 for tk in toks])
    assert np.array_equal(ctg.cpu().numpy(), [ids[tk[0]] for tk in toks])
    assert np.array_equal(kp.cpu().numpy().astype(bool), want_keep) and 0 < want_keep.sum() < n
    assert np.array_equal(truth.cpu().numpy(), want_truth) and (want_truth >= 0).sum() >= 2
    # finish: the loop's dicts
    Xd, Yd = {}, dict(Ytruth)
    for i, tk in enumerate(toks):
        if want_keep[i]:
            k = key_of(tk)
            Xd[k] = i
            if k not in Yd:
                v = [0.0] * 16; v[5] = v[6] = v[10] = 1.0; v["ACGT".index(chr(tk[2][16]).upper())] = 1.0
                Yd[k] = v
    order = sorted(Xd)
    assert len(order) < want_keep.sum()                         # (the slab holds a key twice)
    _lib.check(lib.cv_trainset_finish_workspace(n, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    src = torch.full((n,), -1, dtype=torch.int64, device="cuda"); y = torch.zeros((n, 16), dtype=torch.float32, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(lib.cv_trainset_finish(n, P(ctg), P(pos), P(digits), P(centre), P(kp), P(truth), P(D(utils_v2.contig_ranks(names))), len(names),
                                      P(tab["labels"]), len(t["labels"]), P(src), P(y), P(total), P(ws), need.value, st))
    assert int(total.item()) == len(order)
    assert np.array_equal(src.cpu().numpy()[:len(order)], [Xd[k] for k in order])
    assert np.array_equal(y.cpu().numpy()[:len(order)].astype(np.float64), np.array([Yd[k] for k in order]))


def _variant(files, tmp_path, edit):
    """the k499 file with row 250 changed by edit(fields)"""
    lines = open(files["k499"]["plain"], "rb").read().split(b"\n")
    fields = lines[250].split(b" ")
    edit(fields)
    lines[250] = b" ".join(fields)
    fn = str(tmp_path / "variant.txt")
    with open(fn, "wb") as fh:
        fh.write(b"\n".join(lines))
    return fn


def test_noncanonical_coordinate_goes_to_the_host_builder(files, tmp_path):
    from clairvoyante_amd import utils_v2

    def edit(f):
        f[1] = b"007"
    fn = _variant(files, tmp_path, edit)
    random.seed(3); want = cases.arrays_of(utils_v2._training_array_host(fn, None, None))
    random.seed(3); ts = utils_v2.GetTrainingSetDevice(fn, None, None, num=100)
    assert ts.route == "host" and "canonical" in ts.reason and "chr3:007" in want[4]
    got = cases.arrays_of(ts.blocks())
    assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]


def test_contig_with_a_colon_raises_what_the_host_loop_raises(files, tmp_path):
    from clairvoyante_amd import utils_v2

    def edit(f):
        f[0] = b"ch:r1"
    fn = _variant(files, tmp_path, edit)
    with pytest.raises(ValueError) as host:
        utils_v2._training_array_host(fn, None, None)
    with pytest.raises(ValueError) as device:
        utils_v2.GetTrainingSetDevice(fn, None, None, num=100)
    assert str(device.value) == str(host.value)


def test_a_set_that_would_not_fit_goes_to_the_host_builder(files, monkeypatch):
    from clairvoyante_amd import utils_v2
    f = files["full"]
    want = cases.host_result(f, "full", True)
    monkeypatch.setattr(utils_v2, "TRAINSET_FREE_BYTES", 1 << 20)
    random.seed(cases.SEED)
    ts = utils_v2.GetTrainingSetDevice(f["plain"], f["var"], f["bed"])
    assert ts.route == "host" and "fit" in ts.reason
    got = cases.arrays_of(ts.blocks())
    assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]


def _slim_model():
    from clairvoyante_amd import clairvoyante_v3_slim
    m = clairvoyante_v3_slim.Clairvoyante()
    m._seed_rng.seed(5)
    m._dropout_seed = 12345
    m.init()
    m.setLearningRate(1e-3)
    return m


def _weights(m):
    import torch
    from clairvoyante_amd import _lib
    w = torch.empty(m.numParameters, device="cuda")
    _lib.check(m._lib.cv_flat_copy(m._h, 0, ctypes.c_void_p(w.data_ptr()), 0, None))
    return w.cpu().numpy().view(np.uint32).copy()


def test_an_epoch_from_the_resident_set_equals_one_from_its_blocks(files, monkeypatch):
    """two models with equal parameters and dropout seed: one epoch over slices of the set in HBM, one over its blocks
    (decompressed, copied back) -- the same batches, so the same parameters bit for bit and the same loss sums"""
    from clairvoyante_amd import param, train, utils_v2
    monkeypatch.setattr(param, "trainBatchSize", 256)
    monkeypatch.setattr(param, "predictBatchSize", 16)
    f = files["nobed"]
    random.seed(cases.SEED)
    ts = utils_v2.GetTrainingSetDevice(f["plain"], f["var"], None)
    assert ts.route == "device" and ts.total > 1200
    total, XC, YC, _PC = ts.blocks()
    vstart = int(total * param.trainingDatasetPercentage) + 1
    _t, XR, YR = ts.resident()
    assert len(XR) == len(XC)
    x, nx, end = utils_v2.DecompressArray(XR, 300, 256, total)
    assert x.is_cuda and nx == 256 and end == 0 and x.data_ptr() == ts.X[300:].data_ptr()       # a view: no copy
    out = []
    for xc, yc in ((XR, YR), (XC, YC)):
        m = _slim_model()
        before = _weights(m)
        sums = train.run_epoch(train._BatchStream(utils_v2, xc, yc, total, vstart), m, 0, 1, None, 1, vstart)
        out.append((sums, _weights(m), before))
        m.close()
    assert np.array_equal(out[0][2], out[1][2]) and not np.array_equal(out[0][1], out[0][2])
    assert np.array_equal(out[0][1], out[1][1])
    assert out[0][0] == out[1][0] and out[0][0][0] > 0 and out[0][0][1] > 0


def test_train_run_from_text_tensors_keeps_the_set_resident(files, tmp_path, monkeypatch):
    from clairvoyante_amd import param, train, utils_v2
    monkeypatch.setattr(param, "trainBatchSize", 256)
    monkeypatch.setattr(param, "predictBatchSize", 16)
    monkeypatch.setattr(param, "maxEpoch", 3)
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    routes, build = [], utils_v2.GetTrainingSetDevice

    def spy(*a, **kw):
        ts = build(*a, **kw)
        routes.append((ts.route, ts.host_lines))
        return ts
    monkeypatch.setattr(utils_v2, "GetTrainingSetDevice", spy)
    f = files["full"]
    prefix = str(tmp_path / "out" / "model")
    os.makedirs(os.path.dirname(prefix))
    args = types.SimpleNamespace(bin_fn=None, tensor_fn=f["plain"], var_fn=f["var"], bed_fn=f["bed"], chkpnt_fn=None,
                                 learning_rate=1e-3, lambd=1e-3, ochk_prefix=prefix, olog_dir=None, v2=False, v3=True, slim=True)
    train.Run(args)
    assert routes == [("device", f["planted"])]
    assert os.path.exists("%s-%06d.index" % (prefix, 1)) and os.path.exists("%s-%06d.index" % (prefix, 2))


def test_tensor2bin_writes_the_host_loops_arrays(files, tmp_path, monkeypatch):
    from clairvoyante_amd import tensor2Bin, utils_v2
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    f = files["full"]
    want = cases.host_result(f, "full", True)
    routes, build = [], utils_v2.GetTrainingSetDevice

    def spy(*a, **kw):
        ts = build(*a, **kw)
        routes.append((ts.route, ts.host_lines))
        return ts
    monkeypatch.setattr(utils_v2, "GetTrainingSetDevice", spy)
    out = str(tmp_path / "t.bin")
    random.seed(cases.SEED)
    tensor2Bin.Run(types.SimpleNamespace(tensor_fn=f["bgzf"], var_fn=f["var"], bed_fn=f["bed"], bin_fn=out))
    assert routes == [("device", f["planted"])]
    for lazy in (False, True):
        got = cases.arrays_of(utils_v2.LoadBin(out, lazy=lazy))
        assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]
