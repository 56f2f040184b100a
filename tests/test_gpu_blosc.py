"""The blocks of a .bin set decoded on the device (csrc/cv_blosc_dev.hip) and the route built on it
(utils_v2.DecompressArrayDevice).  The checker is the host decoder (cv_blosc_unpack_blocks / DecompressArray), bit for
bit.  On the corpus NO chunk may go to the host: the fallback must not hide a decoder that only takes easy streams.  The
damaged chunks are the first few hundred of the seeded set tests/test_blosc_core_sanitized.py runs through the same
decode core under AddressSanitizer; they are given to the device once."""
import ctypes
import os

import numpy as np
import pytest

import blosc_cases as B

pytestmark = pytest.mark.gpu

CANARY, GAP = 0xC7, 128


def host_unpack(chunks, block_bytes):
    """cv_blosc_unpack_blocks -> (status [n], lens [n], [payload bytes])"""
    from clairvoyante_amd import _lib
    n = len(chunks)
    hold = [np.frombuffer(c, dtype=np.uint8) for c in chunks]
    src = (ctypes.c_void_p * n)(*[h.ctypes.data for h in hold])
    clen = (ctypes.c_int64 * n)(*[len(c) for c in chunks])
    out = np.zeros(max(1, n * block_bytes), dtype=np.uint8)
    lens, status = (ctypes.c_int64 * n)(), (ctypes.c_int32 * n)()
    _lib.load().cv_blosc_unpack_blocks(src, clen, n, out.ctypes.data_as(ctypes.c_void_p), block_bytes, lens, status)
    return np.array(status[:]), np.array(lens[:]), [out[i * block_bytes:i * block_bytes + lens[i]].tobytes() for i in range(n)]


def device_unpack(chunks, block_bytes, max_nbytes=B.NBYTES_CAP):
    """the chunks through cv_blosc_plan, cv_blosc_decode_dev and cv_blosc_unpack_dev in ONE call each, with GAP canary bytes
    in front of and behind the scratch and the destination -> (status, lens, [payload bytes], stream status, planned,
    canaries intact)"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    n = len(chunks)
    hold = [np.frombuffer(c, dtype=np.uint8) for c in chunks]
    src = (ctypes.c_void_p * n)(*[h.ctypes.data for h in hold])
    clen = (ctypes.c_int64 * n)(*[len(c) for c in chunks])
    max_streams = 1 << 17
    srows = np.zeros((max_streams, 5), dtype=np.int64)
    crows = np.zeros((n, 10), dtype=np.int64)
    ns, comp_bytes, scratch_bytes = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    refused = lib.cv_blosc_plan(src, clen, n, max_nbytes, max_streams, srows.ctypes.data_as(ctypes.c_void_p),
                                crows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ns), ctypes.byref(comp_bytes),
                                ctypes.byref(scratch_bytes))
    assert refused >= 0
    ns, comp_bytes, scratch_bytes = ns.value, comp_bytes.value, scratch_bytes.value
    slab = np.full(comp_bytes + 16, 0xEE, dtype=np.uint8)
    for i in range(n):
        if not crows[i, 7]:
            slab[crows[i, 8]:crows[i, 8] + len(chunks[i])] = hold[i]
    comp = torch.from_numpy(slab).cuda()
    srows_dev = torch.from_numpy(srows[:max(ns, 1)].copy()).cuda()
    crows_dev = torch.from_numpy(crows).cuda()
    scratch = torch.full((GAP + scratch_bytes + GAP,), CANARY, dtype=torch.uint8, device="cuda")
    dst = torch.full((GAP + n * block_bytes + GAP,), CANARY, dtype=torch.uint8, device="cuda")
    sstat = torch.zeros(max(ns, 1), dtype=torch.uint8, device="cuda")
    lens = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(lib.cv_blosc_decode_dev(comp.data_ptr(), comp_bytes, srows_dev.data_ptr(), ns, scratch.data_ptr() + GAP,
                                       scratch_bytes, sstat.data_ptr(), stream))
    _lib.check(lib.cv_blosc_unpack_dev(crows_dev.data_ptr(), n, sstat.data_ptr(), ns, scratch.data_ptr() + GAP, scratch_bytes,
                                       dst.data_ptr() + GAP, block_bytes, lens.data_ptr(), status.data_ptr(), stream))
    torch.cuda.synchronize()
    sc, out = scratch.cpu().numpy(), dst.cpu().numpy()
    lens, status = lens.cpu().numpy(), status.cpu().numpy()
    intact = bool(np.all(sc[:GAP] == CANARY) and np.all(sc[GAP + scratch_bytes:] == CANARY) and np.all(out[:GAP] == CANARY)
                  and np.all(out[GAP + n * block_bytes:] == CANARY))
    outs = []
    for i in range(n):
        lo = GAP + i * block_bytes
        ln = int(lens[i]) if status[i] == 0 else 0
        outs.append(out[lo:lo + ln].tobytes())
        if status[i] == 0:                       # (a chunk that is not ok may have written inside its own place)
            intact = intact and bool(np.all(out[lo + ln:lo + block_bytes] == CANARY))
    return status, lens, outs, sstat.cpu().numpy()[:ns], crows[:, 7] == 0, intact


def test_the_corpus_against_the_host_decoder_and_no_chunk_goes_to_the_host():
    """every chunk alone as the last of its call (its own payload length as block_bytes), and in front of an empty block"""
    empty = dict(B.corpus())["empty trailing block, old writer"]
    for name, chunk in B.corpus():
        if B.unsupported(chunk):
            continue
        hs, hl, ho = host_unpack([chunk], B.NBYTES_CAP // 2)
        block_bytes = max(int(hl[0]), 16)
        for group in ([chunk], [chunk, empty]):
            hs, hl, ho = host_unpack(group, block_bytes)
            ds, dl, do, sstat, planned, intact = device_unpack(group, block_bytes)
            assert intact, name
            assert planned.all() and np.all(sstat == B.OK), "%s: a stream came back HOST" % name
            assert list(ds) == list(hs) and list(dl) == list(hl), (name, ds, hs, dl, hl)
            assert do == ho, name
            assert ds[0] != 1


def test_the_invalid_ending_goes_back_to_the_host():
    ds, _dl, _do, sstat, planned, intact = device_unpack([B.zero_literal_ending()], 4096)
    assert intact and planned.all() and list(sstat) == [B.HOST] and list(ds) == [1]


def test_several_hundred_chunks_in_one_call():
    """mixed layouts side by side: both writers, block sizes from 1 KiB to 1 MiB, real c-blosc chunks, one short last"""
    from clairvoyante_amd import utils_v2
    x, _y = B.candidates(40, seed=7)
    block_bytes = x[:8].nbytes
    chunks = []
    for k in range(320):
        a = x[(k * 3) % 32:(k * 3) % 32 + 8]
        chunks.append(utils_v2.pack_array(a, [None, 1024, 4096, 16384, 1 << 20][k % 5]))
    chunks.append(utils_v2.pack_array(x[:3], 4096))
    hs, hl, ho = host_unpack(chunks, block_bytes)
    assert not hs.any()
    ds, dl, do, sstat, planned, intact = device_unpack(chunks, block_bytes)
    assert intact and planned.all() and np.all(sstat == B.OK)
    assert list(ds) == list(hs) and list(dl) == list(hl) and do == ho


def test_damaged_chunks_are_handed_back_or_right():
    base, block_bytes = B.equal_payload_base()
    chunks = list(B.mutations(300, seed=4321, base=base))
    ds, dl, do, sstat, planned, intact = device_unpack(chunks, block_bytes, max_nbytes=block_bytes + 4096)
    assert intact
    assert set(np.unique(sstat)) <= {B.OK, B.HOST}
    # (a header that claims more than the cap is not given to the host decoder, which would allocate it: not ok)
    hs, hl, ho = host_unpack([c if len(c) >= 16 and 0 <= int.from_bytes(c[4:8], "little", signed=True) <= B.NBYTES_CAP else b"\x00"
                              for c in chunks], block_bytes)
    ok = 0
    for k in range(len(chunks)):
        if ds[k] == 0:
            ok += 1
            assert hs[k] == 0 and dl[k] == hl[k] and do[k] == ho[k], "mutation %d: ok on the device, but not the host's bytes" % k
    print("%d damaged chunks: %d ok on the device, %d on the host" % (len(chunks), ok, int((hs == 0).sum())))
    assert 0 < ok <= int((hs == 0).sum()) < len(chunks) // 2


def _lists(blocksize, n=None):
    from clairvoyante_amd import param, utils_v2
    bs = param.bloscBlockSize
    n = n or 2 * bs + 37
    x, y = B.candidates(n, seed=11)
    XC = [utils_v2.pack_array(x[s:s + bs], blocksize) for s in range(0, n + bs, bs)]
    YC = [utils_v2.pack_array(y[s:s + bs], blocksize) for s in range(0, n + bs, bs)]
    assert len(XC) == 4
    return n, x, y, XC, YC


@pytest.mark.parametrize("blocksize", [None, 1 << 20, 65536])
def test_decompress_array_device_against_the_host(blocksize):
    from clairvoyante_amd import param, utils_v2
    total, x, y, XC, YC = _lists(blocksize)
    bs = param.bloscBlockSize
    before = utils_v2.bin_decode_counts()
    windows = [(10, 100, total), (bs - 5, 10, total), (bs, bs, total), (0, total, total), (3, 2 * bs, total),
               (total - 40, 40, total), (bs + 1, 5000, total), (total - 1, 1, total), (total - 1, 10, total),
               (7, 600, 400)]
    for lst, ref in ((XC, x), (YC, y)):
        for start, num, maximum in windows:
            want, wn, wend = utils_v2.DecompressArray(lst, start, num, maximum)
            got = utils_v2.DecompressArrayDevice(lst, start, num, maximum)
            assert got is not None
            t, gn, gend = got
            assert (gn, gend) == (wn, wend) and t.is_cuda
            g = t.cpu().numpy()
            assert g.dtype == want.dtype == ref.dtype and g.shape == want.shape
            assert g.tobytes() == np.ascontiguousarray(want).tobytes()
    after = utils_v2.bin_decode_counts()
    assert after["host"] == before["host"] and after["device"] > before["device"]


def test_an_empty_set_and_position_strings():
    from clairvoyante_amd import utils_v2
    x, _y = B.candidates(4, seed=1)
    XC = [utils_v2.pack_array(x[:0])]
    want = utils_v2.DecompressArray(XC, 0, 0, 0)
    got = utils_v2.DecompressArrayDevice(XC, 0, 0, 0)
    assert got is None or (got[1], got[2]) == (want[1], want[2])
    PC = [utils_v2.pack_array(np.array(["chr1:%d:ACGT" % k for k in range(500)])), utils_v2.pack_array(np.array([], dtype="<U4"))]
    assert utils_v2.DecompressArrayDevice(PC, 0, 500, 500) is None


def test_a_damaged_chunk_gives_the_hosts_exception():
    from clairvoyante_amd import utils_v2
    total, _x, _y, XC, _YC = _lists(65536)
    bad = bytearray(XC[1])
    bad[16:20] = (8).to_bytes(4, "little")               # the first block would start inside the header
    XC = [XC[0], bytes(bad), XC[2], XC[3]]
    with pytest.raises(Exception) as host:
        utils_v2.DecompressArray(XC, 0, total, total)
    with pytest.raises(Exception) as dev:
        utils_v2.DecompressArrayDevice(XC, 0, total, total)
    assert type(dev.value) is type(host.value) and str(dev.value) == str(host.value)


def test_the_route_rule(monkeypatch):
    from clairvoyante_amd import _lib, utils_v2
    _total, _x, _y, XC, _YC = _lists(None)
    monkeypatch.delenv("CV_BIN_DECODE", raising=False)
    floors = [f for f in utils_v2.BIN_DECODE_FLOOR.values() if f is not None]
    assert utils_v2.bin_decode_route(XC, 1) == "host"              # 500 candidates: below every floor
    assert not floors or min(floors) > 500
    monkeypatch.setenv("CV_BIN_DECODE", "device")
    assert utils_v2.bin_decode_route(XC, 1) == "device"
    assert utils_v2.bin_decode_route(utils_v2.ResidentBlocks(__import__("torch").zeros(3, 2, device="cuda")), 1) == "host"
    monkeypatch.setenv("CV_BIN_DECODE", "host")
    assert utils_v2.bin_decode_route(XC, 1000) == "host"
    monkeypatch.setenv("CV_BIN_DECODE", "yes")
    with pytest.raises(_lib.CvError):
        utils_v2.bin_decode_route(XC, 1)


# ---- the drivers ---------------------------------------------------------------------------------------------------

N_BIN = 2000


@pytest.fixture(scope="module")
def bins(tmp_path_factory):
    """a 2 000-candidate .bin in c-blosc's layout and in 64 KiB blocks, and two slim checkpoints"""
    import pickle
    import types
    import common
    from clairvoyante_amd import clairvoyante_v3_slim, synth, utils_v2
    d = tmp_path_factory.mktemp("blosc_bin")
    xt, cls, rf, alt, il = synth.make_candidates(N_BIN, seed=41, return_class=True)
    y = synth.make_labels(cls, rf, alt, il).numpy().astype(np.float64); x = xt.numpy()
    fns = {}
    for tag, blocksize in (("cblosc", 1 << 20), ("own64k", 65536)):
        XC = [utils_v2.pack_array(x[s:s + 500], blocksize) for s in range(0, N_BIN + 1, 500)]
        YC = [utils_v2.pack_array(y[s:s + 500], blocksize) for s in range(0, N_BIN + 1, 500)]
        fns[tag] = str(d / (tag + ".bin"))
        with open(fns[tag], "wb") as fh:
            pickle.dump(N_BIN, fh); pickle.dump(XC, fh); pickle.dump(YC, fh); pickle.dump([], fh)
    prefixes = []
    m = clairvoyante_v3_slim.Clairvoyante()
    for seed in (1, 2):
        m.setParameters(common.bench_params(None, "slim", seed=seed))
        prefixes.append(str(d / ("model-%06d" % seed))); m.saveParameters(prefixes[-1])
    m.close()
    lst = d / "models.txt"
    lst.write_text("".join(p + "\n" for p in prefixes))
    return types.SimpleNamespace(fns=fns, prefixes=prefixes, lst=str(lst), chunks=2 * (N_BIN // 500 + 1))


def _logged(fn):
    import logging
    logs = []

    class H(logging.Handler):
        def emit(self, rec):
            msg = rec.getMessage()
            if "time elapsed" not in msg:
                logs.append(msg)
    h = H(); root = logging.getLogger(); level = root.level
    root.addHandler(h); root.setLevel(logging.INFO)
    try:
        fn()
    finally:
        root.removeHandler(h); root.setLevel(level)
    return logs


@pytest.mark.parametrize("layout", ["cblosc", "own64k"])
@pytest.mark.parametrize("mode", ["resident", "streamed"])
def test_evaluate_lines_are_the_same_on_both_routes(bins, monkeypatch, layout, mode):
    import types
    from clairvoyante_amd import evaluate, evaluateListOfModels, train, utils_v2
    if mode == "streamed":
        monkeypatch.setattr(utils_v2, "TRAINSET_FREE_BYTES", 1 << 20)   # the set does not "fit": it stays in its blocks
        monkeypatch.setattr(train, "EVAL_PASS", 512)
    a = dict(bin_fn=bins.fns[layout], tensor_fn=None, var_fn=None, bed_fn=None, v2=False, v3=True, slim=True)
    runs = (lambda: evaluate.Run(types.SimpleNamespace(chkpnt_fn=bins.prefixes[0], **a)),
            lambda: evaluateListOfModels.Run(types.SimpleNamespace(chkpnt_list=bins.lst, **a)))
    lines = {}
    for route in ("host", "device"):
        monkeypatch.setenv("CV_BIN_DECODE", route)
        before = utils_v2.bin_decode_counts()
        lines[route] = [_logged(r) for r in runs]
        after = utils_v2.bin_decode_counts()
        assert after["host"] == before["host"]
        if route == "host":
            assert after == before
        else:
            assert after["device"] - before["device"] >= bins.chunks     # every chunk of X and Y, of every walk
    assert lines["device"] == lines["host"]
    assert len(lines["host"][0]) == 4 + 17


def test_two_epochs_of_training_are_the_same_bits_on_both_routes(tmp_path, monkeypatch):
    import types
    import common
    from clairvoyante_amd import clairvoyante_v3_slim, param, train, utils_v2
    monkeypatch.setattr(param, "maxEpoch", 3)              # two epochs
    out = {}
    for route in ("host", "device"):
        monkeypatch.setenv("CV_BIN_DECODE", route)
        before = utils_v2.bin_decode_counts()
        m = clairvoyante_v3_slim.Clairvoyante(dropoutRateFC4=0.0, dropoutRateFC5=0.0)
        m.setParameters(common.bench_params(None, "slim", seed=3))
        args = types.SimpleNamespace(bin_fn=os.path.join(B.GOLDEN, "mini.bin"), tensor_fn=None, var_fn=None, bed_fn=None,
                                     chkpnt_fn=None, learning_rate=1e-3, lambd=1e-3, ochk_prefix=str(tmp_path / route / "model"),
                                     olog_dir=None, v2=False, v3=True, slim=True)
        os.makedirs(str(tmp_path / route))
        logs = _logged(lambda: train.TrainAll(args, m, utils_v2))
        w = [np.asarray(v).copy() for _k, v in sorted(m.getParameters().items())]
        m.close()
        after = utils_v2.bin_decode_counts()
        out[route] = ([l for l in logs if "model-" not in l and str(tmp_path) not in l], w, after["device"] - before["device"])
    assert out["host"][2] == 0 and out["device"][2] > 0
    assert out["device"][0] == out["host"][0] and any("loss" in l.lower() for l in out["host"][0])
    assert len(out["host"][1]) == len(out["device"][1])
    for a, b in zip(out["host"][1], out["device"][1]):
        assert a.tobytes() == b.tobytes()
