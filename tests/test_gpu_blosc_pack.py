"""The X blocks of a resident training set packed on the device (csrc/cv_blosc_pack_dev.hip) and the route built on it
(utils_v2.pack_blocks_device, TrainingSet.blocks() under CV_BIN_PACK=device, tensor2Bin --pack device).  The kernel is
held to the host form of the same encode core (cv_blosc_pack_host_form, which tests/test_lz4enc_core_host.py runs under
sanitizers) byte for byte, and every chunk must be the pickle of its rows again, through the host decoder and through
the device's strict one.  The shapes are the smallest at which the writer can go wrong: sets around one and two chunks,
blocks that split, blocks that do not, a leftover block, streams above the device's cap."""
import ctypes
import os
import pickle
import random
import types

import numpy as np
import pytest

import bamtrain_cases as bc
import trainset_cases as cases

pytestmark = pytest.mark.gpu

CANARY, GAP = 0xC7, 256
BS = 500
SHAPE = (33, 4, 4)
ROW = 33 * 4 * 4 * 4


def _synth(n):
    from clairvoyante_amd import synth
    return np.ascontiguousarray(synth.make_candidates(n).numpy(), dtype=np.float32) if n else np.zeros((0,) + SHAPE, np.float32)


def _contents(name, n):
    r = np.random.RandomState(len(name))
    if name == "synth":
        return _synth(n)
    if name == "zero":
        return np.zeros((n,) + SHAPE, np.float32)
    if name == "constant":
        return np.full((n,) + SHAPE, 3.0, np.float32)
    if name == "specials":                                       # -0.0, NaNs, denormals, infinities
        bits = np.array([0x80000000, 0x7fc00000, 0xffc00001, 0x00000001, 0x807fffff, 0x7f800000, 0, 0x3f800000], dtype=np.uint32)
        return bits[r.randint(0, len(bits), size=(n,) + SHAPE)].view(np.float32)
    if name.startswith("period"):
        base = _synth(3)[:int(name[-1])]
        return np.ascontiguousarray(base[np.arange(n) % len(base)])
    if name == "random bits":
        return r.randint(0, 1 << 32, size=(n,) + SHAPE, dtype=np.uint64).astype(np.uint32).view(np.float32)
    raise KeyError(name)


def _pieces(n):
    """[(first item, chunks, items per chunk)]: the full chunks in one call, the partial one in a call of its own"""
    out = [(0, n // BS, BS)] if n >= BS else []
    if n % BS:
        out.append((n // BS * BS, 1, n % BS))
    return out


def host_form(x, lo, chunks, items, blocksize):
    from clairvoyante_amd import _lib, utils_v2
    lib = _lib.load()
    head, tail = utils_v2.pickle_envelope((items,) + SHAPE, np.float32)
    cap = chunks * (16 + len(head) + items * ROW + len(tail))
    out = ctypes.create_string_buffer(cap)
    off, status = (ctypes.c_int64 * (chunks + 1))(), (ctypes.c_int32 * chunks)()
    part = np.ascontiguousarray(x[lo:lo + chunks * items])
    _lib.check(lib.cv_blosc_pack_host_form(part.ctypes.data_as(ctypes.c_void_p), chunks, items * ROW, head, len(head), tail, len(tail), 4,
                                           blocksize, out, cap, off, status))
    return [out.raw[off[c]:off[c + 1]] if status[c] == 1 else None for c in range(chunks)]


def device_form(x_dev, lo, chunks, items, blocksize):
    """cv_blosc_pack_dev over one piece, GAP canary bytes around the output slab, the tables and the workspace
    -> [chunk or None (HOST)]"""
    import torch
    from clairvoyante_amd import _lib, utils_v2
    lib = _lib.load()
    head, tail = utils_v2.pickle_envelope((items,) + SHAPE, np.float32)
    ws_bytes, bound = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.cv_blosc_pack_workspace(chunks, len(head) + items * ROW + len(tail), 4, blocksize, ctypes.byref(ws_bytes), ctypes.byref(bound)))
    ws_bytes, bound = ws_bytes.value, bound.value
    assert bound == chunks * (16 + len(head) + items * ROW + len(tail))
    st_bytes = 8 * (chunks + 1) + 4 * chunks
    bufs = [torch.full((GAP + n + GAP,), CANARY, dtype=torch.uint8, device="cuda") for n in (bound, st_bytes, ws_bytes)]
    slab, state, ws = [b[GAP:GAP + n] for b, n in zip(bufs, (bound, st_bytes, ws_bytes))]
    assert all(t.data_ptr() % 16 == 0 for t in (slab, state, ws))
    _lib.check(lib.cv_blosc_pack_dev(x_dev.data_ptr() + lo * ROW, chunks, items * ROW, head, len(head), tail, len(tail), 4, blocksize,
                                     slab.data_ptr(), bound, state.data_ptr(), state.data_ptr() + 8 * (chunks + 1), ws.data_ptr(), ws_bytes,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for b, n in zip(bufs, (bound, st_bytes, ws_bytes)):
        edge = torch.cat([b[:GAP], b[GAP + n:]]).cpu().numpy()
        assert (edge == CANARY).all(), "bytes around a buffer of %d were written" % n
    got = state.cpu().numpy()
    off, status = got[:8 * (chunks + 1)].view(np.int64), got[8 * (chunks + 1):].view(np.int32)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[chunks] <= bound and set(status.tolist()) <= {1, 2}
    raw = slab[:int(off[chunks])].cpu().numpy()
    # what lies behind the last chunk was never written
    assert (slab[int(off[chunks]):].cpu().numpy() == CANARY).all()
    for c in range(chunks):
        assert status[c] == 1 or off[c + 1] == off[c]
    return [raw[off[c]:off[c + 1]].tobytes() if status[c] == 1 else None for c in range(chunks)]


def check_set(x, blocksize):
    """every chunk of the set: device bytes == host form's, twice; the chunk is the pickle of its rows again -> [chunk or None]"""
    import torch
    from clairvoyante_amd import utils_v2
    x_dev = torch.from_numpy(x).cuda()
    out = []
    for lo, chunks, items in _pieces(len(x)):
        dev = device_form(x_dev, lo, chunks, items, blocksize)
        assert dev == device_form(x_dev, lo, chunks, items, blocksize), "two runs differ"
        want = host_form(x, lo, chunks, items, blocksize)
        assert [None if d is None else len(d) for d in dev] == [None if w is None else len(w) for w in want]
        assert dev == want, "the device's bytes are not the host form's"
        for c, chunk in enumerate(dev):
            rows = x[lo + c * items:lo + (c + 1) * items]
            if chunk is not None:
                assert utils_v2.blosc_decompress(chunk) == pickle.dumps(rows, pickle.HIGHEST_PROTOCOL)
                assert np.array_equal(utils_v2.unpack_array(chunk).view(np.uint32), rows.view(np.uint32))
        out += dev
    return out


@pytest.mark.parametrize("blocksize", [512, 65536])
@pytest.mark.parametrize("n", [0, 1, 499, 500, 501, 1037])
def test_set_sizes(n, blocksize):
    got = check_set(_synth(n), blocksize)
    assert len(got) == (n + BS - 1) // BS and None not in got


@pytest.mark.parametrize("blocksize", [508, 4096])
def test_blocks_that_do_not_split_and_small_ones(blocksize):
    got = check_set(_synth(1037), blocksize)
    assert len(got) == 3 and None not in got
    for chunk in got:
        nblocks = -(-int.from_bytes(chunk[4:8], "little") // blocksize)
        first = int.from_bytes(chunk[16:20], "little")
        assert first == 16 + 4 * nblocks


@pytest.mark.parametrize("blocksize", [512, 65536])
@pytest.mark.parametrize("name", ["zero", "constant", "specials", "period 1", "period 2", "period 3", "random bits"])
def test_contents(name, blocksize):
    got = check_set(_contents(name, 501), blocksize)
    assert len(got) == 2
    if name == "random bits":
        assert got == [None, None]                              # every stream stored: no chunk shrinks, every chunk is the host's
    else:
        assert None not in got


def _decoded(blocks, x):
    from clairvoyante_amd import utils_v2
    assert len(blocks) == (len(x) + BS - 1) // BS
    for c, chunk in enumerate(blocks):
        rows = x[c * BS:(c + 1) * BS]
        assert utils_v2.blosc_decompress(chunk) == pickle.dumps(rows, pickle.HIGHEST_PROTOCOL)
        assert np.array_equal(utils_v2.unpack_array(chunk).view(np.uint32), rows.view(np.uint32))


@pytest.mark.parametrize("name,n,blocksize,device,host", [("synth", 1037, None, 3, 0), ("synth", 501, 512, 2, 0), ("random bits", 501, 4096, 0, 2),
                                                          ("synth", 501, 4 * 65536, 1, 1), ("synth", 0, None, 0, 0)])
def test_the_route_and_its_counts(name, n, blocksize, device, host, monkeypatch):
    """pack_blocks_device: the chunks in order, HOST chunks and pieces the device does not take packed by the host, and the
    counts showing which.  4 * 65 536: the planes of a full chunk's blocks exceed the device's cap (the partial chunk of
    one row is a single smaller block and stays on the device)"""
    import torch
    from clairvoyante_amd import _lib, utils_v2
    assert _lib.load().cv_blosc_pack_stream_cap() == 65535
    monkeypatch.setattr(utils_v2, "PACK_PIECE_CHUNKS", 1)       # more than one piece
    x = _contents(name, n)
    before = utils_v2.bin_pack_counts()
    blocks = utils_v2.pack_blocks_device(torch.from_numpy(x).cuda(), blocksize)
    after = utils_v2.bin_pack_counts()
    assert (after["device"] - before["device"], after["host"] - before["host"]) == (device, host)
    _decoded(blocks, x)
    for chunk in blocks:                                        # the blocksize asked for (65 536 when none is), cut to the data
        assert int.from_bytes(chunk[8:12], "little") <= min(blocksize or 65536, int.from_bytes(chunk[4:8], "little"))


def _training_set(x, seed=5):
    import torch
    from clairvoyante_amd import utils_v2
    n = len(x)
    r = np.random.RandomState(seed)
    y = np.zeros((n, 16), np.float32)
    y[np.arange(n), r.randint(0, 16, n)] = 1
    return utils_v2.TrainingSet(n, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), "device", names=[b"ctgA", b"ctgB"],
                                key_ctg=torch.from_numpy(r.randint(0, 2, n).astype(np.int32)).cuda(),
                                key_pos=torch.from_numpy(np.arange(n, dtype=np.int64) * 7 + 1).cuda())


@pytest.mark.parametrize("n", [1000, 1037])
def test_blocks_on_both_routes_and_both_decoders(n, monkeypatch):
    """TrainingSet.blocks(): without a setting (and under CV_BIN_PACK=host) the blocks are pack_array's, byte for byte; under
    CV_BIN_PACK=device X comes back the same through DecompressArray and, under CV_BIN_DECODE=device, through the
    device's strict decoder without one chunk handed to the host"""
    from clairvoyante_amd import utils_v2
    x = _synth(n)
    monkeypatch.setattr(utils_v2, "PACK_ROUTE", None)
    monkeypatch.delenv("CV_BIN_PACK", raising=False)
    plain = _training_set(x).blocks()
    want_x = [utils_v2.pack_array(np.ascontiguousarray(x[s:s + BS])) for s in range(0, n, BS)] + ([utils_v2.pack_array(np.array([]))] if n % BS == 0 else [])
    assert plain[0] == n and plain[1] == want_x
    monkeypatch.setenv("CV_BIN_PACK", "host")
    assert utils_v2.bin_pack_route() == "host"
    asked_host = _training_set(x).blocks()
    assert asked_host[1:] == plain[1:]
    monkeypatch.setenv("CV_BIN_PACK", "device")
    assert utils_v2.bin_pack_route() == "device"
    before = utils_v2.bin_pack_counts()
    ts = _training_set(x)
    packed = ts.blocks()
    after = utils_v2.bin_pack_counts()
    assert after["device"] - before["device"] == (n + BS - 1) // BS and after["host"] == before["host"] and ts.times["pack"] > 0
    assert packed[0] == n and packed[2] == plain[2] and packed[3] == plain[3] and len(packed[1]) == n // BS + 1
    assert packed[1] != plain[1]
    if n % BS == 0:
        assert packed[1][-1] == plain[1][-1]                    # the trailing empty block is the host's on both routes
    a, b = cases.arrays_of(packed), cases.arrays_of(plain)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
    got, num, end = utils_v2.DecompressArray(packed[1], 0, n, n)
    assert num == n and end == 1 and np.array_equal(np.asarray(got).view(np.uint32), x.view(np.uint32))
    monkeypatch.setenv("CV_BIN_DECODE", "device")
    assert utils_v2.bin_decode_route(packed[1], len(packed[1])) == "device"
    before = utils_v2.bin_decode_counts()
    got, num, end = utils_v2.DecompressArrayDevice(packed[1], 0, n, n)
    after = utils_v2.bin_decode_counts()
    assert after["host"] == before["host"] and after["device"] - before["device"] == (n + BS - 1) // BS
    assert num == n and np.array_equal(got.cpu().numpy().view(np.uint32), x.view(np.uint32))
    monkeypatch.setenv("CV_BIN_PACK", "elsewhere")
    with pytest.raises(Exception):
        utils_v2.bin_pack_route()


def test_size_condition():
    """make_candidates(2 000) at blocksize 65 536: the device route's X blocks total at most 1.5 times the host writer's"""
    import torch
    from clairvoyante_amd import utils_v2
    x = _synth(2000)
    blocks = utils_v2.pack_blocks_device(torch.from_numpy(x).cuda(), 65536)
    _decoded(blocks, x)
    mine = sum(len(b) for b in blocks)
    theirs = sum(len(utils_v2.pack_array(np.ascontiguousarray(x[s:s + BS]), 65536)) for s in range(0, 2000, BS))
    print("device route %d bytes, cv_blosc_compress_lz4_blocks %d: ratio %.3f" % (mine, theirs, mine / theirs))
    assert mine <= 1.5 * theirs


def _same_file(plain_fn, packed_fn):
    from clairvoyante_amd import utils_v2
    a, b = utils_v2.LoadBin(plain_fn), utils_v2.LoadBin(packed_fn)
    fa, fb = cases.arrays_of(a), cases.arrays_of(b)
    assert fa[:2] == fb[:2] and fa[0] > 0 and np.array_equal(fa[2], fb[2]) and np.array_equal(fa[3], fb[3]) and fa[4] == fb[4]
    # without the flag: what pack_array gives, as before
    x = fa[2].view(np.float32).reshape((-1,) + SHAPE)
    want = [utils_v2.pack_array(np.ascontiguousarray(x[s:s + BS])) for s in range(0, len(x) + 1, BS)]
    if len(x) % BS == 0:
        want[-1] = utils_v2.pack_array(np.array([]))
    assert [bytes(c) for c in a[1]] == want
    assert [bytes(c) for c in a[1]] != [bytes(c) for c in b[1]] and [bytes(c) for c in a[2]] == [bytes(c) for c in b[2]]
    return fa[0]


def test_tensor2bin_pack_device_from_text_tensors(tmp_path, monkeypatch):
    from clairvoyante_amd import tensor2Bin, utils_v2
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    monkeypatch.delenv("CV_BIN_PACK", raising=False)
    monkeypatch.setattr(utils_v2, "PACK_ROUTE", None)
    f = cases.write_case(str(tmp_path), "full")
    outs = [str(tmp_path / "plain.bin"), str(tmp_path / "packed.bin")]
    before = utils_v2.bin_pack_counts()
    for out, pack in zip(outs, (None, "device")):
        random.seed(cases.SEED)
        tensor2Bin.Run(types.SimpleNamespace(tensor_fn=f["bgzf"], var_fn=f["var"], bed_fn=f["bed"], bin_fn=out, pack=pack))
        if pack is None:
            assert utils_v2.bin_pack_counts() == before
    total = _same_file(*outs)
    after = utils_v2.bin_pack_counts()
    assert after["device"] - before["device"] == (total + BS - 1) // BS and after["host"] == before["host"]


def test_tensor2bin_pack_device_from_a_bam(tmp_path, monkeypatch):
    from clairvoyante_amd import tensor2Bin, utils_v2
    monkeypatch.delenv("CV_BIN_PACK", raising=False)
    monkeypatch.setattr(utils_v2, "PACK_ROUTE", None)
    d = str(tmp_path)
    a = bc.make_source(d, "a", "ctgA", 11)
    var_fn = bc.write_rows(os.path.join(d, "var.gz"), bc.truth_rows("ctgA", a["ref"], 3, 100))
    bed_fn = bc.write_rows(os.path.join(d, "bed.gz"), bc.bed_rows("ctgA", 6000, 900))
    cli = ["--bam_fn", a["sam"], "--ref_fn", a["fa"], "--ctgName", "ctgA", "--var_fn", var_fn, "--bed_fn", bed_fn, "--candidates",
           str(bc.CANDIDATES), "--genomeSize", str(bc.GENOME), "--seed", "77", "--samtools", bc.FAKE]
    outs = [str(tmp_path / "plain.bin"), str(tmp_path / "packed.bin")]
    before = utils_v2.bin_pack_counts()
    for out, extra in zip(outs, ([], ["--pack", "device"])):
        random.seed(5)
        tensor2Bin.Run(tensor2Bin.build_parser().parse_args(cli + ["--bin_fn", out] + extra))
    total = _same_file(*outs)
    after = utils_v2.bin_pack_counts()
    assert after["device"] - before["device"] == (total + BS - 1) // BS and after["host"] == before["host"]
