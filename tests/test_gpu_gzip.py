"""An ordinary gzip file (one DEFLATE stream, block starts unknown) inflated on the device: csrc/cv_gzip_dev.hip behind
utils_v2._gzip_slabs / GetTensorDevice / callVar.  The checker of the inflate is zlib, byte for byte; of the reader,
GetTensor over the plain file, bit for bit; of callVar, the plain file's VCF, byte for byte.  On the corpus NOTHING may go
to the host: the hand-over must not hide a finder or a decoder that only takes easy streams."""
import ctypes
import gzip
import os
import types
import zlib

import numpy as np
import pytest

import common
import gzip_cases as G
import textparse_cases as T

pytestmark = pytest.mark.gpu

CANARY = 0x5A


def _write(path, data):
    with open(str(path), "wb") as fh:
        fh.write(data)
    return str(path)


def device_inflate(fn, monkeypatch, spacing=4096, slab=None):
    """the file through utils_v2._gzip_slabs, the text of every slab copied back -> (text, device chunks, hand-overs,
    slabs the device inflated)"""
    from clairvoyante_amd import utils_v2
    monkeypatch.setenv("CV_GZIP_GUESS_BYTES", str(spacing))
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    gz = utils_v2._map_gzip(fn)
    assert gz is not None and not utils_v2.is_bgzf(fn)
    before = dict(utils_v2.gzip_chunk_counts)
    dev = utils_v2._TextSlabDevice("cuda", 64)
    parts, slabs = [], 0
    try:
        for item in utils_v2._gzip_slabs(fn, gz[0], gz[1], 300, dev):
            if isinstance(item, utils_v2._GzipText):
                slabs += 1
                item.up[2].synchronize()
                h = item.up[0][utils_v2.BGZF_HEADROOM:item.end].cpu().numpy().tobytes()
                if item.last:
                    assert h[-1:] == b"\n"
                    h = h[:-1]
                parts.append(h)
            else:
                parts.append(item.tobytes())
    finally:
        dev.close()
    grew = {k: utils_v2.gzip_chunk_counts[k] - before[k] for k in before}
    return b"".join(parts), grew["device"], grew["host"], slabs


def _host_text(text):
    """what the host reader's spans hold of a text: its last line gets a newline"""
    return text if not text or text.endswith(b"\n") else text + b"\n"


# ---- the kernels against zlib ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.kernel_corpus()))
def test_the_corpus_against_zlib(tmp_path, monkeypatch, name):
    data, text, may_fall_back = G.kernel_corpus()[name]
    got, device, host, _slabs = device_inflate(_write(tmp_path / "c.gz", data), monkeypatch)
    print("%s: %d device chunks, %d hand-overs" % (name, device, host))
    if may_fall_back:
        assert got == (text if host == 0 else _host_text(text))
    else:
        assert got == text
        assert host == 0 and device >= 3                     # a condition: no chunk of these files may go to the host


@pytest.mark.parametrize("name", ["level6_mem1", "level6_mem8", "level1_mem4"])
@pytest.mark.parametrize("slab", [4096, 65536])
def test_small_slabs_carry_bit_offset_and_window(tmp_path, monkeypatch, name, slab):
    data, text, _f = G.kernel_corpus()[name]
    got, device, host, slabs = device_inflate(_write(tmp_path / "c.gz", data), monkeypatch, spacing=1024, slab=slab)
    assert got == text and host == 0 and slabs >= 2 and device >= slabs


@pytest.mark.parametrize("name", sorted(G.unserved_corpus()))
def test_files_without_a_dynamic_block_go_to_the_host_whole(tmp_path, monkeypatch, name):
    data, text = G.unserved_corpus()[name]
    got, device, host, slabs = device_inflate(_write(tmp_path / "u.gz", data), monkeypatch)
    assert got == text and (device, host, slabs) == (0, 1, 0)


def test_decoy_headers_are_rejected_by_the_chain(tmp_path, monkeypatch):
    data, payload = G.decoy(T.volume_text(300))
    from clairvoyante_amd import _lib
    lib = _lib.load()
    a = np.frombuffer(data, dtype=np.uint8)
    at = data.index(payload[:64]) * 8                        # the inner stream's first header: a valid header, no block start
    assert lib.cv_gzip_header_at(ctypes.c_void_p(a.ctypes.data), len(a), at) == 1
    got, device, host, _slabs = device_inflate(_write(tmp_path / "d.gz", data), monkeypatch)
    print("decoy: %d device chunks, %d hand-overs" % (device, host))
    assert got == (payload if host == 0 else _host_text(payload))
    assert zlib.decompress(data, 31) == payload


def test_the_abi_touches_nothing_outside_what_a_row_states():
    """a writing pass with canaries around every chunk's symbols; rows that describe no chunk; null and negative
    arguments"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    data, text, _f = G.kernel_corpus()["level6_mem4"]
    first, n = G.header_end(data), len(data) - 8
    a = np.frombuffer(data, dtype=np.uint8)
    comp = torch.from_numpy(a.copy()).cuda()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    guesses = (n * 8 - first * 8 + 8 * 4096 - 1) // (8 * 4096)
    found = torch.full((guesses + 4,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.cv_gzip_find_dev(ptr(comp), n, first * 8, 4096, guesses, ptr(found), s))
    f = found.cpu().numpy()
    assert np.all(f[guesses:] == -7)
    want = [b for b in range(first * 8 + 1, first * 8 + 8 * 4096 * 3) if lib.cv_gzip_header_at(ctypes.c_void_p(a.ctypes.data), n, b)]
    for g in range(3):                                        # the finder against the host form of the header test
        inside = [b for b in want if first * 8 + g * 8 * 4096 <= b < first * 8 + (g + 1) * 8 * 4096]
        assert f[g] == (inside[0] if inside else -1)
    starts = np.concatenate(([first * 8], f[:guesses][f[:guesses] >= 0]))
    chunks = len(starts)
    rows = np.zeros((chunks + 3, 6), dtype=np.int64)
    rows[:chunks, 0], rows[:chunks, 1], rows[:chunks, 4] = starts, np.append(starts[1:], -1), 32768
    rows[0, 4] = 0
    rows[chunks] = (-5, -1, 0, 0, 0, 0)                      # no chunk: a negative start,
    rows[chunks + 1] = (n * 8 + 3, -1, 0, 0, 0, 0)          # one behind the data,
    rows[chunks + 2] = (starts[1], starts[0], 0, 0, 0, 0)   # an end in front of the start
    table = torch.from_numpy(rows).cuda()
    res = torch.zeros((chunks + 3, 4), dtype=torch.int64, device="cuda")
    _lib.check(lib.cv_gzip_decode_dev(ptr(comp), n, ptr(table), chunks + 3, None, 0, ptr(res), s))
    r = res.cpu().numpy()
    assert list(r[:chunks - 1, 2]) == [G.LANDED] * (chunks - 1) and r[chunks - 1, 2] == G.FINAL and list(r[chunks:, 2]) == [G.BAD] * 3
    assert np.array_equal(r[:chunks - 1, 1], starts[1:]) and int(r[:chunks, 0].sum()) == len(text)
    gap = 64
    off = np.concatenate(([0], np.cumsum(r[:chunks, 0] + gap)))[:chunks] + gap
    rows[:chunks, 2], rows[:chunks, 3] = off, r[:chunks, 0]
    rows[chunks:, 2], rows[chunks:, 3] = 0, 100
    rows[chunks + 2, 3] = -1
    cap = int(off[-1] + r[chunks - 1, 0] + gap)
    sym = torch.full((cap,), CANARY * 257, dtype=torch.int16, device="cuda")
    res2 = torch.zeros((chunks + 3, 4), dtype=torch.int64, device="cuda")
    _lib.check(lib.cv_gzip_decode_dev(ptr(comp), n, ptr(torch.from_numpy(rows).cuda()), chunks + 3, ptr(sym), cap, ptr(res2), s))
    h, r2 = sym.cpu().numpy().view(np.uint16), res2.cpu().numpy()
    assert np.array_equal(r2[:, :3], r[:, :3])
    out, at = b"", 0
    for k in range(chunks):
        lo, m = int(off[k]), int(r[k, 0])
        assert np.all(h[at:lo] == CANARY * 257)
        out += G.resolve(h[lo:lo + m], out[-32768:])
        at = lo + m
    assert np.all(h[at:] == CANARY * 257) and out == text
    # a row whose stated length is one short: BAD, and still nothing outside it
    rows[1, 3] -= 1
    sym.fill_(CANARY * 257)
    _lib.check(lib.cv_gzip_decode_dev(ptr(comp), n, ptr(torch.from_numpy(rows).cuda()), chunks, ptr(sym), cap, ptr(res2), s))
    h, r2 = sym.cpu().numpy().view(np.uint16), res2.cpu().numpy()
    assert r2[1, 2] == G.BAD and np.all(h[int(off[1]) + int(rows[1, 3]):int(off[2])] == CANARY * 257)
    p = ptr(sym)
    for args in ((None, 10, p, 1, None, 0, p, None), (p, -1, p, 1, None, 0, p, None), (p, 10, p, -1, None, 0, p, None),
                 (p, 10, ctypes.c_void_p(sym.data_ptr() + 2), 1, None, 0, p, None)):
        assert lib.cv_gzip_decode_dev(*args) != 0
    assert lib.cv_gzip_find_dev(p, 10, 0, 0, 1, p, None) != 0 and lib.cv_gzip_find_dev(None, 10, 0, 64, 1, p, None) != 0
    assert lib.cv_gzip_resolve_dev(p, p, 1, 5, 40000, p, p, None) != 0 and lib.cv_gzip_crc_dev(None, 5, p, None) != 0
    assert lib.cv_gzip_decode_dev(None, 0, None, 0, None, 0, None, None) == 0
    torch.cuda.synchronize()


# ---- damage ------------------------------------------------------------------------------------------------------------
def _outcome(batches):
    try:
        got = T.collect(batches)
        return ("rows", got[0].tobytes(), got[1])
    except Exception as e:                                    # noqa: the class is what is compared
        return ("raised", type(e))


@pytest.mark.parametrize("group", range(8))
def test_single_bit_flips_give_what_the_host_reader_gives(tmp_path, monkeypatch, group):
    from clairvoyante_amd import utils_v2
    monkeypatch.setenv("CV_GZIP_GUESS_BYTES", "4096")
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    data = G.deflate(T.volume_text(300), 6, 6)
    first, n = G.header_end(data), len(data) - 8
    rng = np.random.RandomState(77)
    bits = np.sort(rng.choice(np.arange(first * 8, n * 8), 200, replace=False))[group::8]
    same_rows = 0
    for bit in bits:
        b = bytearray(data); b[bit >> 3] ^= 1 << (bit & 7)
        fn = _write(tmp_path / "f.gz", bytes(b))
        want = _outcome(utils_v2.GetTensor(fn, 300, log=False))
        got = _outcome(utils_v2.GetTensorDevice(fn, 300, "cuda", log=False))
        assert got == want, "bit %d: %r against %r" % (bit, got[:2] if got[0] == "raised" else got[0], want[:2] if want[0] == "raised" else want[0])
        same_rows += got[0] == "rows"
    print("group %d: %d of %d flipped files still gave rows" % (group, same_rows, len(bits)))


def test_a_flipped_trailer_crc_raises_from_both_readers(tmp_path, monkeypatch):
    from clairvoyante_amd import _lib, utils_v2
    monkeypatch.setenv("CV_GZIP_GUESS_BYTES", "4096")
    data = bytearray(G.deflate(T.volume_text(300)))
    data[-6] ^= 0x10
    fn = _write(tmp_path / "t.gz", bytes(data))
    with pytest.raises(_lib.CvError):
        T.collect(utils_v2.GetTensor(fn, 300, log=False))
    with pytest.raises(_lib.CvError):
        T.collect(utils_v2.GetTensorDevice(fn, 300, "cuda", log=False))


# ---- the reader --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volume(tmp_path_factory):
    from clairvoyante_amd import utils_v2
    d = tmp_path_factory.mktemp("gzip_reader")
    text = T.volume_text(2000)
    out = {"plain": _write(d / "v.txt", text), "gzip6": _write(d / "v6.gz", G.deflate(text)), "mem4": _write(d / "v4.gz", G.deflate(text, 6, 4))}
    out["want"] = T.collect(utils_v2.GetTensor(out["plain"], 300, log=False))
    # (hundreds of slabs of a few blocks each: a shorter file keeps that case to a second or two)
    short = T.volume_text(500)
    out["short_mem4"] = _write(d / "s4.gz", G.deflate(short, 6, 4))
    out["short_want"] = T.collect(utils_v2.GetTensor(_write(d / "s.txt", short), 300, log=False))
    return out


def _same_batches(fn, want, num, monkeypatch, slab, spacing=4096, host_ok=False):
    from clairvoyante_amd import utils_v2
    monkeypatch.setenv("CV_GZIP_GUESS_BYTES", str(spacing))
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    before, members = dict(utils_v2.gzip_chunk_counts), dict(utils_v2.bgzf_member_counts)
    got = T.collect(utils_v2.GetTensorDevice(fn, num, "cuda", log=False))
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert got[2][-1] == 1 and not any(got[2][:-1])
    after = utils_v2.gzip_chunk_counts
    assert utils_v2.bgzf_member_counts == members
    if not host_ok:
        assert after["host"] == before["host"] and after["device"] > before["device"]
    return got


@pytest.mark.parametrize("form,slab", [("gzip6", None), ("gzip6", 4096), ("gzip6", 65536), ("mem4", None), ("mem4", 65536), ("short_mem4", 4096)])
def test_get_tensor_device_over_gzip(volume, monkeypatch, form, slab):
    got = _same_batches(volume[form], volume["short_want" if form == "short_mem4" else "want"], 300, monkeypatch, slab)
    assert sum(got[3]) == len(got[1]) > (400 if form == "short_mem4" else 1500)


@pytest.mark.parametrize("name", ["nonl", "off_format", "empty"])
def test_edge_files_over_gzip(tmp_path, monkeypatch, name):
    from clairvoyante_amd import utils_v2
    text = {"nonl": T.volume_text(2000)[:400000].rstrip(b"\n"), "off_format": T.off_format_text()[0], "empty": b""}[name]
    plain = _write(tmp_path / "e.txt", text)
    fn = _write(tmp_path / "e.gz", G.deflate(text, 6, 4))
    want = T.collect(utils_v2.GetTensor(plain, 50, log=False))
    for slab in (None, 4096):
        _same_batches(fn, want, 50, monkeypatch, slab, host_ok=name == "empty")


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tensors(tmp_path_factory):
    d = tmp_path_factory.mktemp("gzip_e2e")
    x = common.inputs(6000, seed=17)
    raw = x.copy()
    for i in range(1, 4):
        raw[:, :, :, i] += raw[:, :, :, 0]
    rng = np.random.RandomState(3)
    lines = []
    for j in range(raw.shape[0]):
        seq = "".join(rng.choice(list("ACGT"), 33))
        if j % 97 == 5:
            seq = seq[:16] + "N" + seq[17:]
        lines.append("%s %d %s %s" % ("chr%d" % (1 + j % 4), 10000 + 7 * j, seq, " ".join("%0.1f" % v for v in raw[j].reshape(-1))))
    text = ("\n".join(lines) + "\n").encode()
    out = {"plain": str(d / "t.txt"), "gz": str(d / "t.txt.gz"), "bgzf": str(d / "t.bgzf.gz"), "dir": str(d)}
    _write(out["plain"], text)
    with gzip.open(out["gz"], "wb") as fh:
        fh.write(text)
    from clairvoyante_amd import utils_v2
    with utils_v2.BgzfWriter(out["bgzf"]) as w:
        w.write(text)
    return out


@pytest.fixture(scope="module")
def checkpoints(oracle, tmp_path_factory):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    d = tmp_path_factory.mktemp("gzip_ckpt")
    out = {}
    for arch, mod in (("full", clairvoyante_v3), ("slim", clairvoyante_v3_slim)):
        m = mod.Clairvoyante(); m.setParameters(common.bench_params(oracle, arch))
        out[arch] = str(d / arch / "model"); m.saveParameters(out[arch]); m.close()
    return out


def _run(tensors, checkpoints, form, arch, show_ref, tag):
    from clairvoyante_amd import callVar
    out = os.path.join(tensors["dir"], "%s_%s_%d_%s.vcf" % (form, arch, show_ref, tag))
    a = types.SimpleNamespace(tensor_fn=tensors[form], chkpnt_fn=checkpoints[arch], call_fn=out, qual=30, sampleName="S", ref_fn=None,
                              threads=None, showRef=show_ref, v3=True, v2=False, slim=arch == "slim")
    callVar.Run(a)
    return open(out, "rb").read()


@pytest.mark.parametrize("arch", ["full", "slim"])
@pytest.mark.parametrize("show_ref", [False, True])
def test_callvar_gives_the_plain_files_vcf(tensors, checkpoints, arch, show_ref, monkeypatch):
    from clairvoyante_amd import utils_v2
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    monkeypatch.setenv("CV_GZIP_GUESS_BYTES", "4096")
    vcf = {}
    for form, side in (("plain", "host"), ("gz", "host"), ("gz", "device")):
        monkeypatch.setenv("CV_TEXT_PARSE", side)
        before = dict(utils_v2.gzip_chunk_counts)
        vcf[form, side] = _run(tensors, checkpoints, form, arch, show_ref, side)
        grew = {k: utils_v2.gzip_chunk_counts[k] - before[k] for k in before}
        if (form, side) == ("gz", "device"):
            assert grew["host"] == 0 and grew["device"] >= 10
        else:
            assert grew == {"device": 0, "host": 0}
    assert len([l for l in vcf["plain", "host"].splitlines() if not l.startswith(b"#")]) >= 200
    assert vcf["gz", "host"] == vcf["plain", "host"] and vcf["gz", "device"] == vcf["plain", "host"]


def test_the_input_chooses_the_reader(tensors, checkpoints, monkeypatch):
    from clairvoyante_amd import callVar, utils_v2
    monkeypatch.delenv("CV_TEXT_PARSE", raising=False)
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    assert callVar.GZIP_DEVICE_MIN_BYTES is None or callVar.GZIP_DEVICE_MIN_BYTES > 0
    size = os.path.getsize(tensors["gz"])
    for floor, side in ((size, "device"), (size + 1, "host")):        # a file at the threshold and one byte below it
        monkeypatch.setattr(callVar, "GZIP_DEVICE_MIN_BYTES", floor)
        before, chunks = dict(utils_v2.text_parse_counts), dict(utils_v2.gzip_chunk_counts)
        _run(tensors, checkpoints, "gz", "full", False, "rule_" + side)
        after = utils_v2.text_parse_counts
        assert after[side] == before[side] + 1 and sum(after.values()) == sum(before.values()) + 1
        assert (utils_v2.gzip_chunk_counts["device"] > chunks["device"]) == (side == "device")
        assert utils_v2.gzip_chunk_counts["host"] == chunks["host"]
    # a BGZF file still takes the BGZF route
    monkeypatch.setattr(callVar, "GZIP_DEVICE_MIN_BYTES", 1 << 60)
    monkeypatch.setattr(callVar, "BGZF_DEVICE_MIN_BYTES", 1)
    chunks, members = dict(utils_v2.gzip_chunk_counts), dict(utils_v2.bgzf_member_counts)
    _run(tensors, checkpoints, "bgzf", "full", False, "rule_bgzf")
    assert utils_v2.gzip_chunk_counts == chunks and utils_v2.bgzf_member_counts["device"] > members["device"]
