"""BGZF members inflated on the device (csrc/cv_inflate_dev.hip), the token hand-back (cv_text_gather_tokens) and
callVar over BGZF tensor files.  The checker of the inflate is zlib, bit for bit; of callVar, the host reader's VCF, byte
for byte.  On the corpus NO member may come back HOST: the host fallback must not hide a decoder that only takes easy
streams.  The damaged members are the first few hundred of the seeded set tests/test_bgzf_sanitized.py runs through the
same decode core under AddressSanitizer; they are given to the device once."""
import ctypes
import gzip
import os
import types
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import common
import textparse_cases as T

pytestmark = pytest.mark.gpu

CANARY, GAP = 0xC7, 96


def device_inflate(members, offset=0):
    """members [(data, isize, crc)] through cv_inflate_bgzf_dev in ONE call, the compressed data back to back with 3
    bytes between, the outputs with GAP canary bytes in front of, between and behind them, everything `offset` bytes
    into its buffer -> (status [m], [output bytes], canaries intact)"""
    import torch
    from clairvoyante_amd import _lib
    m = len(members)
    table = np.zeros((m, 4), dtype=np.int64)
    comp, at, out_at = bytearray(), 0, 0
    for i, (data, isize, crc) in enumerate(members):
        table[i] = (1000 + at, len(data), 5000 + out_at, (isize << 32) | crc)     # (only differences to row 0 count)
        comp += data + b"\xee\xee\xee"; at += len(data) + 3
        out_at += isize + GAP
    cap = out_at
    text = torch.full((offset + GAP + cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    comp_dev = torch.zeros(offset + len(comp) + 64, dtype=torch.uint8, device="cuda")
    comp_dev[offset:offset + len(comp)] = torch.frombuffer(comp, dtype=torch.uint8).cuda()
    table_dev = torch.from_numpy(table).cuda()
    status = torch.zeros(m, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().cv_inflate_bgzf_dev(
        ctypes.c_void_p(comp_dev.data_ptr() + offset), ctypes.c_void_p(table_dev.data_ptr()), m,
        ctypes.c_void_p(text.data_ptr() + offset + GAP), cap, ctypes.c_void_p(status.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host, status = text.cpu().numpy(), status.cpu().numpy()
    outs, canaries, p = [], [host[:offset + GAP]], offset + GAP
    for _data, isize, _crc in members:
        outs.append(host[p:p + isize].tobytes()); p += isize
        canaries.append(host[p:p + GAP]); p += GAP
    canaries.append(host[p:])
    return status, outs, all(np.all(c == CANARY) for c in canaries)


@pytest.mark.parametrize("offset", [0, 5])
def test_the_corpus_against_zlib_and_no_member_goes_to_the_host(offset):
    corpus = B.corpus() + B.small_corpus()
    status, outs, intact = device_inflate([(data, len(raw), zlib.crc32(raw)) for _n, data, raw in corpus], offset)
    assert intact
    for (name, _data, raw), s, o in zip(corpus, status, outs):
        assert s == B.OK, "%s came back %d" % (name, s)
        assert o == raw, name


def test_many_members_in_one_call():
    """more members than the grid has waves: text-tensor rows in members of every size up to 65 280"""
    text = T.volume_text()
    rng = np.random.RandomState(5)
    members, at = [], 0
    while len(members) < 17500:                              # (the grid is 4096 workgroups of 4 waves)
        n = int(rng.choice([0, 1, 300, 700, 2000, 65280], p=[0.05, 0.05, 0.4, 0.3, 0.19, 0.01]))
        raw = text[at:at + n]; at += n
        members.append((B.deflate(raw, int(rng.choice([1, 6]))), len(raw), zlib.crc32(raw), raw))
    assert at < len(text)
    status, outs, intact = device_inflate([m[:3] for m in members])
    assert intact and np.all(status == B.OK)
    assert all(o == m[3] for o, m in zip(outs, members))


def test_damaged_members_are_handed_back_or_right():
    members = list(B.mutations(400, seed=1234))
    status, outs, intact = device_inflate(members)
    assert intact
    assert set(np.unique(status)) <= {B.OK, B.HOST}
    accepted = 0
    for k, ((data, isize, crc), s, o) in enumerate(zip(members, status, outs)):
        if s == B.OK:
            accepted += 1
            assert o == B.zlib_verdict(data, isize, crc), "mutation %d" % k
    print("400 damaged members: %d accepted" % accepted)
    assert accepted < 200


def test_rows_that_describe_no_member_are_not_touched():
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    raw = T.volume_text(2000)[:3000]
    data = B.deflate(raw)
    good = (data, len(raw), zlib.crc32(raw))
    status, outs, intact = device_inflate([good, (data, 70000, 0), good])        # ISIZE above 64 KiB (its range stays canary)
    assert list(status) == [B.OK, B.HOST, B.OK] and outs[0] == raw and outs[2] == raw
    assert set(outs[1]) == {CANARY} and intact
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    for args, word in (((None, p, 1, p, 10, p, None), "null"), ((p, p, -1, p, 10, p, None), "negative"), ((p, p, 1, p, -1, p, None), "negative"),
                       ((p, ctypes.c_void_p(buf.data_ptr() + 1), 1, p, 10, p, None), "aligned")):
        assert lib.cv_inflate_bgzf_dev(*args) != 0 and word in lib.cv_last_error().decode()
    assert lib.cv_inflate_bgzf_dev(None, None, 0, None, 0, None, None) == 0
    assert lib.cv_text_gather_tokens(None, p, p, 3, p, 10, p, None) != 0 and lib.cv_text_gather_tokens(p, p, p, -1, p, 10, p, None) != 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


def test_gather_tokens_against_the_host_meta():
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    text = T.volume_text(3000, seed=8)
    _c, _bad, _x, meta = T.host_parse(text)
    rng = np.random.RandomState(2)
    for keep in (np.arange(len(meta)), np.sort(rng.choice(len(meta), 1500, replace=False)), np.array([7]), np.array([5, 5, 2])):
        total = int(meta[keep][:, 1::2].sum())
        k = len(keep)
        text_dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        meta_dev, keep_dev = torch.from_numpy(meta).cuda(), torch.from_numpy(keep.astype(np.int64)).cuda()
        out = torch.full((k * 48 + total + 16,), CANARY, dtype=torch.uint8, device="cuda")
        _lib.check(lib.cv_text_gather_tokens(
            ctypes.c_void_p(text_dev.data_ptr()), ctypes.c_void_p(meta_dev.data_ptr()), ctypes.c_void_p(keep_dev.data_ptr()), k,
            ctypes.c_void_p(out.data_ptr() + k * 48), total, ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        got_meta, got = h[:k * 48].view(np.int64).reshape(k, 6), h[k * 48:k * 48 + total].tobytes()
        assert np.all(h[k * 48 + total:] == CANARY)
        assert np.array_equal(got_meta[:, 1::2], meta[keep][:, 1::2])
        assert got_meta[0, 0] == 0 and np.array_equal(got_meta[:, 0::2].reshape(-1)[1:], np.cumsum(got_meta[:, 1::2].reshape(-1))[:-1])
        for g, m in zip(got_meta, meta[keep]):
            for t in range(3):
                assert got[g[2 * t]:g[2 * t] + g[2 * t + 1]] == text[m[2 * t]:m[2 * t] + m[2 * t + 1]]


# ---- the reader --------------------------------------------------------------------------------------------------------
def _write(path, data):
    with open(str(path), "wb") as fh:
        fh.write(data)
    return str(path)


def _same_batches(fn, plain, num, monkeypatch, slab=None):
    from clairvoyante_amd import utils_v2
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    want = T.collect(utils_v2.GetTensor(plain, num, log=False))
    before = dict(utils_v2.bgzf_member_counts)
    got = T.collect(utils_v2.GetTensorDevice(fn, num, "cuda", log=False))
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert got[2][-1] == 1 and not any(got[2][:-1])
    after = utils_v2.bgzf_member_counts
    assert after["host"] == before["host"] and after["device"] > before["device"]
    return got


@pytest.mark.parametrize("block,slab", [(65280, None), (65280, 65536), (5000, 4096), (700, 1 << 20)])
def test_get_tensor_device_over_bgzf(tmp_path, monkeypatch, block, slab):
    text = T.volume_text(2000)
    plain = _write(tmp_path / "v.txt", text)
    fn = _write(tmp_path / "v.gz", B.bgzf_file(text, block=block, level=1))
    got = _same_batches(fn, plain, 300, monkeypatch, slab)
    assert sum(got[3]) == len(got[1]) > 1500


@pytest.mark.parametrize("name", ["nonl", "off_format", "empty"])
def test_edge_files_over_bgzf(tmp_path, monkeypatch, name):
    text = {"nonl": T.volume_text(2000)[:400000].rstrip(b"\n"), "off_format": T.off_format_text()[0], "empty": b""}[name]
    plain = _write(tmp_path / "e.txt", text)
    fn = _write(tmp_path / "e.gz", B.bgzf_file(text, block=3000 if name == "off_format" else 65280))
    for slab in (None, 4096):
        _same_batches(fn, plain, 50, monkeypatch, slab)


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tensors(tmp_path_factory):
    from clairvoyante_amd import utils_v2
    d = tmp_path_factory.mktemp("bgzf_e2e")
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
    # (off-format lines in ASCII only: a VCF record with other bytes in its contig name is callVar's error with any reader)
    off = b"".join(l + b"\n" for l, _s in T.off_format_lines() if all(0 < c < 128 for c in l))
    mixed = text[:len(text) // 2] + off + text[len(text) // 2:]
    out = {"plain": str(d / "t.txt"), "gz": str(d / "t.txt.gz"), "bgzf": str(d / "t.bgzf.gz"), "mixed_plain": str(d / "m.txt"),
           "mixed": str(d / "m.bgzf.gz"), "corrupt": str(d / "c.bgzf.gz"), "dir": str(d)}
    _write(out["plain"], text)
    _write(out["mixed_plain"], mixed)
    with gzip.open(out["gz"], "wb") as fh:
        fh.write(text)
    for key, body in (("bgzf", text), ("mixed", mixed)):
        with utils_v2.BgzfWriter(out[key]) as w:
            w.write(body)
    data = bytearray(open(out["bgzf"], "rb").read())
    members = B.walk(bytes(data))
    mid = members[len(members) // 2]
    data[mid[0] + mid[1] // 2] ^= 0x04                       # one flipped bit inside the DEFLATE data of a member in mid-file
    _write(out["corrupt"], bytes(data))
    assert utils_v2.is_bgzf(out["corrupt"]) and len(members) > 100
    return out


@pytest.fixture(scope="module")
def checkpoints(oracle, tmp_path_factory):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    d = tmp_path_factory.mktemp("bgzf_ckpt")
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
def test_callvar_gives_the_same_vcf_from_every_form(tensors, checkpoints, arch, show_ref, monkeypatch):
    from clairvoyante_amd import utils_v2
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    vcf = {}
    for form, side in (("plain", "host"), ("gz", "host"), ("bgzf", "host"), ("bgzf", "device"), ("plain", "device"), ("gz", "device")):
        monkeypatch.setenv("CV_TEXT_PARSE", side)
        before = dict(utils_v2.bgzf_member_counts)
        vcf[form, side] = _run(tensors, checkpoints, form, arch, show_ref, side)
        grew = {k: utils_v2.bgzf_member_counts[k] - before[k] for k in before}
        if (form, side) == ("bgzf", "device"):
            assert grew["host"] == 0 and grew["device"] > 100        # every member was inflated on the device
        else:
            assert grew == {"device": 0, "host": 0}
    records = [l for l in vcf["plain", "host"].splitlines() if not l.startswith(b"#")]
    assert len(records) >= 200
    for key, text in vcf.items():
        assert text == vcf["plain", "host"], key


@pytest.mark.parametrize("form", ["bgzf", "mixed"])
def test_callvar_with_small_slabs_and_off_format_lines(tensors, checkpoints, form, monkeypatch):
    from clairvoyante_amd import utils_v2
    vcf = {}
    for side, slab in (("host", None), ("device", None), ("device", 4096)):
        monkeypatch.setenv("CV_TEXT_PARSE", side)
        if slab is None:
            monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
        else:
            monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
        before = dict(utils_v2.bgzf_member_counts)
        vcf[side, slab] = _run(tensors, checkpoints, form, "full", True, "%s_%s" % (side, slab))
        if side == "device":
            assert utils_v2.bgzf_member_counts["host"] == before["host"] and utils_v2.bgzf_member_counts["device"] > before["device"]
    plain = "mixed_plain" if form == "mixed" else "plain"
    monkeypatch.setenv("CV_TEXT_PARSE", "host")
    assert vcf["host", None] == _run(tensors, checkpoints, plain, "full", True, "ref")
    assert vcf["device", None] == vcf["host", None] and vcf["device", 4096] == vcf["host", None]


def test_a_corrupted_member_raises_from_both_readers(tensors, checkpoints, monkeypatch):
    from clairvoyante_amd import _lib
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    for side in ("host", "device"):
        monkeypatch.setenv("CV_TEXT_PARSE", side)
        with pytest.raises(_lib.CvError):
            _run(tensors, checkpoints, "corrupt", "full", False, "corrupt_" + side)


def test_the_input_chooses_the_reader(tensors, checkpoints, monkeypatch):
    from clairvoyante_amd import callVar, utils_v2
    monkeypatch.delenv("CV_TEXT_PARSE", raising=False)
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    size = os.path.getsize(tensors["bgzf"])
    for floor, side in ((size, "device"), (size + 1, "host")):        # a file at the threshold and one byte below it
        monkeypatch.setattr(callVar, "BGZF_DEVICE_MIN_BYTES", floor)
        before, members = dict(utils_v2.text_parse_counts), dict(utils_v2.bgzf_member_counts)
        _run(tensors, checkpoints, "bgzf", "full", False, "rule_" + side)
        after = utils_v2.text_parse_counts
        assert after[side] == before[side] + 1 and sum(after.values()) == sum(before.values()) + 1
        assert (utils_v2.bgzf_member_counts["device"] > members["device"]) == (side == "device")
