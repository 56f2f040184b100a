"""BGZF members compressed on the device (csrc/cv_bgzf_deflate_dev.hip, CV_BGZF_DEFLATE=device; opt-in).  The device's
bytes, sizes and counts equal cv_bgzf_deflate_host_form's (held to zlib's judgement and run under the sanitizers by
test_bgzf_deflate_core_host.py), with canaries behind every output and the workspace; then the writer and its two drivers:
MergeVcf and CreateTensor --bgzf write files whose inflated bytes, ISIZEs and index answers are the host route's, and the
device's own inflater reads what the device's compressor wrote.

bd_compress has 512 workgroups and loops over the members: test_multi_tile_members_past_the_workgroup_line gives it 589
members of 16 tiles and 515 of 255 tiles, text and random bytes in turn so that a workgroup's second member has the other
block type than its first (bgzf_deflate_cases.two_trip_text; test_bgzf_deflate_core_host.py holds the text to that).  With
the member loop cut to one trip, in a library built from a scratch copy, it fails: sizes[512] keeps its canary.
Seconds on one MI355X (pytest --durations): 0.27 at block 4 096, 0.71 at block 65 280 (33.6 MB, the host form's time);
the output too small for its members 0.01."""
import ctypes
import gzip
import io
import os
import sys
import types

import numpy as np
import pytest

import bgzf_deflate_cases as bc
import vcf_merge_cases as vc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = "%s %s" % (sys.executable, os.path.join(HERE, "golden", "fake_samtools.py"))
CANARY = 0x5A


class _Guarded(object):
    """`size` bytes on the device with 256 canary bytes on either side, the first at `phase` mod 256"""

    def __init__(self, torch, dev, size, phase=0, fill=None):
        self.size = size
        self.buf = torch.full((size + 1024,), CANARY, dtype=torch.uint8, device=dev)
        self.at = 256 + (phase - (self.buf.data_ptr() + 256)) % 256
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.at)
        if fill is not None and size:
            self.buf[self.at:self.at + size] = torch.from_numpy(np.frombuffer(fill, dtype=np.uint8).copy()).to(dev)

    def read(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.at] == CANARY).all() and (b[self.at + self.size:] == CANARY).all(), "a canary was overwritten"
        return b[self.at:self.at + self.size]


def dev_call(text, block, offset=0, ws_shift=0, ws_short=0, out_cap=None):
    """cv_bgzf_deflate_dev over `text` lying `offset` bytes behind a 256-byte boundary, everything guarded
    -> (file bytes without the EOF marker, sizes, info) like bc.host_form; with out_cap, the room the call is told the
    output has: the WHOLE output comes back, the canary where nothing was written"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    members = max(1, -(-len(text) // block))
    cap = members * (block + 31)
    src = _Guarded(torch, dev, len(text), offset, fill=text)
    out, sizes, info = _Guarded(torch, dev, cap), _Guarded(torch, dev, 4 * members), _Guarded(torch, dev, 64)
    need = _lib.workspace(lib.cv_bgzf_deflate_workspace, members, block)
    ws = _Guarded(torch, dev, need - ws_short, ws_shift)
    _lib.check(lib.cv_bgzf_deflate_dev(src.ptr if len(text) else None, len(text), block, out.ptr, cap if out_cap is None else out_cap,
                                       sizes.ptr, info.ptr, ws.ptr, need - ws_short, _lib.stream_arg(dev)))
    torch.cuda.synchronize()
    ws.read()
    assert src.read().tobytes() == text
    i, s = info.read().view(np.int64).copy(), sizes.read().view(np.int32).copy()
    return (out.read()[:int(i[0])] if out_cap is None else out.read()).tobytes(), s, i


def same(text, block, offset=0):
    got, want = dev_call(text, block, offset), bc.host_form(text, block)
    assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    assert got[0] == want[0]
    return got


def test_single_members_equal_the_host_form():
    text = bc.fixture("tensor_rows")
    for n in (0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 258, 259, 260, 4095, 4096, 65279, 65280):
        data, sizes, info = same(text[:n], 65280)
        assert len(sizes) == 1 and info[1] == 1
        if n in (0, 65, 65280):
            bc.judge(data, sizes, text[:n], 65280)


@pytest.mark.parametrize("name,text", bc.special_texts(), ids=[n for n, _t in bc.special_texts()])
def test_the_special_texts_equal_the_host_form(name, text):
    _data, _sizes, info = same(text, 65280)
    assert info[2:5].sum() == 1 and (name != "random" or info[2] == 1) and (name != "no match" or info[4] == 1)


@pytest.mark.parametrize("block", (1000, 65280))
@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_the_fixtures_equal_the_host_form(name, block):
    text = bc.fixture(name)
    assert len(text) % block                                     # a partial last member
    data, sizes, info = same(text, block)
    assert info[1] == len(sizes) == -(-len(text) // block) and info[4] > 0
    bc.judge(data, sizes, text, block)


def test_more_members_than_workgroups():
    text = (bc.fixture("vcf_records") * 3)[:5000 * 64 - 17]
    data, sizes, info = same(text, 64)
    assert len(sizes) == 5000 == info[1] and info[2:5].sum() == 5000


@pytest.mark.parametrize("members,block", bc.TWO_TRIPS)
def test_multi_tile_members_past_the_workgroup_line(members, block):
    """more members than bd_compress has workgroups, of 16 and of 255 tiles: a workgroup's second member reads a hash
    table, verdicts and an LDS state its first one filled tile after tile, and follows a stored member with a dynamic one
    or the other way round (tests/test_bgzf_deflate_core_host.py holds the text to that)"""
    text = bc.two_trip_text(members, block)
    data, sizes, info = same(text, block)
    assert len(sizes) == members == info[1] > bc.WORKGROUPS and info[2] > 0 and info[4] > 0 and info[2:5].sum() == members
    kinds = bc.member_kinds(data, sizes)
    assert all(kinds[m] != kinds[m + bc.WORKGROUPS] for m in range(members - bc.WORKGROUPS))
    if block == 4096:
        assert bc.judge(data, sizes, text, block) == kinds


def test_an_output_too_small_for_its_members():
    """bd_assemble skips a member that does not fit below out_cap; info[0] still names what all of them need"""
    text = bc.fixture("vcf_records")[:9 * 1000 + 123]
    full, sizes, info = dev_call(text, 1000)
    off = np.concatenate(([0], np.cumsum(sizes)))
    assert len(sizes) == 10 and info[0] == len(full) == off[-1]
    for cap, fit in bc.small_output_caps(sizes):
        got, want = dev_call(text, 1000, out_cap=cap), bc.host_form(text, 1000, out_cap=cap, fill=CANARY)
        assert got[1].tolist() == want[1].tolist() == sizes.tolist() and got[2].tolist() == want[2].tolist() == info.tolist(), cap
        assert got[0] == want[0], cap
        edge = int(off[fit])
        assert edge <= cap and (fit == len(sizes) or off[fit + 1] > cap)
        assert got[0][:edge] == full[:edge] and got[0][edge:] == bytes([CANARY]) * (len(got[0]) - edge), cap


@pytest.mark.parametrize("offset", (1, 7, 15))
def test_a_text_at_any_alignment(offset):
    text = bc.fixture("candidate_list")[:70000]
    same(text, 65280, offset)
    same(text[:3001], 1000, offset)


def test_workspaces_and_arguments_are_refused_with_a_message():
    from clairvoyante_amd import _lib
    text = bc.fixture("vcf_records")[:5000]
    with pytest.raises(_lib.CvError, match="workspace holds"):
        dev_call(text, 1000, ws_short=1)
    with pytest.raises(_lib.CvError, match="256-byte aligned"):
        dev_call(text, 1000, ws_shift=8)
    with pytest.raises(_lib.CvError, match="out of range"):
        dev_call(text, 65281)


# ---- the writer ----------------------------------------------------------------------------------------------------------------
def test_write_device_pieces_straddle_the_cuts():
    import torch
    from clairvoyante_amd import utils_v2
    text = bc.fixture("tensor_rows")[:40 * 1000 + 77]
    block = 1000
    one = io.BytesIO()
    utils_v2.bgzf_deflate_counts(reset=True)
    with utils_v2.BgzfWriter(one, block=block, deflate="device") as w1:
        assert w1.deflate == "device"
        w1.write(text)
    c = utils_v2.bgzf_deflate_counts()
    assert c["device"] == 41 and c["host"] == 0 and c["uploaded"] == len(text) and c["downloaded"] == len(one.getvalue()) - 28
    data, sizes, _info = bc.host_form(text, block)
    assert one.getvalue() == data + utils_v2.BgzfWriter.EOF and w1.member_sizes == sizes.tolist()
    whole = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    for step in (1, block - 1, block + 1, 3 * block + 7):
        n = 3 * block + 5 if step == 1 else len(text)
        want = bc.host_form(text[:n], block)[0] + utils_v2.BgzfWriter.EOF
        for every in (1, 2):                                     # write_device alone, and mixed with write
            fh = io.BytesIO()
            utils_v2.bgzf_deflate_counts(reset=True)
            with utils_v2.BgzfWriter(fh, block=block, deflate="device") as w:
                for k, at in enumerate(range(0, n, step)):
                    if k % every == 0:
                        w.write_device(whole[at:min(at + step, n)])
                    else:
                        w.write(text[at:min(at + step, n)])
            assert fh.getvalue() == want, (step, every)
            c = utils_v2.bgzf_deflate_counts()
            assert c["device"] == -(-n // block) and c["host"] == 0 and (c["uploaded"] == 0) == (every == 1)


def test_a_slab_and_a_reused_buffer(monkeypatch):
    """more than a slab in one call, and a caller that overwrites its buffer between calls"""
    import torch
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2.BgzfWriter, "SLAB_MEMBERS", 8)
    text = bc.fixture("vcf_records")[:30 * 1000 + 1]
    fh = io.BytesIO()
    buf = torch.zeros(7001, dtype=torch.uint8, device="cuda")
    with utils_v2.BgzfWriter(fh, block=1000, deflate="device") as w:
        for at in range(0, len(text), 7001):
            piece = text[at:at + 7001]
            buf[:len(piece)] = torch.from_numpy(np.frombuffer(piece, dtype=np.uint8).copy()).cuda()
            w.write_device(buf[:len(piece)])
            buf.fill_(0)
    assert fh.getvalue() == bc.host_form(text, 1000)[0] + utils_v2.BgzfWriter.EOF


# ---- MergeVcf ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", (1000, None))
def test_mergevcf_with_the_device_writer(block, tmp_path, monkeypatch):
    from test_vcf_merge_host import _brute, _regions
    from clairvoyante_amd import utils_v2, vcf_merge
    files, fai, per = vc.build(tmp_path, 2000)
    out = {}
    for route in ("host", "device"):
        monkeypatch.setenv("CV_VCF_MERGE", route)
        monkeypatch.setenv("CV_BGZF_DEFLATE", route)
        fn = str(tmp_path / ("%s.vcf.gz" % route))
        vcf_merge.counts(reset=True)
        utils_v2.bgzf_deflate_counts(reset=True)
        vcf_merge.merge(files, fn, fai_fn=fai, block=block, threads=4)
        out[route] = (fn, vcf_merge.counts(), utils_v2.bgzf_deflate_counts())
    raw = {r: open(out[r][0], "rb").read() for r in out}
    text = gzip.decompress(raw["host"])
    assert gzip.decompress(raw["device"]) == text == vc.HEADER + b"".join(vc.expected_order(per))
    th, td = (utils_v2.bgzf_scan(np.frombuffer(raw[r], dtype=np.uint8))[0] for r in ("host", "device"))
    assert (td[:, 3] >> 32).tolist() == (th[:, 3] >> 32).tolist()                 # the same cuts
    c = out["device"][1]
    assert (c["device_calls"], c["host_calls"], c["handed_over_calls"]) == (1, 0, 0)
    members = len(td) - 1 if (td[-1, 3] >> 32) == 0 else len(td)
    d, h = out["device"][2], out["host"][2]
    assert d["device"] == members > 0 and d["host"] > 0 and h["device"] == 0      # (the device route's "host" members: the .tbi's)
    assert d["host"] == h["host"] - members and d["uploaded"] == len(vc.HEADER)
    # the .tbi names the device writer's compressed offsets: every region through it is the brute-force filter's answer
    lines = vc.expected_order(per)
    idx = {r: vcf_merge.TabixIndex.read(out[r][0] + ".tbi") for r in out}
    hits = 0
    for ctg, b, e in _regions(lines):
        got = list(vcf_merge.fetch(out["device"][0], ctg, b, e, index=idx["device"]))
        assert got == _brute(lines, ctg, b, e) == list(vcf_merge.fetch(out["host"][0], ctg, b, e, index=idx["host"])), (ctg, b, e)
        hits += len(got)
    assert hits > 1000


# ---- CreateTensor --bgzf, and callVar over the file ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pileup_inputs(tmp_path_factory):
    from clairvoyante_amd import synth_pileup
    d = tmp_path_factory.mktemp("bgzf_deflate_ct")
    ref, sam = synth_pileup.fast_alignments(4000, 30000, read_len=150, seed=5, ctg="ctgA")
    base = str(d / "synth")
    with open(base + ".fa", "w") as fh:
        fh.write(">ctgA\n")
        s = ref.decode()
        fh.write("\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    with open(base + ".fa.fai", "w") as fh:
        fh.write("ctgA\t%d\t6\t60\t61\n" % len(ref))
    with open(base + ".sam", "wb") as fh:
        fh.write(sam)
    with open(base + ".can", "w") as fh:
        fh.write("\n".join(synth_pileup.candidate_rows("ctgA", list(range(200, 29800, 9)))) + "\n")
    return base


def run_ct(monkeypatch, base, out, rows_side, deflate):
    from clairvoyante_amd import CreateTensor, pileup, utils_v2
    monkeypatch.setenv("CV_ROW_FORMAT", rows_side)
    monkeypatch.setenv("CV_BGZF_DEFLATE", deflate)
    a = types.SimpleNamespace(bam_fn=base + ".sam", ref_fn=base + ".fa", can_fn=base + ".can", tensor_fn=out, minMQ=0, ctgName="ctgA",
                              ctgStart=None, ctgEnd=None, samtools=FAKE, dcov=250, minCoverage=0, considerleftedge=True, bgzf=True)
    pileup.row_format_counts(reset=True)
    utils_v2.bgzf_deflate_counts(reset=True)
    res = CreateTensor.OutputAlnTensor(a)
    return len(res["centers"]), pileup.row_format_counts(), utils_v2.bgzf_deflate_counts()


def test_createtensor_bgzf_and_callvar_over_the_file(pileup_inputs, tmp_path, monkeypatch, oracle):
    sys.path.insert(0, HERE)
    from clairvoyante_amd import callVar, clairvoyante_v3, utils_v2
    from common import bench_params
    fn = {side: str(tmp_path / (side + ".bgzf.gz")) for side in ("host", "device")}
    rows, rc, dc = run_ct(monkeypatch, pileup_inputs, fn["host"], "host", "host")
    assert rows > 2000 and rc == {"host": rows, "device": 0} and dc["device"] == 0 and dc["host"] > 0
    rows_d, rc, dc = run_ct(monkeypatch, pileup_inputs, fn["device"], "device", "device")
    assert rows_d == rows and rc == {"host": 0, "device": rows}
    text = gzip.open(fn["host"], "rb").read()
    assert text.count(b"\n") == rows and gzip.open(fn["device"], "rb").read() == text
    assert dc["device"] == -(-len(text) // 65280) and dc["host"] == 0 and dc["uploaded"] == 0      # the text never crossed
    assert dc["downloaded"] == os.path.getsize(fn["device"]) - 28
    # a batch the host formatter takes goes through write: the same file
    mixed = str(tmp_path / "mixed.bgzf.gz")
    _rows, rc, dc = run_ct(monkeypatch, pileup_inputs, mixed, "host", "device")
    assert rc["host"] == rows and dc["device"] > 0 and dc["uploaded"] == len(text)
    assert open(mixed, "rb").read() == open(fn["device"], "rb").read()
    m = clairvoyante_v3.Clairvoyante()
    m.init()
    m.setParameters(bench_params(oracle, "full", seed=11))
    chk = str(tmp_path / "model-000001")
    m.saveParameters(chk)
    m.close()
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    vcf = {}
    for side in ("host", "device"):
        v = types.SimpleNamespace(tensor_fn=fn[side], chkpnt_fn=chk, call_fn=str(tmp_path / (side + ".vcf")), qual=None,
                                  sampleName="SAMPLE", ref_fn=pileup_inputs + ".fa", threads=None, showRef=False, v3=True,
                                  v2=False, slim=False)
        before = dict(utils_v2.bgzf_member_counts)
        callVar.Run(v)
        grew = {k: utils_v2.bgzf_member_counts[k] - before[k] for k in before}
        assert grew["host"] == 0 and grew["device"] >= -(-len(text) // 65280), (side, grew)   # the device's inflater takes them all
        vcf[side] = open(v.call_fn).read()
    assert vcf["device"] == vcf["host"] and len([l for l in vcf["host"].splitlines() if not l.startswith("#")]) > 100
