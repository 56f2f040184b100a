"""callVarBam's row selection and candidate tokens made on the device (csrc/cv_callcols_dev.hip through
pileup.Pileup.call_columns and the C ABI) against the Python definition -- the filter of callVarBam.region_tensors plus
utils_v2.PosBatch.from_columns (call_columns_cases.definition): index, meta and text are equal, byte for byte.  Through the
drivers: callVarBam.Run under CV_CALL_COLUMNS=host and =device, crossed with CV_VCF_FORMAT, writes byte-identical VCF
files, the device takes every region, and callVar.CallFromDevice reads a DevicePosBatch where it lies."""
import ctypes
import io
import os
import shutil
import sys
import types

import numpy as np
import pytest

import common
from call_columns_cases import definition
from test_pileup_oracle import G, load_case

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
FAKE = "%s %s" % (sys.executable, os.path.join(HERE, "golden", "fake_samtools.py"))
LONG_NAME = "contig_0001.2|arrow_pilon|quiver.polished_x"
CANARY = 256


# ---- a reference of 300 bases by hand -------------------------------------------------------------------------------------
def handmade_reference():
    """300 bytes of ACGT with, at chosen 1-based positions, lower case, N / n, IUPAC letters and bytes >= 0x80: at centres
    (1, 9, 10, 16, 17, 18, 99, 100, the last 17 positions) and inside the windows of their neighbours"""
    rng = np.random.default_rng(7)
    ref = bytearray(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300)].tobytes())
    plant = {1: "a", 9: "n", 10: "N", 16: "c", 17: "g", 18: "R", 25: "t", 30: 0x80, 31: 0xFF, 40: "t", 41: "y", 60: "a", 61: "c",
             99: "N", 100: "a", 101: "g", 120: 0xE9, 121: "K", 150: "m", 151: "t", 210: "S", 211: "w", 230: 0xB5, 260: "c",
             284: "n", 285: "a", 288: "T", 290: "t", 293: "B", 296: 0x9C, 297: "c", 299: "N", 300: "g"}
    for p, b in plant.items():
        ref[p - 1] = b if isinstance(b, int) else ord(b)
    return bytes(ref)


def handmade_reads(ref, first0):
    """five reads: the centres 117 .. 183 and their like stay out of reach"""
    clean = bytes(b if b in b"ACGT" else ord("A") for b in ref.upper()).decode()
    lines = []
    for k, (start, length) in enumerate(((1, 60), (20, 50), (85, 16), (200, 60), (255, 46))):
        lines.append("r%d\t0\tctgA\t%d\t60\t%dM\t*\t0\t0\t%s\t*" % (k, first0 + start, length, clean[start - 1:start - 1 + length]))
    return ("\n".join(lines) + "\n").encode()


def device_columns(ref, first0, centres, sam, ctg, mask=None):
    """Pileup.call_columns behind finish() -> (the centres, touched as the definition gets it, index, the batch)"""
    import torch
    from clairvoyante_amd.pileup import Pileup
    pl = Pileup()
    pl.set_reference(ref, first0)
    pl.set_candidates(centres)
    if sam:
        pl.add_sam(sam, final=True)
    t, _d, touched = pl.finish(subtract=True)
    if mask is not None:
        touched = touched & torch.from_numpy(mask).to(touched.device)
    index, pos = pl.call_columns(touched, ctg)
    out = pl.centers.copy(), touched.cpu().numpy(), index, pos, t
    pl.close()
    return out


def assert_is_the_definition(ctg, centres, touched, ref, first0, index, pos):
    from clairvoyante_amd.utils_v2 import DevicePosBatch
    windex, wtext, wmeta = definition(ctg, centres, touched, ref, first0)
    assert isinstance(pos, DevicePosBatch) and not pos.fetched
    assert str(index.dtype) == "torch.int64" and index.is_cuda and np.array_equal(index.cpu().numpy(), windex)
    assert len(pos) == len(windex)
    # where the device VCF route reads them
    assert pos.device["keep"] is None and not pos.device["merged"] and pos.device["longest"] == len(ctg)
    assert pos.device["text_ptr"] == pos.text_dev.data_ptr() and pos.device["meta_ptr"] == pos.meta_dev.data_ptr()
    assert np.array_equal(pos.meta_dev.cpu().numpy(), wmeta) and pos.text_dev.cpu().numpy().tobytes() == wtext
    assert not pos.fetched
    # the host copy, fetched on the first read
    (start, rows, buf, meta), = pos.pieces()
    assert pos.fetched and (start, rows) == (0, len(windex))
    assert np.array_equal(meta, wmeta) and bytes(buf) == wtext
    return windex, wtext, wmeta


@pytest.mark.parametrize("ctg", ["c", LONG_NAME])
@pytest.mark.parametrize("first0", [0, 900, 999999850, 2100000000])
def test_handmade_reference(first0, ctg):
    """every position 1 .. ref_len + 1 as a centre (1, 9 / 10, 16, 17, 18, 99 / 100, the last 17, ref_len, one beyond);
    first0 moves the coordinates over 999 / 1000 and 999 999 999 / 1 000 000 000 and to the 2 100 000 000 of DESIGN.md 7"""
    ref = handmade_reference()
    L = len(ref)
    centres = first0 + np.arange(1, L + 2, dtype=np.int64)
    c, touched, index, pos, _t = device_columns(ref, first0, centres, handmade_reads(ref, first0), ctg)
    assert np.array_equal(c, centres)
    windex, wtext, wmeta = assert_is_the_definition(ctg.encode(), c, touched, ref, first0, index, pos)
    local = set((windex + 1).tolist())
    assert touched.any() and not touched.all() and touched[L - 1]
    assert not local & {1, 9, 10, 16, 18, 99, L - 1, L + 1} and {17, 100, 285, 288, L} <= local     # window, centre base, the ends
    assert not touched[119:179].any() and not local & set(range(120, 180))                        # out of the reads' reach
    assert sorted(set(wmeta[:, 5].tolist()))[:3] == [17, 19, 20] and wmeta[:, 5].max() == 33       # short windows at the end
    digits = set(wmeta[:, 3].tolist())
    assert digits == {0: {2, 3}, 900: {3, 4}, 999999850: {9, 10}, 2100000000: {10}}[first0]
    windows = wtext[int(wmeta[0, 4]):]
    assert any(b >= 0x80 for b in windows) and not any(97 <= b <= 122 for b in windows) and b"N" in windows and b"R" in windows
    j = int(np.flatnonzero(windex + 1 == 100)[0])
    assert pos[j] == "%s:%d:%s" % (ctg, first0 + 100, ref[83:116].upper().decode("ascii"))


# ---- dense centres: the scans and the compaction cross workgroups ------------------------------------------------------------
@pytest.fixture(scope="module")
def long_case():
    contigs, sam, _can, _opts, _want = load_case("long")
    ref = contigs["ctgA"].encode()
    text = ("\n".join(l for l in sam if not l.startswith("@")) + "\n").encode()
    return ref, text


def test_dense_centres_with_untouched_ones_interleaved(long_case):
    ref, sam = long_case
    centres = np.arange(2001, 2001 + 3200, dtype=np.int64)
    mask = np.random.default_rng(3).random(len(centres)) < 0.7
    c, touched, index, pos, _t = device_columns(ref, 0, centres, sam, "ctgA", mask)
    windex, _wtext, _wmeta = assert_is_the_definition(b"ctgA", c, touched, ref, 0, index, pos)
    assert len(windex) > 1500 and (np.diff(windex) > 1).sum() > 400 and (np.diff(windex) == 1).sum() > 400
    assert np.all(np.diff(index.cpu().numpy()) > 0)                      # stable: ascending


def abi_call(ctg, centres, touched, ref, first0):
    """cv_call_columns_dev over its own buffers -> (info, index, meta, text) whole, canaries and all"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    n = len(centres)
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c32, t8, rf = up(centres.astype(np.int32)), up(touched.astype(np.uint8)), up(np.frombuffer(ref, dtype=np.uint8).copy())
    cap = len(ctg) + 43 * n
    index = torch.full((n + CANARY,), -7, dtype=torch.int64, device=dev)
    meta = torch.full((n + CANARY, 6), -7, dtype=torch.int64, device=dev)
    text = torch.full((cap + CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    info = torch.full((4,), -7, dtype=torch.int64, device=dev)
    need = ctypes.c_int64()
    _lib.check(lib.cv_call_columns_workspace(n, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.cv_call_columns_dev(ctg, len(ctg), p(c32), p(t8), n, p(rf), first0, len(ref), p(index), p(meta), p(text), cap, p(info),
                                       p(ws), need.value, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return info.cpu().numpy(), index.cpu().numpy(), meta.cpu().numpy(), text.cpu().numpy()


def test_the_abi_writes_nothing_behind_its_rows(long_case):
    """unsorted centres with repeats (the ABI does not ask for sorted ones), 9 000 of them: many workgroups, several tiles
    of the scans; index, meta and text end where info says and the bytes behind them are untouched"""
    ref, _sam = long_case
    rng = np.random.default_rng(11)
    first0 = 999995000
    centres = rng.integers(first0 - 20, first0 + len(ref) + 40, size=9000).astype(np.int64)
    touched = (rng.random(9000) < 0.75).astype(np.uint8)
    info, index, meta, text = abi_call(b"chrX", centres, touched, ref, first0)
    windex, wtext, wmeta = definition(b"chrX", centres, touched, ref, first0)
    k = len(windex)
    assert 4000 < k < 8000 and info.tolist() == [k, len(wtext), 9000, 0]
    assert np.array_equal(index[:k], windex) and (index[k:] == -7).all()
    assert np.array_equal(meta[:k], wmeta) and (meta[k:] == -7).all()
    assert text[:len(wtext)].tobytes() == wtext and (text[len(wtext):] == 0xA5).all()
    assert {9, 10} <= set(wmeta[:, 3].tolist())


# ---- degenerate sizes and refusals ---------------------------------------------------------------------------------------------
def test_no_centre_and_nothing_kept():
    ref = handmade_reference()
    none = np.zeros(0, dtype=np.int64)
    c, touched, index, pos, _t = device_columns(ref, 50, none, handmade_reads(ref, 50), LONG_NAME)
    assert_is_the_definition(LONG_NAME.encode(), c, touched, ref, 50, index, pos)
    assert index.numel() == 0 and len(pos) == 0 and bytes(pos.pieces()[0][2]) == LONG_NAME.encode() and list(pos) == []
    centres = 50 + np.arange(1, 200, dtype=np.int64)
    for sam, mask in ((b"", None), (handmade_reads(ref, 50), np.zeros(199, dtype=bool))):        # no read at all / every flag cleared
        c, touched, index, pos, _t = device_columns(ref, 50, centres, sam, "c", mask)
        assert not touched.any()
        assert_is_the_definition(b"c", c, touched, ref, 50, index, pos)
        assert index.numel() == 0 and len(pos) == 0 and bytes(pos.pieces()[0][2]) == b"c"
    # every centre touched, none of them ACGT
    info, index, meta, text = abi_call(b"c", np.arange(17, 60, dtype=np.int64), np.ones(43, np.uint8), b"N" * 100, 0)
    assert info.tolist() == [0, 1, 43, 0] and text[:1].tobytes() == b"c" and (text[1:] == 0xA5).all() and (index == -7).all() and (meta == -7).all()


def test_refusals():
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    n = 4
    c32 = torch.arange(17, 21, dtype=torch.int32, device=dev); t8 = torch.ones(n, dtype=torch.uint8, device=dev)
    rf = torch.full((80,), ord("A"), dtype=torch.uint8, device=dev)
    index = torch.zeros(n + 1, dtype=torch.int64, device=dev); meta = torch.zeros((n + 1, 6), dtype=torch.int64, device=dev)
    text = torch.zeros(512, dtype=torch.uint8, device=dev); info = torch.zeros(5, dtype=torch.int64, device=dev)
    need = ctypes.c_int64()
    _lib.check(lib.cv_call_columns_workspace(n, ctypes.byref(need)))
    ws = torch.empty(need.value + 256, dtype=torch.uint8, device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    order = ("ctg", "ctg_len", "centres", "touched", "n", "ref", "first", "ref_len", "index", "meta", "text", "cap", "info", "ws", "ws_bytes")
    good = dict(ctg=b"ctgA", ctg_len=4, centres=p(c32), touched=p(t8), n=n, ref=p(rf), first=0, ref_len=80, index=p(index), meta=p(meta),
                text=p(text), cap=4 + 43 * n, info=p(info), ws=p(ws), ws_bytes=need.value)
    call = lambda **kw: lib.cv_call_columns_dev(*([dict(good, **kw)[k] for k in order] + [stream]))
    assert call() == 0
    torch.cuda.synchronize()
    assert info[:3].tolist() == [4, 4 + 4 * 2 + 4 * 33, 4]
    for bad in (dict(centres=None), dict(touched=None), dict(ref=None), dict(index=None), dict(meta=None), dict(text=None), dict(info=None),
                dict(ws=None), dict(centres=p(c32, 2)), dict(index=p(index, 4)), dict(meta=p(meta, 4)), dict(info=p(info, 4)),
                dict(ws=p(ws, 128)), dict(ws_bytes=need.value - 1), dict(cap=4 + 43 * n - 1), dict(first=-1), dict(n=-1),
                dict(n=(1 << 27) + 1), dict(ctg_len=1025), dict(ctg=None), dict(ref_len=-1)):
        assert call(**bad) == 1, bad
        assert b"cv_call_columns_dev" in lib.cv_last_error()
    torch.cuda.synchronize()


# ---- through the drivers --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(oracle, tmp_path_factory):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    out = {}
    for arch, mod in (("full", clairvoyante_v3), ("slim", clairvoyante_v3_slim)):
        m = mod.Clairvoyante()
        m.init()
        m.setParameters(common.bench_params(oracle, arch, seed=11))
        chk = str(tmp_path_factory.mktemp("call_columns_" + arch) / "model-000001")
        m.saveParameters(chk)
        out[arch] = (m, chk)
    yield out
    for m, _chk in out.values():
        m.close()


def _sites(tmp_path, rows):
    fn = str(tmp_path / "sites.vcf")
    with open(fn, "w") as fh:
        fh.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n")
        for ctg, p in rows:
            fh.write("%s\t%d\t.\tA\tC\t50\tPASS\t.\tGT:DP\t0/1:30\n" % (ctg, p))
    return fn


def _native_bam(tmp_path):
    from bam_writer import write_bam
    base = os.path.join(G, "noisy")
    recs = [l.rstrip("\n") for l in open(base + ".sam") if not l.startswith("@")]
    bam = str(tmp_path / "noisy.bam")
    write_bam(bam, recs, [("ctgA", 2600), ("other", 10)], block_payload=9001)
    fa = str(tmp_path / "ref.fa")
    shutil.copy(base + ".fa", fa)
    with open(fa + ".fai", "w") as fh:       # the 70-column FASTA of the generator: ">ctgA synthetic\n" is 16 bytes
        fh.write("ctgA\t2600\t16\t70\t71\n")
    return ["--bam_fn", bam, "--ref_fn", fa, "--samtools", "native", "--minCoverage", "2", "--ctgStart", "300", "--ctgEnd", "1900"]


def _fixture(name):
    base = os.path.join(G, name)
    return ["--bam_fn", base + ".sam", "--ref_fn", base + ".fa", "--samtools", FAKE]


RUNS = {
    "plain": lambda tmp: ("full", _fixture("plain")),
    "noisy": lambda tmp: ("full", _fixture("noisy") + ["--ctgStart", "0", "--ctgEnd", "2000", "--minCoverage", "2", "--dcov", "3"]),
    "region": lambda tmp: ("slim", _fixture("region") + ["--ctgStart", "600", "--ctgEnd", "2900", "--threshold", "0.2", "--slim",
                                                         "--bed_fn", os.path.join(G, "region_bed.bed")]),
    "sites": lambda tmp: ("full", _fixture("plain") + ["--qual", "30", "--vcf_fn",
                                                       _sites(tmp, [("ctgA", p) for p in (120, 455, 456, 457, 1010, 1500, 2222, 2950)] + [("other", 5)])]),
    "native": lambda tmp: ("full", _native_bam(tmp)),
    "site_without_a_window": lambda tmp: ("full", _fixture("plain") + ["--vcf_fn", _sites(tmp, [("ctgA", 5)])]),
    "no_site": lambda tmp: ("full", _fixture("plain") + ["--vcf_fn", _sites(tmp, [("other", 5)])]),
}


@pytest.mark.parametrize("case", list(RUNS))
def test_callvarbam_writes_the_same_vcf_on_either_route(case, models, tmp_path, monkeypatch):
    from clairvoyante_amd import callVar, callVarBam
    arch, cli = RUNS[case](tmp_path)
    m, chk = models[arch]
    vcf, kept = {}, {}
    for columns in ("host", "device"):
        for records in ("host", "device"):
            monkeypatch.setenv("CV_CALL_COLUMNS", columns)
            monkeypatch.setenv("CV_VCF_FORMAT", records)
            out = str(tmp_path / ("%s_%s.vcf" % (columns, records)))
            a = callVarBam.build_parser().parse_args(["--chkpnt_fn", chk, "--ctgName", "ctgA", "--call_fn", out] + cli)
            before, fbefore = callVarBam.call_column_counts(), callVar.vcf_format_counts()
            res = callVarBam.Run(a, model=m)
            after, fafter = callVarBam.call_column_counts(), callVar.vcf_format_counts()
            grew = {k: after[k] - before[k] for k in after}
            other = "device" if columns == "host" else "host"
            assert grew[columns + "_regions"] == 1 and grew[columns + "_candidates"] == res["candidates"], grew
            assert grew[other + "_regions"] == 0 and grew[other + "_candidates"] == 0 and grew["handed_over_regions"] == 0, grew
            assert fafter["handed_over"] == fbefore["handed_over"]
            assert res["route"] == columns and len(res["pos"]) == res["tensors"].shape[0]
            if columns == "device":
                assert "centers" not in res and "seqs" not in res                  # made only when asked for
                if records == "device":
                    assert not res["pos"].fetched                                  # the tokens never came to the host
            vcf[columns, records] = open(out, "rb").read()
            kept[columns, records] = (np.asarray(res["centers"]).copy(), list(res["seqs"]))
            assert kept[columns, records][0].dtype == np.int64 and len(kept[columns, records][0]) == res["tensors"].shape[0]
    records = [l for l in vcf["host", "host"].splitlines() if not l.startswith(b"#")]
    if case in ("site_without_a_window", "no_site"):
        assert records == [] and vcf["host", "host"].startswith(b"##fileformat")     # a header-only VCF
    else:
        assert len(records) > (0 if case == "sites" else 10)             # (eight sites, most of them called REF)
    for key in vcf:
        assert vcf[key] == vcf["host", "host"], key
        assert np.array_equal(kept[key][0], kept["host", "host"][0]) and kept[key][1] == kept["host", "host"][1], key


def test_an_unknown_route_raises(monkeypatch):
    from clairvoyante_amd import callVarBam
    monkeypatch.setenv("CV_CALL_COLUMNS", "gpu")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        callVarBam.call_columns_route()


def test_callfromdevice_cuts_device_columns_into_slices(long_case, models, monkeypatch):
    """~700 rows in batches of 256: the slices with first > 0 read meta from their own row on, in HBM on the device VCF
    route and from the one host copy on the host's; the records are those of the host PosBatch"""
    from clairvoyante_amd import callVar
    from clairvoyante_amd.utils_v2 import PosBatch
    ref, sam = long_case
    centres = np.arange(3001, 3001 + 760, dtype=np.int64)
    m = models["full"][0]
    a = types.SimpleNamespace(showRef=True, qual=15)

    def run(route, pos, x):
        monkeypatch.setenv("CV_VCF_FORMAT", route)
        fh = io.StringIO()
        before = callVar.vcf_format_counts()
        callVar.CallFromDevice(a, m, fh, x, pos, batch=256)
        after = callVar.vcf_format_counts()
        return fh.getvalue(), {k: after[k] - before[k] for k in after}

    text = {}
    for route in ("host", "device"):
        c, touched, index, pos, t = device_columns(ref, 0, centres, sam, LONG_NAME)
        x = t.index_select(0, index)
        rows = x.shape[0]
        assert 512 < rows <= 760 and len(pos) == rows
        text[route], grew = run(route, pos, x)
        assert grew == {"host": 3 if route == "host" else 0, "device": 3 if route == "device" else 0, "handed_over": 0}
        assert pos.fetched == (route == "host")
        part = pos.part(256, 256)
        assert len(part) == 256 and part.device["meta_ptr"] == pos.device["meta_ptr"] + 256 * 48 and part[0] == pos[256]
    windex, wtext, wmeta = definition(LONG_NAME.encode(), c, touched, ref, 0)
    want, grew = run("host", PosBatch(wtext, wmeta), x)
    assert grew == {"host": 3, "device": 0, "handed_over": 0}
    assert text["host"] == want and text["device"] == want and want.count("\n") > 600
