"""The truth list and the BED file read on the GPU (utils_v2.truth_tables with CV_TRUTH_TABLES=device,
csrc/cv_truth_dev.hip) against the host loop that defines the result: names, every table (values, dtype, shape) and the
positions of all truth rows, no tolerance.  Every test asserts the route it took and the counters of truth_table_counts(),
so that neither a silent hand-over nor a dropped line can pass.  A single irregular line sends the whole call to the host:
same result or same exception there."""
import ctypes
import os
import pickle
import random

import numpy as np
import pytest

import truth_cases as tc

pytestmark = pytest.mark.gpu
FORMATS = ("plain", "gz", "bgzf")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("truth_tables"))
    out = {"dir": d, "var_lines": tc.truth_lines(), "bed_lines": tc.bed_lines()}
    for how in FORMATS:
        out["var", how] = tc.write_lines(os.path.join(d, "truth." + how), out["var_lines"], how)
        out["bed", how] = tc.write_lines(os.path.join(d, "conf.bed." + how), out["bed_lines"], how)
    out["want", True] = tc.definition_tables(out["var", "plain"], out["bed", "plain"])
    out["want", False] = tc.definition_tables(out["var", "plain"], None)
    return out


@pytest.fixture
def device_route(monkeypatch):
    from clairvoyante_amd import utils_v2
    monkeypatch.setenv("CV_TRUTH_TABLES", "device")
    utils_v2.truth_table_counts(reset=True)
    return utils_v2


def _on_device(got, lines):
    from clairvoyante_amd import utils_v2
    assert got.route == "device" and got.reason is None
    assert all(v.is_cuda for v in got.tables.values())
    c = utils_v2.truth_table_counts(reset=True)
    assert c["host_lines"] == 0 and c["host_calls"] == 0 and c["handed_over_calls"] == 0 and c["device_calls"] == 1
    assert lines <= c["device_lines"] <= lines + 2           # (+ the blank line behind each file's last newline)


@pytest.mark.parametrize("slab", [None, 4096, 257])
@pytest.mark.parametrize("use_bed", [True, False])
@pytest.mark.parametrize("fmt", FORMATS)
def test_tables_equal_the_definition(files, device_route, monkeypatch, fmt, use_bed, slab):
    """slabs of 4096 and 257 bytes put dozens of seams inside lines; 257 also starts the slabs off the 16-byte granules"""
    utils_v2 = device_route
    if slab is not None:
        monkeypatch.setattr(utils_v2, "TRUTH_SLAB_BYTES", slab)
    want = files["want", use_bed]
    assert len(want[0]) == 5 and len(want[1]["truth_pos"]) > (300 if use_bed else 1000) and (not use_bed or len(want[1]["bed_begin"]) > 400)
    got = utils_v2.truth_tables(files["var", fmt], files["bed", fmt] if use_bed else None, want_every=True)
    tc.same_tables(got, want, (fmt, use_bed, slab))
    _on_device(got, len(files["var_lines"]) + (len(files["bed_lines"]) if use_bed else 0))
    assert got.tables["labels"].dtype.is_floating_point and tuple(got.tables["labels"].shape) == want[1]["labels"].shape


def test_degenerate_inputs(files, device_route, tmp_path):
    utils_v2 = device_route
    d = str(tmp_path)
    for var, bed, lines in ((None, files["bed", "bgzf"], len(files["bed_lines"])), (None, None, 0)):
        got = utils_v2.truth_tables(var, bed, want_every=True)
        tc.same_tables(got, tc.definition_tables(var, bed), (var, bed))
        _on_device(got, lines)
    # a last line without a newline is a line; an empty file and a file of blank lines have no row
    cut = tc.write_lines(os.path.join(d, "cut.var"), files["var_lines"][:40], "plain", last_newline=False)
    empty = tc.write_lines(os.path.join(d, "empty.var"), [], "plain")
    blank = tc.write_lines(os.path.join(d, "blank.bed"), [b"", b"  ", b"\t"], "gz")
    for var, bed, lines in ((cut, None, 40), (empty, None, 0), (empty, blank, 3), (None, blank, 3)):
        got = utils_v2.truth_tables(var, bed, want_every=True)
        tc.same_tables(got, tc.definition_tables(var, bed), (var, bed))
        _on_device(got, lines)


IRREGULAR = tuple(i for i in tc.IRREGULAR if i[1] != tc.VCF) + (("truth_contig_absent_from_the_bed", tc.VAR, b"chrUn 80 A C 0 1", False),)


@pytest.mark.parametrize("k", range(len(IRREGULAR)), ids=[i[0] for i in IRREGULAR])
def test_one_irregular_line(files, device_route, tmp_path, k):
    """a single irregular line in an otherwise regular file: the whole call goes to the host, with the definition's result
    or its exception (type and message) -- unless the device vouches for the line, then it stays"""
    utils_v2 = device_route
    name, fmt, line, stays = IRREGULAR[k]
    var_lines, bed_lines = list(files["var_lines"]), list(files["bed_lines"])
    (var_lines if fmt == tc.VAR else bed_lines).insert(333, line)
    var = tc.write_lines(str(tmp_path / "truth.gz"), var_lines, "bgzf")
    bed = tc.write_lines(str(tmp_path / "conf.bed"), bed_lines, "plain")
    try:
        want, raised = tc.definition_tables(var, bed), None
    except Exception as e:                                   # noqa: BLE001 -- whatever the definition raises
        want, raised = None, e
    if raised is not None:
        assert not stays
        with pytest.raises(type(raised)) as e:
            utils_v2.truth_tables(var, bed, want_every=True)
        assert str(e.value) == str(raised)
    else:
        got = utils_v2.truth_tables(var, bed, want_every=True)
        tc.same_tables(got, want, name)
        assert got.route == ("device" if stays else "host") and (got.reason is None) == stays, got.reason
    c = utils_v2.truth_table_counts(reset=True)
    assert (c["device_calls"], c["handed_over_calls"], c["host_calls"]) == ((1, 0, 0) if stays else (0, 1, 1))
    assert stays or c["host_lines"] == 1 or name == "truth_contig_absent_from_the_bed"
    assert {"noncanonical_integer": raised is None, "five_token_truth_row": isinstance(raised, IndexError),
            "two_token_bed_row": isinstance(raised, IndexError), "n_first_base_of_het_indel": isinstance(raised, KeyError),
            "truth_contig_absent_from_the_bed": isinstance(raised, KeyError)}.get(name, True)


VCF_SOURCES = (   # 1, 2 and 3 sources: overlapping bounds on one contig, a source without bounds, a contig with no record
    (("a.bam", "a.fa", "chr1", 100, 700),),
    (("a.bam", "a.fa", "chr1", 100, 700), ("b.bam", "b.fa", "chr1", 400, 1200)),
    (("a.bam", "a.fa", "chr10", None, None), ("b.bam", "b.fa", "chrUn", 5, 900), ("c.bam", "c.fa", "chr2", 0, 300)),
)


def _vcf_definition(utils_v2, vcf, sources, bed, d, tag):
    """the --vcf_fn definition: GetTruth's rows per source, concatenated, through the host loop"""
    var = tc.write_lines(os.path.join(d, "from_vcf_%s.var" % tag), [r.rstrip("\n").encode() for r in utils_v2.vcf_truth_rows(vcf, sources)])
    return tc.definition_tables(var, bed)


@pytest.mark.parametrize("slab", [None, 257])
@pytest.mark.parametrize("use_bed", [True, False])
@pytest.mark.parametrize("k", range(len(VCF_SOURCES)))
def test_vcf_tables_equal_the_definition(files, device_route, monkeypatch, k, use_bed, slab):
    utils_v2 = device_route
    if slab is not None:
        monkeypatch.setattr(utils_v2, "TRUTH_SLAB_BYTES", slab)
    lines = tc.vcf_lines()
    vcf = tc.write_lines(os.path.join(files["dir"], "truth.vcf.gz"), lines, "bgzf")
    bed = files["bed", "plain"] if use_bed else None
    want = _vcf_definition(utils_v2, vcf, VCF_SOURCES[k], bed, files["dir"], "%d" % k)
    assert len(want[1]["truth_pos"]) > 10 and (k != 1 or len(want[2]["chr1"]) < sum(1 for _ in utils_v2.vcf_truth_rows(vcf, VCF_SOURCES[k])))
    got = utils_v2.truth_tables(None, bed, vcf_fn=vcf, sources=VCF_SOURCES[k], want_every=True)
    tc.same_tables(got, want, (k, use_bed, slab))
    assert got.route == "device" and got.reason is None and all(v.is_cuda for v in got.tables.values())
    c = utils_v2.truth_table_counts(reset=True)
    assert c["host_lines"] == 0 and c["host_calls"] == 0 and c["handed_over_calls"] == 0 and c["device_calls"] == 1
    nbed = len(files["bed_lines"]) if use_bed else 0
    assert nbed + len(lines) * len(VCF_SOURCES[k]) <= c["device_lines"] <= nbed + 1 + (len(lines) + 1) * len(VCF_SOURCES[k])


VCF_IRREGULAR = [i for i in tc.IRREGULAR if i[1] == tc.VCF]


@pytest.mark.parametrize("k", range(len(VCF_IRREGULAR)), ids=[i[0] for i in VCF_IRREGULAR])
def test_one_irregular_vcf_line(files, device_route, tmp_path, k):
    utils_v2 = device_route
    name, _fmt, line, stays = VCF_IRREGULAR[k]
    lines = tc.vcf_lines()
    lines.insert(120, line)
    vcf = tc.write_lines(str(tmp_path / "truth.vcf.gz"), lines, "bgzf")
    sources = VCF_SOURCES[1]
    try:
        want, raised = _vcf_definition(utils_v2, vcf, sources, None, str(tmp_path), "irr"), None
    except Exception as e:                                   # noqa: BLE001 -- whatever the definition raises
        want, raised = None, e
    assert (raised is None) == stays and (stays or isinstance(raised, ValueError))
    if raised is not None:
        with pytest.raises(type(raised)) as e:
            utils_v2.truth_tables(None, None, vcf_fn=vcf, sources=sources, want_every=True)
        assert str(e.value) == str(raised)
    else:
        got = utils_v2.truth_tables(None, None, vcf_fn=vcf, sources=sources, want_every=True)
        tc.same_tables(got, want, name)
        assert got.route == "device"
    c = utils_v2.truth_table_counts(reset=True)
    assert (c["device_calls"], c["handed_over_calls"], c["host_calls"]) == ((1, 0, 0) if stays else (0, 1, 1))


# ---- end to end: the sets bit for bit under both routes -------------------------------------------------------------------
def _set_of(ts):
    return ts.total, ts.X.cpu().numpy().view(np.uint32), ts.Y.cpu().numpy().view(np.uint32), ts.keys()


def _same_sets(a, b):
    assert a[0] == b[0] > 0 and a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_training_set_from_text_is_the_same_under_both_routes(tmp_path, monkeypatch):
    import trainset_cases as cases
    from clairvoyante_amd import utils_v2
    f = cases.write_case(str(tmp_path), "full")
    sets = {}
    for route in ("host", "device"):
        monkeypatch.setenv("CV_TRUTH_TABLES", route)
        utils_v2.truth_table_counts(reset=True)
        random.seed(cases.SEED)
        ts = utils_v2.GetTrainingSetDevice(f["bgzf"], f["var"], f["bed"], True, num=400)
        assert ts.route == "device" and ts.times["tables"] > 0
        assert utils_v2.truth_table_counts()[route + "_calls"] == 1 and utils_v2.truth_table_counts()["handed_over_calls"] == 0
        sets[route] = _set_of(ts)
    _same_sets(sets["host"], sets["device"])
    want = cases.host_result(f, "full", True)
    assert sets["device"][0] == want[0] and sets["device"][3] == want[4]


@pytest.fixture(scope="module")
def bam_world(tmp_path_factory):
    import bamtrain_cases as bc
    d = str(tmp_path_factory.mktemp("truth_bam"))
    a = bc.make_source(d, "a", "ctgA", 11, region=(500, 5000))
    truth = bc.truth_rows("ctgA", a["ref"], 3, 100, extra=(900, 5900))
    return {"d": d, "a": a, "truth": truth, "var_fn": bc.write_rows(os.path.join(d, "var.gz"), truth),
            "bed_fn": bc.write_rows(os.path.join(d, "bed.gz"), bc.bed_rows("ctgA", 6000, 900))}


def test_training_set_from_bam_is_the_same_under_both_routes(bam_world, monkeypatch):
    import bamtrain_cases as bc
    from clairvoyante_amd import utils_v2
    w, sets = bam_world, {}
    for route in ("host", "device"):
        monkeypatch.setenv("CV_TRUTH_TABLES", route)
        utils_v2.truth_table_counts(reset=True)
        ts = utils_v2.GetTrainingSetFromBam([bc.source_tuple(w["a"])], w["var_fn"], w["bed_fn"], amp=2, candidates=bc.CANDIDATES,
                                            genomeSize=bc.GENOME, seed=77, shuffle=False, samtools=bc.FAKE)
        assert utils_v2.truth_table_counts()[route + "_calls"] == 1 and utils_v2.truth_table_counts()["handed_over_calls"] == 0
        sets[route] = _set_of(ts) + (ts.pairing,)
    _same_sets(sets["host"], sets["device"])
    assert sets["host"][4] == sets["device"][4] and sets["host"][4]["v"] > 50


def test_tensor2bin_vcf_fn_writes_the_recipes_bin(bam_world, tmp_path, monkeypatch):
    """tensor2Bin --bam_fn ... --vcf_fn V writes the .bin bytes of the recipe GetTruth per source + --var_fn, same --seed"""
    import subprocess
    import sys
    import bamtrain_cases as bc
    from clairvoyante_amd import tensor2Bin, utils_v2
    w = bam_world
    utils_v2.truth_table_counts(reset=True)
    rows = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for k, (ctg, p, ref, alt, g1, g2) in enumerate(w["truth"]):
        gt = ("%s/%s", "%s|%s")[k % 2] % ((g2, g1) if k % 3 == 0 else (g1, g2))
        rows.append(("\t".join((ctg, str(p), ".", ref, alt, "50", "PASS", ".", "GT:DP", gt + ":30"))).encode())
        rows.append(("\t".join(("ctgB", str(p), ".", ref, alt, "50", "PASS", ".", "GT", gt))).encode())
    vcf = tc.write_lines(str(tmp_path / "truth.vcf.gz"), rows, "bgzf")
    var = str(tmp_path / "truth_from_vcf.gz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-m", "clairvoyante_amd.GetTruth", "--vcf_fn", vcf, "--var_fn", var, "--ctgName", "ctgA",
                           "--ctgStart", "500", "--ctgEnd", "5000"], cwd=root)
    a = w["a"]
    common = ["--bam_fn", a["sam"], "--ref_fn", a["fa"], "--ctgName", "ctgA", "--ctgStart", "500", "--ctgEnd", "5000", "--bed_fn", w["bed_fn"],
              "--candidates", str(bc.CANDIDATES), "--genomeSize", str(bc.GENOME), "--seed", "77", "--samtools", bc.FAKE]
    out = {}
    for tag, route, truth in (("var", "host", ["--var_fn", var]), ("var", "device", ["--var_fn", var]), ("vcf", "device", ["--vcf_fn", vcf])):
        monkeypatch.setenv("CV_TRUTH_TABLES", route)
        fn = str(tmp_path / ("%s_%s.bin" % (tag, route)))
        random.seed(5)
        tensor2Bin.Run(tensor2Bin.build_parser().parse_args(common + truth + ["--bin_fn", fn]))
        out[tag, route] = open(fn, "rb").read()
        c = utils_v2.truth_table_counts(reset=True)            # the route named is the route taken, the VCF's too
        assert c[route + "_calls"] == 1 and c["handed_over_calls"] == 0 and c["host_calls" if route == "device" else "device_calls"] == 0
    assert pickle.loads(out["var", "host"]) > 150           # (the first pickle: the set's total)
    assert out["var", "host"] == out["var", "device"] == out["vcf", "device"]


from test_gpu_call_columns import models  # noqa: E402,F401 -- the fixture: a small model of each topology and its checkpoint


def test_callvarbam_vcf_fn_writes_the_same_vcf_under_both_routes(models, tmp_path, monkeypatch):  # noqa: F811
    """callVarBam --vcf_fn: the candidate sites from the device VCF pass are the host loop's, and so is the VCF written"""
    import test_gpu_call_columns as cc
    from clairvoyante_amd import callVarBam, utils_v2
    m, chk = models["full"]
    sites = cc._sites(tmp_path, [("ctgA", p) for p in (120, 455, 456, 457, 455, 1010, 1500, 2222, 2950)] + [("other", 5)])
    out = {}
    for bounds in ([], ["--ctgStart", "400", "--ctgEnd", "2000"]):
        for route in ("host", "device"):
            monkeypatch.setenv("CV_TRUTH_TABLES", route)
            utils_v2.truth_table_counts(reset=True)
            fn = str(tmp_path / ("%s_%d.vcf" % (route, len(bounds))))
            a = callVarBam.build_parser().parse_args(["--chkpnt_fn", chk, "--ctgName", "ctgA", "--call_fn", fn, "--qual", "30", "--vcf_fn", sites]
                                                     + cc._fixture("plain") + bounds)
            res = callVarBam.Run(a, model=m)
            c = utils_v2.truth_table_counts()
            assert c["device_calls"] == (1 if route == "device" else 0) and c["handed_over_calls"] == 0
            out[route, len(bounds)] = (open(fn, "rb").read(), res["candidates"])
        assert out["host", len(bounds)] == out["device", len(bounds)]
        assert out["host", len(bounds)][1] > 3
        assert len([l for l in out["host", len(bounds)][0].splitlines() if not l.startswith(b"#")]) > 0


# ---- the stream contract at the ABI level --------------------------------------------------------------------------------
CANARY = 0x5A


def _lines_dev(torch, lib, text, fmt, stream):
    """cv_truth_lines_dev over its own buffers on `stream` -> (info, pos, aux, run, tok) as numpy, whole, canaries and all"""
    from clairvoyante_amd import _lib
    n, pad = text.count(b"\n") + 3, 7
    dev = torch.device("cuda")
    buf = torch.full((len(text) + 64,), CANARY, dtype=torch.uint8, device=dev)
    buf[17:17 + len(text)].copy_(torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()))       # (off the 16-byte granule)
    def fill(shape, dt):
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
        return torch.full((nbytes,), CANARY, dtype=torch.uint8, device=dev).view(dt).reshape(shape)

    pos, aux = fill((n + pad,), torch.int64), fill((n + pad,), torch.int64) if fmt == tc.BED else fill((n + pad, 16), torch.float32)
    run, tok, info = fill((n + pad,), torch.int32), fill((n + pad, 2), torch.int64), fill((8 + pad,), torch.int64)
    need = ctypes.c_int64()
    _lib.check(lib.cv_truth_lines_workspace(len(text), n, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.stream(stream):
        _lib.check(lib.cv_truth_lines_dev(ctypes.c_void_p(buf.data_ptr() + 17), len(text), fmt, None, 0, 0, 0, 0, n, p(pos), p(aux) if fmt == tc.BED else None,
                                          None if fmt == tc.BED else p(aux), p(run), p(tok), p(info), p(ws), need.value,
                                          ctypes.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    assert (buf[:17] == CANARY).all() and (buf[17 + len(text):] == CANARY).all()
    return [t.cpu().numpy() for t in (info, pos, aux, run, tok)], (pos, aux, run), n


def _host_form(lib, text, fmt, n):
    from clairvoyante_amd import _lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos = np.zeros(n, np.int64); end = np.zeros(n, np.int64); lab = np.zeros((n, 16), np.float32)
    run = np.zeros(n, np.int32); tok = np.zeros((n, 2), np.int64); info = np.zeros(8, np.int64)
    _lib.check(lib.cv_truth_lines_host_form(p(np.frombuffer(text, dtype=np.uint8)), len(text), fmt, None, 0, 0, 0, 0, n, p(pos), p(end) if fmt == tc.BED else None,
                                            None if fmt == tc.BED else p(lab), p(run), p(tok), p(info)))
    return info, pos, end if fmt == tc.BED else lab, run, tok


def _canary_of(a):
    return np.frombuffer(bytes([CANARY]) * a.dtype.itemsize, dtype=a.dtype)[0]


def _ids(text, tok, runs, ids):
    out = []
    for o, ln in tok[:runs].tolist():
        out.append(ids.setdefault(text[o:o + ln], len(ids)))
    return np.array(out or [0], dtype=np.int32)


def test_stream_contract(files):
    """the line pass and both table passes on a non-default stream: equal to the host form / the definition, and the bytes
    behind every output (and between the rows and the end of a row array) untouched"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    stream = torch.cuda.Stream()
    dev = torch.device("cuda")
    texts = {fmt: b"\n".join(files[k]) + b"\n" for fmt, k in ((tc.BED, "bed_lines"), (tc.VAR, "var_lines"))}
    ids, kept = {}, {}
    for fmt in (tc.BED, tc.VAR):                              # (BED first: its contigs get the first ids)
        (info, pos, aux, run, tok), dev_cols, n = _lines_dev(torch, lib, texts[fmt], fmt, stream)
        want = _host_form(lib, texts[fmt], fmt, n)
        rows, runs = int(want[0][2]), int(want[0][5])
        assert info[:8].tolist() == want[0].tolist() and rows > 400 and runs > 50 and info[4] == 0
        assert (info[8:] == _canary_of(info)).all()
        for got, exp, k in ((pos, want[1], rows), (aux, want[2], rows), (run, want[3], rows), (tok, want[4], runs)):
            assert np.array_equal(got[:k], exp[:k]) and (got[k:] == _canary_of(got)).all()
        kept[fmt] = (dev_cols, rows, _ids(texts[fmt], tok, runs, ids), runs)
    nctg = len(ids)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    fill = lambda k, dt=torch.int64: torch.full((k,), -77, dtype=dt, device=dev)
    need = ctypes.c_int64()
    # the BED table
    (begin, end, run), nb, run_ctg, runs = kept[tc.BED]
    bed_off, bed_begin, bed_emax = fill(nctg + 1 + 5), fill(nb + 5), fill(nb + 5)
    _lib.check(lib.cv_bed_table_workspace(nb, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    rc = torch.from_numpy(run_ctg).to(dev)
    with torch.cuda.stream(stream):
        _lib.check(lib.cv_bed_table_dev(nb, p(begin), p(end), p(run), p(rc), runs, nctg, p(bed_off), p(bed_begin), p(bed_emax), p(ws),
                                        need.value, ctypes.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    names, tables, every = files["want", True]
    assert [n for n, _i in sorted(ids.items(), key=lambda kv: kv[1])] == names
    for got, k, key in ((bed_off, nctg + 1, "bed_off"), (bed_begin, nb, "bed_begin"), (bed_emax, nb, "bed_emax")):
        assert np.array_equal(got[:k].cpu().numpy(), tables[key]) and (got[k:] == -77).all(), key
    # the truth tables
    (pos, label, run), n, run_ctg, runs = kept[tc.VAR]
    truth_off, every_off, truth_pos, every_pos = fill(nctg + 1 + 5), fill(nctg + 1 + 5), fill(n + 5), fill(n + 5)
    labels, counts = fill((n + 5) * 16, torch.float32), fill(2 + 5)
    _lib.check(lib.cv_truth_tables_workspace(n, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    rc = torch.from_numpy(run_ctg).to(dev)
    with torch.cuda.stream(stream):
        _lib.check(lib.cv_truth_tables_dev(n, p(pos), p(label), p(run), p(rc), runs, nctg, 1, p(bed_off), p(bed_begin), p(bed_emax),
                                           p(truth_off), p(truth_pos), p(labels), p(every_off), p(every_pos), p(counts), p(ws), need.value,
                                           ctypes.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    nt, ne = counts[:2].tolist()
    assert nt == len(tables["truth_pos"]) and ne == sum(len(v) for v in every.values()) and (counts[2:] == -77).all()
    assert np.array_equal(truth_off[:nctg + 1].cpu().numpy(), tables["truth_off"]) and (truth_off[nctg + 1:] == -77).all()
    assert np.array_equal(truth_pos[:nt].cpu().numpy(), tables["truth_pos"]) and (truth_pos[nt:] == -77).all()
    assert np.array_equal(labels[:nt * 16].cpu().numpy().reshape(-1, 16), tables["labels"]) and (labels[nt * 16:] == -77).all()
    off = every_off[:nctg + 1].cpu().numpy()
    assert (every_off[nctg + 1:] == -77).all() and (every_pos[ne:] == -77).all() and off[-1] == ne
    ep = every_pos[:ne].cpu().numpy()
    for c, name in enumerate(names):
        assert np.array_equal(ep[off[c]:off[c + 1]], every.get(name.decode(), np.zeros(0, np.int64))), name
