"""utils_v2.truth_tables without a GPU: the CV_TRUTH_TABLES switch, the host route as a wrapper of the definition, the
--vcf_fn flag and its definition (utils_v2.vcf_truth_rows = GetTruth per source, concatenated), _read_bed_truth(rows=)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import truth_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("truth_host"))
    return {"var": tc.write_lines(os.path.join(d, "truth.gz"), tc.truth_lines(), "gz"),
            "bed": tc.write_lines(os.path.join(d, "conf.bed"), tc.bed_lines(), "plain"),
            "vcf": tc.write_lines(os.path.join(d, "truth.vcf.gz"), tc.vcf_lines(), "bgzf"), "dir": d}


def test_the_switch(monkeypatch, tmp_path):
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: True)
    for value, want in (("host", "host"), ("device", "device")):
        monkeypatch.setenv("CV_TRUTH_TABLES", value)
        assert utils_v2.truth_tables_route() == utils_v2.truth_tables_route("no such file", None) == want
    for bad in ("Device", "gpu", "1"):
        monkeypatch.setenv("CV_TRUTH_TABLES", bad)
        with pytest.raises(ValueError, match="CV_TRUTH_TABLES must be 'host' or 'device', got '%s'" % bad):
            utils_v2.truth_tables_route()
        with pytest.raises(ValueError, match="CV_TRUTH_TABLES"):
            utils_v2.truth_tables(None, None)
    # unset (or empty): the size of the truth list decides, of the BED file when there is no truth list
    floors = utils_v2.TRUTH_TABLES_DEVICE_MIN_BYTES
    assert sorted(floors) == ["bgzf", "gz", "plain"]
    big, small = str(tmp_path / "big.txt"), str(tmp_path / "small.txt")
    for fn, size in ((big, floors["plain"]), (small, floors["plain"] - 1)):
        with open(fn, "wb") as fh:
            fh.write(b"chr1 5 A C 0 1\n")
            fh.truncate(size)
    for value in (None, ""):
        if value is None:
            monkeypatch.delenv("CV_TRUTH_TABLES", raising=False)
        else:
            monkeypatch.setenv("CV_TRUTH_TABLES", value)
        assert utils_v2.truth_tables_route() == "host" and utils_v2.truth_tables_route("no such file", None) == "host"
        assert utils_v2.truth_tables_route(big, None) == "device" and utils_v2.truth_tables_route(small, big) == "host"
        assert utils_v2.truth_tables_route(None, big) == "device" and utils_v2.truth_tables_route(None, small) == "host"
        # a truth VCF: BGZF from its own floor on, any other form on the host
        assert utils_v2.truth_tables_route(None, big, vcf_fn=big) == "host" and utils_v2.truth_tables_route(vcf_fn="no such file") == "host"
        bg = tc.write_lines(str(tmp_path / "t.vcf.gz"), [b"chr1\t5\t.\tA\tC\t5\tPASS\t.\tGT\t0/1"], "bgzf")
        assert utils_v2.truth_tables_route(vcf_fn=bg) == "host"
        monkeypatch.setattr(utils_v2, "TRUTH_VCF_DEVICE_MIN_BYTES", os.path.getsize(bg))
        assert utils_v2.truth_tables_route(vcf_fn=bg) == "device"
        monkeypatch.setattr(utils_v2, "TRUTH_VCF_DEVICE_MIN_BYTES", os.path.getsize(bg) + 1)
        assert utils_v2.truth_tables_route(vcf_fn=bg) == "host"
    monkeypatch.setitem(floors, "plain", None)
    assert utils_v2.truth_tables_route(big, None) == "host"
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)      # without a GPU the route is the host's, whatever is asked
    monkeypatch.setenv("CV_TRUTH_TABLES", "device")
    assert utils_v2.truth_tables_route() == "host" and utils_v2.truth_tables_route(big, None) == "host"


def test_the_host_route_wraps_the_definition(files, monkeypatch):
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    monkeypatch.setenv("CV_TRUTH_TABLES", "device")
    utils_v2.truth_table_counts(reset=True)
    for var, bed in ((files["var"], files["bed"]), (files["var"], None), (None, files["bed"]), (None, None)):
        got = utils_v2.truth_tables(var, bed, want_every=True)
        assert got.route == "host" and got.reason is None and "tables" in got.times
        tc.same_tables(got, tc.definition_tables(var, bed), (var, bed))
        assert utils_v2.truth_tables(var, bed).every is None
    counts = utils_v2.truth_table_counts(reset=True)
    assert counts["host_calls"] == 8 and counts["device_calls"] == 0 and counts["handed_over_calls"] == 0 and counts["device_lines"] == 0
    assert set(utils_v2.truth_table_counts().values()) == {0}
    # exceptions pass through: a truth contig the BED lacks, a malformed coordinate
    d = files["dir"]
    bed = tc.write_lines(os.path.join(d, "short.bed"), [b"chr1 0 5000"], "plain")
    with pytest.raises(KeyError):
        utils_v2.truth_tables(files["var"], bed)
    bad = tc.write_lines(os.path.join(d, "bad.var"), [b"chr1 12 A C 0 1", b"chr1 x A C 0 1"], "plain")
    with pytest.raises(ValueError, match="invalid literal"):
        utils_v2.truth_tables(bad, None)


def test_rows_in_place_of_the_file(files):
    from clairvoyante_amd import utils_v2
    rows = list(utils_v2._gz_lines(files["var"]))
    assert len(rows) > 1000
    for bed in (files["bed"], None):
        e1, e2 = {}, {}
        tree1, Y1 = utils_v2._read_bed_truth(files["var"], bed, e1)
        tree2, Y2 = utils_v2._read_bed_truth(None, bed, e2, rows=rows)
        assert Y1 == Y2 and list(Y1) == list(Y2) and e1 == e2 and list(e1) == list(e2) and len(Y1) > 100
        assert list(tree1) == list(tree2) and all(tree1[k].iv == tree2[k].iv for k in tree1)
    assert utils_v2._read_bed_truth(None, None) == ({}, {}) and utils_v2._read_bed_truth(None, None, rows=[]) == ({}, {})


SOURCES = (   # (bam, ref, contig, ctgStart, ctgEnd): overlapping bounds on one contig, one source without bounds, a contig with no record
    (("a.bam", "a.fa", "chr1", 100, 700),),
    (("a.bam", "a.fa", "chr1", 100, 700), ("b.bam", "b.fa", "chr1", 400, 1200)),
    (("a.bam", "a.fa", "chr10", None, None), ("b.bam", "b.fa", "chrUn", 5, 900), ("c.bam", "c.fa", "chr2", 0, 300)),
    (("a.bam", "a.fa", "chr2", 50, None),),                  # one bound alone is no bound (GetTruth.py:58)
)


@pytest.mark.parametrize("k", range(len(SOURCES)))
def test_the_vcf_definition_is_gettruth_per_source(files, k):
    from clairvoyante_amd import utils_v2
    sources = SOURCES[k]
    want = b""
    for _b, _r, ctg, cs, ce in sources:
        cmd = [sys.executable, "-m", "clairvoyante_amd.GetTruth", "--vcf_fn", files["vcf"], "--ctgName", ctg]
        cmd += [] if cs is None else ["--ctgStart", str(cs)]
        cmd += [] if ce is None else ["--ctgEnd", str(ce)]
        want += subprocess.check_output(cmd, cwd=ROOT)
    rows = utils_v2.vcf_truth_rows(files["vcf"], sources)
    assert "".join(rows).encode("ascii") == want and (len(rows) > 20 or k == 0)
    # ... and truth_tables(vcf_fn=) is the definition over those rows
    var = os.path.join(files["dir"], "from_vcf_%d.var" % k)
    with open(var, "wb") as fh:
        fh.write(want)
    for bed in (None, files["bed"]):
        got = utils_v2.truth_tables(None, bed, vcf_fn=files["vcf"], sources=sources, want_every=True)
        assert got.route == "host"
        tc.same_tables(got, tc.definition_tables(var, bed), (k, bed))
    with pytest.raises(ValueError, match="both given"):
        utils_v2.truth_tables(var, None, vcf_fn=files["vcf"], sources=sources)
    with pytest.raises(ValueError, match="needs the sources"):
        utils_v2.truth_tables(None, None, vcf_fn=files["vcf"])


def test_the_vcf_flag(capsys, monkeypatch):
    from clairvoyante_amd import tensor2Bin, train, utils_v2
    assert "--vcf_fn" in [f[0] for f in utils_v2.BAM_FLAGS]
    bam = ["--bam_fn", "a.bam", "--ref_fn", "a.fa", "--ctgName", "chr1"]
    for parser in (tensor2Bin.build_parser(), train.build_parser("t", bam=True)):
        args = parser.parse_args(bam + ["--vcf_fn", "t.vcf.gz"])
        assert utils_v2.bam_sources(args) == [("a.bam", "a.fa", "chr1", None, None)]
        assert utils_v2.truth_inputs(args) == (None, "t.vcf.gz")
        assert utils_v2.truth_inputs(parser.parse_args(bam + ["--var_fn", "v.gz"])) == ("v.gz", None)
        with pytest.raises(ValueError, match="--vcf_fn and --var_fn are both given"):
            utils_v2.bam_sources(parser.parse_args(bam + ["--vcf_fn", "t.vcf.gz", "--var_fn", "v.gz"]))
        with pytest.raises(ValueError, match="--vcf_fn needs --bam_fn"):
            utils_v2.bam_sources(parser.parse_args(["--vcf_fn", "t.vcf.gz"]))
    # the command line says so through parser.error
    for argv, text in ((["--vcf_fn", "t.vcf.gz", "--bin_fn", "o.bin"], "--vcf_fn needs --bam_fn"),
                       (bam + ["--vcf_fn", "t.vcf.gz", "--var_fn", "v.gz", "--bin_fn", "o.bin"], "both given")):
        monkeypatch.setattr(sys, "argv", ["tensor2Bin"] + argv)
        with pytest.raises(SystemExit) as e:
            tensor2Bin.main()
        assert e.value.code == 2 and text in capsys.readouterr().err
