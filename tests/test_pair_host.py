"""clairvoyante_amd/PairWithNonVariants.py (Pair) on small text files against a straightforward restatement with the
same draws, its log lines against the reference's format strings, and the --bam_fn family of flags of tensor2Bin /
train.py.  No GPU."""
import argparse
import gzip
import logging
import os

import numpy as np
import pytest


def _write(fn, rows):
    with gzip.open(str(fn), "wt") as fh:
        fh.write("".join(r + "\n" for r in rows))
    return str(fn)


def _inputs(tmp_path, n_var, n_can, seed):
    """rows `ctg pos payload` (Pair reads two columns); a few non-variants sit on truth keys, one contig has no BED"""
    rng = np.random.RandomState(seed)
    ctgs = ["ctg10", "ctg9", "nobed"]
    var = [(ctgs[int(rng.randint(0, 2))], int(p)) for p in rng.randint(1, 5000, n_var)]
    can = [(ctgs[int(rng.randint(0, 3))], int(p)) for p in rng.randint(1, 5000, n_can)] + var[:5]
    bed = ["ctg10 0 2500", "ctg9 1000 4000", "ctg9 4500 4501"]
    return (_write(tmp_path / "var.gz", ["%s %d v%d" % (c, p, k) for k, (c, p) in enumerate(var)]),
            _write(tmp_path / "can.gz", ["%s %d c%d" % (c, p, k) for k, (c, p) in enumerate(can)]),
            _write(tmp_path / "bed.gz", bed), var, can)


def _hit(ctg, p):
    return (ctg == "ctg10" and 0 <= p < 2499) or (ctg == "ctg9" and (1000 <= p < 3999 or p == 4500))


def _restated(var, can, use_bed, amp, seed):
    from clairvoyante_amd import draws
    d = set(var)
    usable = [(k, c, p) for k, (c, p) in enumerate(can) if (not use_bed or _hit(c, p)) and (c, p) not in d]
    v, c = len(var), len(usable)
    r = min(1.0, (v * amp) / c) if c else 1.0
    out = ["%s %d v%d" % (cg, p, k) for k, (cg, p) in enumerate(var)]
    out += ["%s %d c%d" % (cg, p, k) for k, cg, p in usable if draws.draws(seed, draws.PAIR, cg, [p])[0] < r]
    return out, v, c, r


@pytest.mark.parametrize("n_var,n_can,amp,use_bed,kind", [
    (40, 600, 2, True, "r<1"), (40, 600, 2, False, "r<1"), (40, 600, 0.25, True, "r<1"), (300, 400, 2, True, "r=1"),
    (30, 0, 2, True, "c=0"), (0, 50, 2, False, "r<1")])
def test_pair_equals_the_restatement(tmp_path, caplog, n_var, n_can, amp, use_bed, kind):
    from clairvoyante_amd import PairWithNonVariants as pw
    var_fn, can_fn, bed_fn, var, can = _inputs(tmp_path, n_var, n_can, 4)
    if kind == "c=0":
        can = var[:5]                                   # every non-variant sits on a truth key
        can_fn = _write(tmp_path / "can.gz", ["%s %d c%d" % (c, p, k) for k, (c, p) in enumerate(can)])
    out = str(tmp_path / "mix.gz")
    with caplog.at_level(logging.INFO):
        got = pw.Pair(argparse.Namespace(tensor_can_fn=can_fn, tensor_var_fn=var_fn, bed_fn=bed_fn if use_bed else None,
                                         output_fn=out, amp=amp, seed=31))
    want, v, c, r = _restated(var, can, use_bed, amp, 31)
    assert gzip.open(out, "rt").read().splitlines() == want
    assert (got["v"], got["c"], got["r"], got["o1"], got["o2"]) == (v, c, r, v, len(want) - v)
    assert {"r<1": 0 <= r < 1, "r=1": r == 1 and c > 0, "c=0": r == 1 and c == 0}[kind]
    if kind == "r<1" and v:
        assert 0 < got["o2"] < c
    # the reference's log lines (PairWithNonVariants.py:36,50,64,66,68,86,90,128)
    msgs = [rec.getMessage() for rec in caplog.records if rec.name == "root"]
    want_msgs = (["Loading BED file ..."] if use_bed else []) + [
        "Counting the number of Truth Variants in %s ..." % var_fn, "%d Truth Variants" % v,
        "%d non-variants to be picked" % (v * amp), "Counting the number of usable non-variants in %s ..." % can_fn,
        "%d usable non-variant" % c, "%.2f of all non-variants are selected" % r,
        "%.2f/%.2f Truth Variants/Non-variants outputed" % (v, len(want) - v)]
    assert [m for m in msgs if not m.startswith("PairWithNonVariants: seed")] == want_msgs
    assert "PairWithNonVariants: seed 31" in msgs


def test_pair_is_repeatable_by_seed_and_by_python_seed(tmp_path):
    import random
    from clairvoyante_amd import PairWithNonVariants as pw
    var_fn, can_fn, bed_fn, _var, _can = _inputs(tmp_path, 40, 600, 4)
    outs = []
    for k, (seed, pyseed) in enumerate(((5, 0), (5, 1), (6, 0), (None, 7), (None, 7), (None, 8))):
        random.seed(pyseed)
        out = str(tmp_path / ("m%d.gz" % k))
        pw.Pair(pw.build_parser().parse_args(["--tensor_can_fn", can_fn, "--tensor_var_fn", var_fn, "--bed_fn", bed_fn,
                                              "--output_fn", out] + ([] if seed is None else ["--seed", str(seed)])))
        outs.append(gzip.open(out, "rt").read())
    assert outs[0] == outs[1] and outs[0] != outs[2] and outs[3] == outs[4] and outs[3] != outs[5]


def test_the_submodule_is_built():
    from clairvoyante_amd import __main__ as m
    assert "PairWithNonVariants" in m.SUBMODULES and "PairWithNonVariants" not in m.NOT_BUILT


# ---- the --bam_fn family of flags ---------------------------------------------------------------------------------------
def _parsers():
    from clairvoyante_amd import tensor2Bin, train
    return (("tensor2Bin", tensor2Bin.build_parser()), ("train", train.build_parser("Train Clairvoyante", bam=True)))


def test_bam_flags_give_the_sources():
    from clairvoyante_amd import utils_v2
    for _name, p in _parsers():
        a = p.parse_args(["--bam_fn", "a.bam,b.bam", "--ref_fn", "a.fa,b.fa", "--ctgName", "chr21,chr22", "--ctgStart", ",100",
                          "--ctgEnd", ",900", "--amp", "0.5", "--seed", "9", "--samtools", "native"])
        assert utils_v2.bam_sources(a) == [("a.bam", "a.fa", "chr21", None, None), ("b.bam", "b.fa", "chr22", 100, 900)]
        assert (a.amp, a.seed, a.samtools, a.candidates, a.genomeSize, a.minMQ, a.dcov) == (0.5, 9, "native", 7000000, 3000000000, 0, 250)
        a = p.parse_args(["--bam_fn", "a.bam", "--ref_fn", "a.fa", "--ctgName", "chr21"])
        assert utils_v2.bam_sources(a) == [("a.bam", "a.fa", "chr21", None, None)]


@pytest.mark.parametrize("argv", [
    ["--bam_fn", "a,b", "--ref_fn", "r", "--ctgName", "x,y"], ["--bam_fn", "a,b", "--ref_fn", "r,s", "--ctgName", "x"],
    ["--bam_fn", "a,b", "--ref_fn", "r,s", "--ctgName", "x,y", "--ctgStart", "1"],
    ["--bam_fn", "a,b", "--ref_fn", "r,s", "--ctgName", "x,y", "--ctgStart", "1,2", "--ctgEnd", "5,6,7"],
    ["--bam_fn", "a", "--ref_fn", "r", "--ctgName", "x", "--tensor_fn", "t.gz"], ["--bam_fn", "a", "--ctgName", "x"],
    ["--bam_fn", "a,", "--ref_fn", "r,s", "--ctgName", "x,y"]])
def test_bad_bam_flags_are_errors(argv, monkeypatch, capsys):
    from clairvoyante_amd import tensor2Bin, train, utils_v2
    for _name, p in _parsers():
        with pytest.raises(ValueError):
            utils_v2.bam_sources(p.parse_args(argv))
    for mod in (tensor2Bin, train):                    # the command lines refuse them before anything is loaded
        monkeypatch.setattr("sys.argv", [mod.__name__] + argv)
        with pytest.raises(SystemExit) as e:
            mod.main()
        assert e.value.code == 2 and "error:" in capsys.readouterr().err


def test_old_invocations_parse_as_before():
    from clairvoyante_amd import train, utils_v2
    for name, p in _parsers():
        a = p.parse_args(["--tensor_fn", "t.gz", "--var_fn", "v.gz", "--bed_fn", "b.bed"] + (["--bin_fn", "o.bin"] if name == "tensor2Bin" else []))
        assert (a.tensor_fn, a.var_fn, a.bed_fn, a.bam_fn) == ("t.gz", "v.gz", "b.bed", None) and utils_v2.bam_sources(a) is None
        a = p.parse_args([])
        assert (a.tensor_fn, a.var_fn, a.bed_fn) == ("vartensors", "truthvars", None) and utils_v2.bam_sources(a) is None
    # callers that hand load_dataset a bare namespace, and the parsers of the other tools, are untouched
    assert utils_v2.bam_sources(argparse.Namespace(tensor_fn="t")) is None
    assert not hasattr(train.build_parser("x").parse_args([]), "bam_fn")
