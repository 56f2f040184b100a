"""The pileup oracle (oracle/create_tensor.py) against what the reference's own CreateTensor.py wrote
for the same inputs (tests/golden/pileup/, generator: tests/golden/make_golden_pileup.py)."""
import gzip
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
G = os.path.join(HERE, "golden", "pileup")
CASES = ["plain", "region", "noleftedge", "noisy", "eqx", "handmade", "handmade_dcov1", "long", "sparse"]


def load_case(name):
    base = os.path.join(G, name)
    contigs = {}
    cur = None
    for line in open(base + ".fa"):
        if line.startswith(">"):
            cur = line[1:].split()[0]; contigs[cur] = []
        else:
            contigs[cur].append(line.strip())
    contigs = {k: "".join(v) for k, v in contigs.items()}
    sam = [l.rstrip("\n") for l in open(base + ".sam")]
    can = [l.rstrip("\n") for l in open(base + ".can")]
    opts = json.load(open(base + ".args.json"))
    want = gzip.open(base + ".tensor.gz", "rt").read().splitlines()
    return contigs, sam, can, opts, want


def norm_opts(opts):
    o = dict(opts)
    if "considerleftedge" in o:
        o["considerleftedge"] = str(o["considerleftedge"]).lower() in ("yes", "true", "t", "y", "1")
    return o


@pytest.mark.parametrize("name", CASES)
def test_oracle_rows_equal_reference_rows(name):
    from oracle import create_tensor as ct
    contigs, sam, can, opts, want = load_case(name)
    got = ct.create_tensor("ctgA", contigs["ctgA"], sam, can, **norm_opts(opts))
    assert len(want) > (40 if not name.startswith("handmade") else 5)
    assert sorted(got) == sorted(want)
    # every golden row is a distinct candidate; ours come out in ascending order
    pos = [int(r.split()[1]) for r in got]
    assert pos == sorted(pos) and len(set(pos)) == len(pos)


EVC_CASES = ["plain", "region_bed", "noisy", "lowcov", "long", "sparse", "long_region"]


def load_evc_case(name):
    meta = json.load(open(os.path.join(G, name + ".evc.args.json")))
    contigs, sam, _, _, _ = load_case(meta["alignments"])
    opts = dict(meta["options"])
    bed_rows = None
    if "bed_fn" in opts:
        bed_rows = [l.rstrip("\n") for l in open(os.path.join(G, opts.pop("bed_fn")))]
    want = gzip.open(os.path.join(G, name + ".evc.gz"), "rt").read().splitlines()
    return meta["alignments"], contigs, sam, opts, bed_rows, want


@pytest.mark.parametrize("name", EVC_CASES)
def test_candidate_oracle_rows_equal_reference_rows(name):
    from oracle import extract_candidates as ec
    _, contigs, sam, opts, bed_rows, want = load_evc_case(name)
    bed = ec.bed_intervals(bed_rows, "ctgA") if bed_rows is not None else None
    got = ec.candidates("ctgA", contigs["ctgA"], sam, bed=bed, **opts)
    assert len(want) > 30
    assert got == want                 # same rows in the same order, late rows included
