"""The labelled training set straight from BAM files (utils_v2.GetTrainingSetFromBam; csrc/cv_bamtrain.hip and the
sampling / union passes of csrc/cv_pileup.hip) against the file recipe it replaces, run through this project's own
command lines, and against the CPU oracles alone (tests/bamtrain_cases.py): total, keys, bits of X, Y -- no tolerance."""
import ctypes
import logging
import math
import os
import random
import sys
import types

import numpy as np
import pytest

import bamtrain_cases as bc
import trainset_cases as cases

pytestmark = pytest.mark.gpu
SEED = 77


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bamtrain"))
    a = bc.make_source(d, "a", "ctgA", 11)
    truth = bc.truth_rows("ctgA", a["ref"], 3, 100, extra=(900, 5900))        # 900: the BED's length-1 interval; 5900: no read
    bed = bc.bed_rows("ctgA", 6000, 900)
    w = {"d": d, "a": a, "truth": truth, "bed": bed,
         "var_fn": bc.write_rows(os.path.join(d, "var.gz"), truth), "bed_fn": bc.write_rows(os.path.join(d, "bed.gz"), bed)}
    # two contigs whose names sort differently as strings than as given
    t10, t9 = bc.make_source(d, "t10", "ctg10", 21, n_reads=450, ref_len=3000), bc.make_source(d, "t9", "ctg9", 22, n_reads=450, ref_len=3000)
    w["two"] = [t10, t9]
    w["two_truth"] = bc.truth_rows("ctg10", t10["ref"], 4, 40) + bc.truth_rows("ctg9", t9["ref"], 5, 40)
    w["two_bed"] = bc.bed_rows("ctg10", 3000, 450) + bc.bed_rows("ctg9", 3000, 450)
    w["two_var_fn"] = bc.write_rows(os.path.join(d, "var2.gz"), w["two_truth"])
    w["two_bed_fn"] = bc.write_rows(os.path.join(d, "bed2.gz"), w["two_bed"])
    # two overlapping regions of one contig
    w["lap"] = [dict(a, cs0=0, ce0=3500), dict(a, cs0=2500, ce0=6000)]
    return w


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).reshape(t.shape[0], 528).view(np.uint32)


def _build(sources, var_fn, bed_fn, amp, **kw):
    from clairvoyante_amd import utils_v2
    kw.setdefault("seed", SEED)
    kw.setdefault("shuffle", False)
    kw.setdefault("samtools", bc.FAKE)
    return utils_v2.GetTrainingSetFromBam([bc.source_tuple(s) for s in sources], var_fn, bed_fn, amp=amp, candidates=bc.CANDIDATES,
                                          genomeSize=bc.GENOME, **kw)


def _same_as_arrays(ts, arrays):
    total, _nblocks, X, Y, keys = arrays
    assert ts.route == "device" and ts.X.is_cuda and ts.Y.is_cuda
    assert ts.total == total and ts.keys() == keys
    assert np.array_equal(_bits(ts.X), X) and np.array_equal(ts.Y.cpu().numpy().astype(np.float64), Y)


def _same_as_model(ts, m):
    assert ts.route == "device"
    assert (ts.pairing["v"], ts.pairing["c"], ts.pairing["r"], ts.pairing["picked"]) == (m["v"], m["c"], m["r"], m["picked"])
    assert ts.total == len(m["keys"]) <= ts.pairing["kept"] and ts.keys() == m["keys"]          # (kept counts rows, not keys)
    assert np.array_equal(_bits(ts.X), m["X"]) and np.array_equal(ts.Y.cpu().numpy().astype(np.float64), m["Y"])


@pytest.mark.parametrize("use_bed", [True, False])
@pytest.mark.parametrize("amp", [2, 0.25, 1000])
def test_device_route_equals_the_file_recipe(world, tmp_path, amp, use_bed):
    """One source, with and without the BED.  amp = 2 and amp = 0.25 both give r < 1 on these sizes (about 1 100 / 1 650
    usable non-variants against 93 truth rows), amp = 1000 gives r = 1.  What the test asserts about its own inputs comes
    from the CPU oracles (bc.model): at amp = 2 at least 50 non-variants are kept and at least 50 dropped; amp = 0.25
    can keep only amp * v = 23 of them by its definition, so there the bound is 'some kept, at least 50 dropped'."""
    bed_fn = world["bed_fn"] if use_bed else None
    want = bc.recipe([bc.source_tuple(world["a"])], world["var_fn"], bed_fn, amp, SEED, str(tmp_path))
    ts = _build([world["a"]], world["var_fn"], bed_fn, amp)
    _same_as_arrays(ts, want["arrays"])
    p = want["pair"]
    assert (ts.pairing["v"], ts.pairing["c"], ts.pairing["r"], ts.pairing["picked"]) == (p["v"], p["c"], p["r"], p["o2"])
    assert ts.keys() == sorted(ts.keys()) and len(set(ts.keys())) == ts.total
    # the inputs cannot pass vacuously
    m = bc.model([world["a"]], world["truth"], world["bed"] if use_bed else None, amp, SEED)
    print({k: v for k, v in m.items() if k not in ("keys", "X", "Y")})
    assert m["truth_kept"] >= 30 and m["truth_without_row"] >= 1 and m["sampled_at_truth"] >= 1 and m["centres_at_N"] >= 1
    assert (m["truth_outside_bed"] >= 1) == use_bed
    assert (m["r"] < 1) == (amp != 1000) and ts.pairing["r"] == m["r"]
    if amp == 2:
        assert m["nonvariants_kept"] >= 50 and m["nonvariants_dropped"] >= 50
    elif amp == 0.25:
        assert m["nonvariants_kept"] >= 1 and m["nonvariants_dropped"] >= 50
    else:
        assert m["nonvariants_kept"] >= 50 and m["nonvariants_dropped"] == 0
    assert ("ctgA:900" in ts.keys()) and "ctgA:5900" not in ts.keys()       # the length-1 interval keeps 900; no read reaches 5900


@pytest.mark.parametrize("amp,use_bed", [(2, True), (0.25, False)])
def test_device_route_equals_the_cpu_oracles(world, amp, use_bed):
    """sampled positions from oracle.extract_candidates filtered by the stream-0 draws, tensors from
    oracle.create_tensor, pairing and labels restated: nothing of the expectation ran on the GPU"""
    m = bc.model([world["a"]], world["truth"], world["bed"] if use_bed else None, amp, SEED)
    _same_as_model(_build([world["a"]], world["var_fn"], world["bed_fn"] if use_bed else None, amp), m)


def test_sampling_and_union_on_the_handle(world):
    """cv_pileup_sample_candidates = the select at threshold 0 / minCoverage 0 filtered by the draws (get_extracted keeps
    working on it); cv_pileup_adopt_union = the sorted unique union with its flags"""
    from clairvoyante_amd import draws
    from clairvoyante_amd.pileup import Pileup
    a = world["a"]
    text = ("\n".join(a["lines"]) + "\n").encode()
    pl = Pileup(evc=True, retain=True, contig="ctgA")
    pl.set_reference(a["ref"], 0)
    pl.add_sam(text, final=True)
    full = pl.extract_candidates(0, 0)
    assert full["late"].sum() > 0
    n = pl.sample_candidates(SEED, bc.PROB)
    got = pl.extracted()
    keep = ~(draws.draws(SEED, draws.SAMPLE, "ctgA", full["pos0"] + 1, full["late"]) > bc.PROB)
    assert 0.25 * len(keep) < n == int(keep.sum()) < 0.35 * len(keep)
    for k in ("pos0", "late", "counts"):
        assert np.array_equal(got[k], full[k][keep])
    assert got["late"].sum() > 0 and (got["reads"], got["last_pos"]) == (full["reads"], full["last_pos"])
    truth = np.array(sorted(set([5, 40, 41, 2000, 5999] + [int(p) + 1 for p in got["pos0"][:7]])), dtype=np.int64)
    lo, hi = 30, 5000
    pl.adopt_union(truth, lo, hi)
    centres = np.zeros(pl.n, dtype=np.int64)
    cnt = ctypes.c_int64(0)
    from clairvoyante_amd import _lib
    _lib.check(pl.lib.cv_pileup_get_candidates(pl.h, centres.ctypes.data_as(ctypes.c_void_p), pl.n, ctypes.byref(cnt)))
    sampled = set(int(p) + 1 for p in got["pos0"] if lo <= p + 1 <= hi)
    assert centres.tolist() == sorted(sampled | set(truth.tolist()))
    _x, depth, touched = pl.finish(subtract=True)
    col = pl.columns(depth, touched)
    flags = col["cflag"].cpu().numpy()
    assert np.array_equal(flags & 1, np.isin(centres, truth).astype(np.uint8))
    assert np.array_equal(flags >> 1, np.array([c in sampled for c in centres.tolist()], dtype=np.uint8))
    assert np.array_equal(col["pos"].cpu().numpy(), centres)
    assert np.array_equal(col["digits"].cpu().numpy(), np.array([len(str(c)) for c in centres.tolist()], dtype=np.uint8))
    base = [a["ref"][c - 1].upper() for c in centres.tolist()]
    assert np.array_equal(col["acgt"].cpu().numpy(), np.array([b in "ACGT" for b in base], dtype=np.uint8))
    assert np.array_equal(col["centre"].cpu().numpy(), np.array(["ACGT".find(b) & 255 for b in base], dtype=np.uint8))
    row = col["row"].cpu().numpy().astype(bool)
    assert np.array_equal(row, touched.cpu().numpy() & (centres - 17 >= 0)) and not row[centres.tolist().index(5)] and row.sum() > 100
    pl.close()


@pytest.mark.parametrize("case", ["two_contigs", "overlap"])
def test_several_sources_are_paired_together(world, tmp_path, case):
    """ctg10 before ctg9 as given, behind it as a string; two overlapping regions of one contig, whose shared positions
    arrive twice (v counts both rows, the set holds the later one)"""
    if case == "two_contigs":
        srcs, truth, bed, var_fn, bed_fn = world["two"], world["two_truth"], world["two_bed"], world["two_var_fn"], world["two_bed_fn"]
    else:
        srcs, truth, bed, var_fn, bed_fn = world["lap"], world["truth"], world["bed"], world["var_fn"], world["bed_fn"]
    want = bc.recipe([bc.source_tuple(s) for s in srcs], var_fn, bed_fn, 2, SEED, str(tmp_path))
    ts = _build(srcs, var_fn, bed_fn, 2)
    _same_as_arrays(ts, want["arrays"])
    p = want["pair"]
    assert (ts.pairing["v"], ts.pairing["c"], ts.pairing["r"], ts.pairing["picked"]) == (p["v"], p["c"], p["r"], p["o2"])
    keys = ts.keys()
    assert keys == sorted(keys) and len(set(keys)) == len(keys) > 100
    m = bc.model(srcs, truth, bed, 2, SEED)
    _same_as_model(ts, m)
    if case == "two_contigs":
        names = [k.split(":")[0] for k in keys]
        assert names.index("ctg9") > names.index("ctg10") and set(names) == {"ctg10", "ctg9"}
        single = [_build([s], var_fn, bed_fn, 2).pairing for s in srcs]
        assert ts.pairing["v"] == single[0]["v"] + single[1]["v"] and ts.pairing["c"] == single[0]["c"] + single[1]["c"]
        assert ts.pairing["r"] not in (single[0]["r"], single[1]["r"])          # r is one figure over all sources
    else:
        in_both = [k for k in keys if 2501 <= int(k.split(":")[1]) <= 3500]
        assert len(in_both) > 10
        assert m["v"] > len(set(r[1] for r in truth))                           # truth rows of the shared stretch count twice


def test_the_result_does_not_depend_on_how_the_reads_arrive(world, tmp_path, monkeypatch):
    """the SAM pipe, --samtools native on the host BAM route and on the device BAM route: the same set"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bam_writer import write_bam
    from clairvoyante_amd import pileup
    a = world["a"]
    bam = str(tmp_path / "a.bam")
    write_bam(bam, a["lines"], [("ctgA", 6000)], block_payload=9001)
    for region in ((None, None), (1000, 4000)):
        s = dict(a, cs0=region[0], ce0=region[1])
        pipe = _build([s], world["var_fn"], world["bed_fn"], 2)
        assert pipe.total > 50
        for route in ("host", "device"):
            monkeypatch.setenv("CV_BAM_DECODE", route)
            before = pileup.bam_decode_counts()
            ts = _build([dict(s, sam=bam)], world["var_fn"], world["bed_fn"], 2, samtools="native")
            after = pileup.bam_decode_counts()
            assert after[route + "_views"] == before[route + "_views"] + 1
            assert ts.total == pipe.total and ts.keys() == pipe.keys() and ts.pairing == pipe.pairing
            assert np.array_equal(_bits(ts.X), _bits(pipe.X)) and np.array_equal(_bits16(ts.Y), _bits16(pipe.Y))


def _bits16(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def test_shuffle_and_seeds(world):
    from clairvoyante_amd import utils_v2
    args = ([world["a"]], world["var_fn"], world["bed_fn"], 2)
    plain = _build(*args)
    random.seed(7)
    perm = utils_v2.shuffled_indices(plain.total)
    random.seed(7)
    ts = _build(*args, shuffle=True)
    assert ts.total == plain.total and ts.keys() == [plain.keys()[p] for p in perm] and ts.keys() != plain.keys()
    assert np.array_equal(_bits(ts.X), _bits(plain.X)[perm]) and np.array_equal(_bits16(ts.Y), _bits16(plain.Y)[perm])
    again = _build(*args)
    assert again.keys() == plain.keys() and np.array_equal(_bits(again.X), _bits(plain.X)) and again.pairing == plain.pairing
    other = _build(*args, seed=SEED + 1)
    assert other.keys() != plain.keys() and other.pairing["v"] == plain.pairing["v"]
    assert abs(other.pairing["sampled"] - plain.pairing["sampled"]) < 0.15 * plain.pairing["sampled"] and plain.pairing["sampled"] > 1000
    # without a seed: one draw from Python's generator per call, so random.seed(k) repeats the run
    random.seed(3)
    s1 = _build(*args, seed=None)
    random.seed(3)
    s2 = _build(*args, seed=None)
    assert s1.seed == s2.seed and s1.keys() == s2.keys() and s1.seed != SEED


def _cli(world, extra):
    a = world["a"]
    return ["--bam_fn", a["sam"], "--ref_fn", a["fa"], "--ctgName", "ctgA", "--var_fn", world["var_fn"], "--bed_fn", world["bed_fn"],
            "--candidates", str(bc.CANDIDATES), "--genomeSize", str(bc.GENOME), "--seed", str(SEED), "--samtools", bc.FAKE] + extra


def test_tensor2bin_from_bam(world, tmp_path):
    from clairvoyante_amd import tensor2Bin, utils_v2
    want = bc.recipe([bc.source_tuple(world["a"])], world["var_fn"], world["bed_fn"], 2, SEED, str(tmp_path))["arrays"]
    perm_seed = 5
    random.seed(perm_seed)
    perm = utils_v2.shuffled_indices(want[0])
    out = str(tmp_path / "t.bin")
    random.seed(perm_seed)
    tensor2Bin.Run(tensor2Bin.build_parser().parse_args(_cli(world, ["--bin_fn", out])))
    got = cases.arrays_of(utils_v2.LoadBin(out))
    assert got[:2] == want[:2] and got[4] == [want[4][p] for p in perm]
    assert np.array_equal(got[2], want[2][perm]) and np.array_equal(got[3], want[3][perm])


def test_train_from_bam_keeps_the_set_resident(world, monkeypatch, caplog):
    from clairvoyante_amd import param, train, utils_v2
    monkeypatch.setattr(param, "trainBatchSize", 64)
    monkeypatch.setattr(param, "predictBatchSize", 16)
    monkeypatch.setattr(param, "maxEpoch", 3)                                  # epochs 1 and 2
    sets, packed, build, pack = [], [], utils_v2.GetTrainingSetFromBam, utils_v2.pack_array

    def spy(*a, **kw):
        sets.append(build(*a, **kw))
        return sets[-1]
    monkeypatch.setattr(utils_v2, "GetTrainingSetFromBam", spy)
    monkeypatch.setattr(utils_v2, "pack_array", lambda *a, **kw: packed.append(1) or pack(*a, **kw))
    args = train.build_parser("Train Clairvoyante", bam=True).parse_args(_cli(world, ["--slim", "--learning_rate", "1e-3"]))
    random.seed(11)
    with caplog.at_level(logging.INFO):
        train.Run(args)
    assert len(sets) == 1 and sets[0].route == "device" and sets[0].total > 200 and packed == []
    loss = [float(r.getMessage().split()[3]) for r in caplog.records if " Training loss: " in r.getMessage()]
    print("training loss per epoch", loss)
    assert len(loss) == 2 and all(math.isfinite(v) for v in loss) and loss[1] < loss[0]


def test_a_set_that_would_not_fit_is_refused_before_anything_is_allocated(world, monkeypatch):
    from clairvoyante_amd import _lib, pileup, utils_v2
    monkeypatch.setattr(utils_v2, "TRAINSET_FREE_BYTES", 1 << 20)

    def no_pileup(*a, **kw):
        raise AssertionError("a Pileup was made")
    monkeypatch.setattr(pileup, "Pileup", no_pileup)
    monkeypatch.setattr(utils_v2, "_BamTrainsetBuilder", no_pileup)
    with pytest.raises(_lib.CvError) as e:
        _build([world["a"]], world["var_fn"], world["bed_fn"], 2)
    assert "would not fit into half of the free device memory" in str(e.value) and str(1 << 20) in str(e.value)


def test_an_empty_region_gives_an_empty_set(world, tmp_path):
    from clairvoyante_amd import tensor2Bin, utils_v2
    s = dict(world["a"], cs0=5800, ce0=5850)                                   # no read, no truth row
    ts = _build([s], world["var_fn"], world["bed_fn"], 2)
    assert ts.route == "device" and ts.total == 0 and ts.keys() == [] and tuple(ts.X.shape) == (0, 33, 4, 4)
    assert ts.pairing == {"v": 0, "c": 0, "r": 1.0, "picked": 0, "kept": 0, "sampled": 0}
    out = str(tmp_path / "e.bin")
    a = world["a"]
    tensor2Bin.Run(tensor2Bin.build_parser().parse_args(_cli(world, ["--ctgStart", "5800", "--ctgEnd", "5850", "--bin_fn", out])))
    assert cases.arrays_of(utils_v2.LoadBin(out))[:2] == (0, 1)
