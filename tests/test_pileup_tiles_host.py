"""CPU side of tests/test_gpu_pileup_tiles.py: the restatement of the tile rule (tests/pileup_tile_cases.py) is tied to
the constants of csrc/cv_pileup.hip, and the inputs of the GPU tests are shown to reach the code path they are for --
the columns the column kernels book straight in HBM, outside the window their tile keeps in LDS.  The shares are
conditions on the inputs (at least half, at least 1 000), not measurements of them."""
import pytest

import bamtrain_cases as bc
import pileup_tile_cases as P


def test_constants_are_the_ones_of_the_source():
    got = P.source_constants()
    assert got == {"SC_SEGS": P.SC_SEGS, "SC_CANDS": P.SC_CANDS, "EVC_SEGS": P.EVC_SEGS, "EVC_WIN": P.EVC_WIN}


def test_segments_restate_emit_on_hand_made_records():
    """runs of 64, 65 and 130 columns, an insertion (all its pieces at the position it precedes), a deletion, N / H / P
    that move nothing, a clipped-only record, the per-POS depth cap, a read neither pass takes"""
    recs = [
        "a\t0\tctgA\t11\t60\t3S64M2I65M\t*\t0\t0\t" + "A" * 134 + "\t*",
        "b\t0\tctgA\t11\t60\t130D1M\t*\t0\t0\tC\t*",
        "c\t0\tctgA\t11\t60\t2M3N2H1P70I2M\t*\t0\t0\t" + "G" * 74 + "\t*",
        "d\t0\tctgA\t40\t60\t8S\t*\t0\t0\tACGTACGT\t*",
        "e\t0\tctgA\t50\t2\t5M\t*\t0\t0\tACGTA\t*",
        "f\t0\tother\t60\t60\t5M\t*\t0\t0\tACGTA\t*",
    ]
    sg = P.segments(recs, minMQ=3, dcov=2, evc_minMQ=3)
    rows = list(zip(sg["type"].tolist(), sg["r0"].tolist(), sg["n"].tolist(), sg["first"].tolist(), sg["pos"].tolist(),
                    sg["ct"].tolist(), sg["evc"].tolist(), sg["q0"].tolist()))
    M, I, D = P.T_MATCH, P.T_INS, P.T_DEL
    assert rows == [
        (M, 10, 64, True, 10, True, True, 3), (I, 74, 2, True, 10, True, True, 67), (M, 74, 64, True, 10, True, True, 69),
        (M, 138, 1, False, 10, True, True, 133),
        (D, 10, 64, True, 10, True, True, 0), (D, 74, 64, False, 10, True, True, 0), (D, 138, 2, False, 10, True, True, 0),
        (M, 140, 1, True, 10, True, True, 134),
        # the third read of POS 11 under dcov 2: the tensor pass drops it, its segments stay for the candidate pass
        (M, 10, 2, True, 10, False, True, 135), (I, 12, 64, True, 10, False, True, 137), (I, 12, 6, False, 10, False, True, 201),
        (M, 12, 2, True, 10, False, True, 207),
        # d: nothing aligned, no segment (its SEQ bytes are kept); e: below both mapping qualities, no segment; f: the tensor pass only
        (M, 59, 5, True, 59, True, False, 217),
    ]
    assert len(sg["seq"]) == 134 + 1 + 74 + 8 + 5


@pytest.mark.parametrize("name", ["long", "sparse", "mix"])
def test_segments_agree_with_the_restatement_of_the_device_bam_reader(name):
    """the other restatement of emit / parse_bam_record in the suite, bam_device_cases.py_parse, works on BAM records:
    every read of the input encoded as one, cut by both, gives the same segments and the same SEQ bytes (py_parse knows
    no running state and marks the opening insertion / deletion runs F_LATE, which this helper leaves out: no depth cap
    here, that bit masked)"""
    import bam_device_cases as C
    import bam_writer
    _ref, lines = P.inputs(name)
    sg = P.segments(lines)
    assert sg["ct"].all() and sg["evc"].any()
    at, base, n_long = 0, 0, 0
    for line in lines:
        blob = bam_writer.encode_record(line.split("\t"), {"ctgA": 0})[0]
        got = C.py_parse(blob, 4, (0, 1, 0, 1), base)
        assert got[0] == C.C_READ
        _what, pos, rf, _leading, cols, segs, seq = got
        k = len(segs)
        mine = [(int(sg["r0"][i]), int(sg["q0"][i]),
                 int(sg["n"][i]) | (int(sg["type"][i]) << 8) | C.F_CT | (C.F_EVC if sg["evc"][i] else 0) | (C.F_FIRST if sg["first"][i] else 0),
                 int(sg["pos"][i])) for i in range(at, at + k)]
        assert mine == [(r0, q0, info & ~C.F_LATE, p) for r0, q0, info, _adv0, p in segs]
        assert bool(rf & C.F_EVC) == bool(sg["evc"][at]) if k else True
        assert int(sg["n"][at:at + k].sum()) == cols and bytes(sg["seq"][base:base + len(seq)]) == seq
        at += k; base += len(seq); n_long += k > 300
    assert at == len(sg["n"]) and base == len(sg["seq"]) and (n_long > 0 or name == "sparse")


@pytest.mark.parametrize("name", ["long", "sparse"])
def test_new_cases_book_most_candidate_pass_columns_outside_the_window(name):
    _ref, lines = P.golden_alignments(name)
    e = P.evc_paths(P.segments(lines))
    print(name, e, "share outside %.3f" % (e["outside"] / float(e["inside"] + e["outside"])))
    assert e["tiles"] > 1 and e["inside"] > 1000
    assert 2 * e["outside"] >= e["inside"] + e["outside"]


def test_the_mix_and_the_slices_reach_both_paths_and_the_bounds_test():
    """the short-read stack under one 9 000-base read; and, per input, the reference slice of the GPU test: bookings of
    BOTH paths fall off BOTH ends of it"""
    for name in sorted(P.SLICES):
        _ref, lines = P.inputs(name)
        cs0, ce0 = P.SLICES[name]
        view = bc._view(lines, "ctgA", cs0 + 1, ce0)
        first, length = cs0 + 1, ce0 - cs0
        e = P.evc_paths(P.segments(view), first, length)
        print(name, e)
        assert e["outside"] >= 1000 and e["inside"] >= 1000
        assert e["outside_off_slice"] >= 500 and e["outside"] - e["outside_off_slice"] >= 500
        assert e["inside_off_slice"] >= 1
        sg = P.segments(view)
        r = sg["r0"][sg["evc"]]
        assert (r < first).any() and (r + sg["n"][sg["evc"]] > first + length).any()


@pytest.mark.parametrize("left,dcov", [(True, 250), (False, 250), (True, 2), (False, 2)])
def test_dense_centres_overflow_the_forty_candidates(left, dcov):
    ref, lines = P.golden_alignments("long")
    s = P.scatter_paths(P.segments(lines, dcov=dcov), P.dense_centres(len(ref)), left)
    print(left, dcov, s)
    assert s["outside"] >= 1000 and s["inside"] >= 1000


def test_the_old_random_shape_never_leaves_the_window():
    """a record of the gap: the shape test_extract_candidates_equals_oracle_on_random_alignments uses, with its filters,
    has not one candidate-pass column outside the window of its tile"""
    from clairvoyante_amd import synth_pileup as sp
    for seed, prof in ((21, sp.DEFAULT_PROFILE), (22, sp.NOISY_PROFILE)):
        _ref, lines = sp.make_alignments(seed=700 + seed, profile=prof, **P.OLD_RANDOM_SHAPE)
        e = P.evc_paths(P.segments(lines, minMQ=1 << 30, evc_minMQ=5))
        assert e["outside"] == 0 and e["inside"] > 100000 and e["tiles"] > 10
