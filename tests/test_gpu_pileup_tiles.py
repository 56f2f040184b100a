"""The column kernels of csrc/cv_pileup.hip on long reads and sparse coverage, where most columns leave the window of
counters their tile keeps in LDS and are booked straight in HBM (tests/pileup_tile_cases.py; the CPU side,
tests/test_pileup_tiles_host.py, shows that these inputs do).  Everything is compared with the CPU oracles
(oracle/extract_candidates.py, oracle/create_tensor.py, themselves pinned on `long` and `sparse` by the reference's own
rows, tests/test_pileup_oracle.py) with row equality or np.array_equal: the counters are integers."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, ".."))
import bam_device_cases as C  # noqa: E402
import bamtrain_cases as bc  # noqa: E402
import pileup_tile_cases as P  # noqa: E402
from test_gpu_pileup import oracle_arrays  # noqa: E402

pytestmark = pytest.mark.gpu
THR, MINCOV = 0.05, 1
FUSED_RANGE = (2000, 5000)            # adopt_candidates(lo1, hi1) of the fused legs: about 1 200 centres
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def text_of(lines):
    return ("\n".join(lines) + "\n").encode()


def oracle_rows(name):
    from oracle import extract_candidates as ec
    ref, lines = P.inputs(name)
    return memo(("rows", name), lambda: ec.candidates("ctgA", ref, lines, minCoverage=MINCOV, threshold=THR))


def candidate_pass(ref, first0, lines, chunk=None, threads=1, region=None):
    """the candidate pass alone (the tensor pass switched off, as ExtractVariantCandidates runs it) -> what
    extract_candidates gives"""
    from clairvoyante_amd.pileup import Pileup
    pl = Pileup(evc=True, contig="ctgA", minMQ=1 << 30, threads=threads)
    pl.set_reference(ref, first0)
    text = text_of(lines)
    step = chunk or len(text)
    for s in range(0, len(text), step):
        pl.add_sam(text[s:s + step])
    res = pl.extract_candidates(THR, MINCOV, region)
    pl.close()
    return res


@pytest.mark.parametrize("name", ["long", "sparse", "mix"])
def test_candidate_pass_equals_the_oracle(name):
    """one piece and 30 011-byte pieces, `threads` 1 and 5: the rows of oracle.extract_candidates, in its order.  (The
    parser takes a second thread only from 1 MiB of text on, cv_pileup_add_sam; these inputs are below 200 KB, so
    `threads` = 5 sets the option and parses on one thread.  What several threads do to the result is
    test_gpu_pileup.test_parser_thread_count_does_not_change_the_result's subject.)"""
    from clairvoyante_amd.ExtractVariantCandidates import candidate_rows
    ref, lines = P.inputs(name)
    want = oracle_rows(name)
    assert len(want) > 500
    for chunk, threads in ((None, 1), (30011, 5), (None, 5), (30011, 1)):
        res = candidate_pass(ref, 0, lines, chunk, threads)
        assert candidate_rows("ctgA", res, ref.encode(), 0) == want, (chunk, threads)


@pytest.mark.parametrize("name", sorted(P.SLICES))
def test_candidate_pass_on_a_reference_slice_the_reads_overhang(name):
    """the reference loaded as exactly the positions the region test lets through: every booking in front of the slice
    (ri < 0) and behind it (ri >= ref_len) must vanish, from the LDS window and from the HBM path alike, and every one
    inside must count -- the oracle's rows of that region, whose first and last positions are the slice's"""
    from clairvoyante_amd.ExtractVariantCandidates import candidate_rows
    from oracle import extract_candidates as ec
    ref, lines = P.inputs(name)
    cs0, ce0 = P.SLICES[name]
    want = ec.candidates("ctgA", ref, lines, cs0, ce0, 0, MINCOV, THR)
    view = bc._view(lines, "ctgA", cs0 + 1, ce0)
    first0, sl = cs0 + 1, ref[cs0 + 1:ce0 + 1]
    for chunk in (None, 30011):
        res = candidate_pass(sl, first0, view, chunk, region=(cs0 + 1, ce0))
        assert candidate_rows("ctgA", res, sl.encode(), first0) == want
    pos = [int(r.split()[1]) for r in want]
    assert min(pos) == first0 + 1 and max(pos) == first0 + len(sl) and len(want) > 300


def run_tensors(ref, first0, lines, centers, chunk=None, **kw):
    from clairvoyante_amd.pileup import Pileup
    pl = Pileup(**kw)
    pl.set_reference(ref, first0)
    pl.set_candidates(centers)
    text = text_of(lines)
    step = chunk or len(text)
    for s in range(0, len(text), step):
        pl.add_sam(text[s:s + step])
    t, d, u = pl.finish()
    out = (t.cpu().numpy(), d.cpu().numpy(), u.cpu().numpy())
    pl.close()
    return out


@pytest.mark.parametrize("left,dcov", [(True, 250), (False, 250), (True, 2), (False, 2)])
def test_tensors_on_long_reads_with_dense_centres_equal_the_oracle(left, dcov):
    """every third position and every position of a 1 kbp stretch: candidate 41 onwards of a tile, in HBM"""
    ref, lines = P.inputs("long")
    centers = P.dense_centres(len(ref))
    To, Do, Uo = oracle_arrays(ref, lines, centers, 0, dcov, left)
    T, D, U = run_tensors(ref, 0, lines, centers, chunk=30011, minMQ=0, dcov=dcov, considerleftedge=left)
    assert np.array_equal(U, Uo)
    assert np.array_equal(D[U], Do[U])
    assert np.array_equal(T, To)
    assert U.sum() > 1500 and T.sum() > 100000


def fused_want():
    """the oracle's two steps on `long`: candidate rows -> the tensors of their positions inside FUSED_RANGE"""
    def make():
        ref, lines = P.inputs("long")
        rows = oracle_rows("long")
        centers = np.asarray(sorted(set(p for p in (int(r.split()[1]) for r in rows) if FUSED_RANGE[0] <= p <= FUSED_RANGE[1])),
                             dtype=np.int64)
        return (rows, centers) + oracle_arrays(ref, lines, centers, 0, 250, True)
    return memo("fused", make)


def fused(pl, feed):
    """evc + retain on one handle: feed(pl), extract, adopt, finish -> (rows, centres, T, D, U)"""
    from clairvoyante_amd.ExtractVariantCandidates import candidate_rows
    ref, _lines = P.inputs("long")
    pl.set_reference(ref, 0)
    feed(pl)
    res = pl.extract_candidates(THR, MINCOV)
    centers = pl.adopt_candidates(*FUSED_RANGE)
    t, d, u = pl.finish()
    return candidate_rows("ctgA", res, ref.encode(), 0), centers.copy(), t.cpu().numpy(), d.cpu().numpy(), u.cpu().numpy()


def same_as_fused_want(got):
    rows, centers, T, D, U = fused_want()
    assert got[0] == rows
    assert np.array_equal(got[1], centers) and len(centers) > 1000
    assert np.array_equal(got[4], U) and np.array_equal(got[3][U], D[U]) and np.array_equal(got[2], T)


@pytest.mark.parametrize("flush", [False, True])
def test_fused_route_on_long_reads_equals_the_oracles_two_steps(flush):
    """evc + retain + adopt_candidates + finish; with an explicit cv_pileup_flush in the middle the retained alignments
    are two batches, whose tiles differ from the one batch's"""
    from clairvoyante_amd import _lib
    from clairvoyante_amd.pileup import Pileup
    _ref, lines = P.inputs("long")

    def feed(pl):
        if not flush:
            pl.add_sam(text_of(lines))
            return
        half = len(lines) // 2
        pl.add_sam(text_of(lines[:half]))
        _lib.check(pl.lib.cv_pileup_flush(pl.h, pl._stream()))
        pl.add_sam(text_of(lines[half:]))
    pl = Pileup(evc=True, retain=True, contig="ctgA")
    got = fused(pl, feed)
    pl.close()
    same_as_fused_want(got)


def _bam_of(tmp_path, lines, ref_len, name="long.bam"):
    bam = str(tmp_path / name)
    C.write_bam(bam, lines, [("ctgA", ref_len), ("other", 10)], block_payload=20000)
    return bam


@pytest.mark.parametrize("route", ["text", "host", "device"])
def test_three_feeds_of_the_long_reads_equal_the_oracle(tmp_path, route):
    """SAM text, BAM records on host threads, BAM on the device: each against the oracle.  The device takes all of it:
    it refuses a slab only for a walker that misses its anchor, a bad block_size or record layout, a placeholder CIGAR
    (more than 65 535 operations, the real ones in the CG tag), POS or CIGAR demands outside what parse_bam_record
    accepts, or slab sums of 2^32 SEQ bytes / 2^31 segments; these records have at most 970 operations."""
    from clairvoyante_amd import pileup
    from clairvoyante_amd.bam import BamFile
    ref, lines = P.inputs("long")
    bam = _bam_of(tmp_path, lines, len(ref))
    pileup.bam_decode_counts(reset=True)

    def feed(pl):
        bf = BamFile(bam, threads=3)
        if route == "text":
            for chunk in bf.view("ctgA", None, None, chunk=1 << 20):
                pl.add_sam(chunk)
        else:
            pl.add_bam(bf, "ctgA", None, None, window=1 << 20, route=route)
        bf.close()
    pl = pileup.Pileup(evc=True, retain=True, contig="ctgA", threads=3)
    got = fused(pl, feed)
    kept = pl.reads_kept
    pl.close()
    cnt = pileup.bam_decode_counts(reset=True)
    print(route, cnt)
    same_as_fused_want(got)
    assert kept == len(lines)
    if route == "device":
        from test_gpu_bam_device import clean
        clean(cnt)
        assert cnt["device_records"] == len(lines)
    elif route == "host":
        assert cnt["host_views"] == 1 and cnt["device_views"] == 0


def test_training_set_from_long_reads_equals_the_cpu_oracles(tmp_path):
    """GetTrainingSetFromBam on one long-read source against bamtrain_cases.model, the definition from the CPU oracles"""
    from clairvoyante_amd import synth_pileup as sp
    from clairvoyante_amd import utils_v2
    d = str(tmp_path)
    s = bc.make_source(d, "L", "ctgA", 31, ref_len=5000, n_reads=14, read_len=(2500, 7000), profile=sp.NOISY_PROFILE)
    e = P.evc_paths(P.segments(s["lines"]))
    assert e["outside"] > e["inside"] > 1000
    truth = bc.truth_rows("ctgA", s["ref"], 3, 60, extra=(900,))
    bed = bc.bed_rows("ctgA", 5000, 900)
    var_fn, bed_fn = bc.write_rows(os.path.join(d, "var.gz"), truth), bc.write_rows(os.path.join(d, "bed.gz"), bed)
    m = bc.model([s], truth, bed, 2, 77)
    assert m["truth_kept"] >= 30 and m["nonvariants_kept"] >= 50 and m["nonvariants_dropped"] >= 50 and m["r"] < 1
    ts = utils_v2.GetTrainingSetFromBam([bc.source_tuple(s)], var_fn, bed_fn, amp=2, candidates=bc.CANDIDATES, genomeSize=bc.GENOME,
                                        seed=77, shuffle=False, samtools=bc.FAKE)
    assert ts.route == "device"
    assert (ts.pairing["v"], ts.pairing["c"], ts.pairing["r"], ts.pairing["picked"]) == (m["v"], m["c"], m["r"], m["picked"])
    assert ts.total == len(m["keys"]) and ts.keys() == m["keys"]
    X = np.ascontiguousarray(ts.X.cpu().numpy()).reshape(ts.total, 528).view(np.uint32)
    assert np.array_equal(X, m["X"]) and np.array_equal(ts.Y.cpu().numpy().astype(np.float64), m["Y"])


# ---- chromosome-scale coordinates: metamorphic, no oracle run -----------------------------------------------------------
K_CHROMOSOME = 248000000              # the length of human chromosome 1
K_LIMIT = 2100000000                  # inside parse_record's 2^31 - 2^24, beyond what a .bai can index (2^29)


def shifted(lines, k):
    out = []
    for l in lines:
        f = l.split("\t")
        f[3] = str(int(f[3]) + k)
        out.append("\t".join(f))
    return out


def both_passes(ref, first0, feed, centers, region):
    """on one input: the candidate pass inside `region` with the fused tensors behind it, and the tensor pass for
    `centers` -> arrays, positions first"""
    from clairvoyante_amd.pileup import Pileup
    pl = Pileup(evc=True, retain=True, contig="ctgA", threads=3)
    pl.set_reference(ref, first0)
    feed(pl)
    res = pl.extract_candidates(THR, MINCOV, region)
    adopted = pl.adopt_candidates(region[0], region[1])
    t, d, u = pl.finish()
    a = [res["pos0"], adopted.copy(), np.int64(res["last_pos"]), res["late"], res["counts"], np.int64(res["reads"]),
         t.cpu().numpy(), d.cpu().numpy(), u.cpu().numpy()]
    pl.close()
    pl = Pileup(dcov=2, considerleftedge=False, threads=3)
    pl.set_reference(ref, first0)
    pl.set_candidates(centers)
    feed(pl)
    t, d, u = pl.finish()
    a += [t.cpu().numpy(), d.cpu().numpy(), u.cpu().numpy()]
    pl.close()
    return a


def unshifted():
    def make():
        ref, lines = P.inputs("long")
        return both_passes(ref, 0, lambda pl: pl.add_sam(text_of(lines)), P.dense_centres(len(ref))[::2], FUSED_RANGE)
    return memo("unshifted", make)


def same_but_shifted(got, k):
    want = unshifted()
    assert len(want[0]) > 1000 and len(want[1]) > 1000 and want[8].sum() > 1000 and want[11].sum() > 500
    for i in range(3):
        assert np.array_equal(got[i], want[i] + k), i                # positions: every one + K
    for i in range(3, len(want)):
        assert np.array_equal(got[i], want[i]), i                    # counts and tensors: bit for bit


@pytest.mark.parametrize("k", [K_CHROMOSOME, K_LIMIT])
def test_text_feed_at_chromosome_scale_coordinates(k):
    """every POS, first_pos0, the centres and the region + K: the unshifted result (which the tests above hold to the
    oracle) with every position + K"""
    ref, lines = P.inputs("long")
    text = text_of(shifted(lines, k))

    def feed(pl):
        for s in range(0, len(text), 30011):
            pl.add_sam(text[s:s + 30011])
    got = both_passes(ref, k, feed, P.dense_centres(len(ref))[::2] + k, (FUSED_RANGE[0] + k, FUSED_RANGE[1] + k))
    same_but_shifted(got, k)


@pytest.mark.parametrize("route", ["host", "device"])
def test_bam_feeds_at_chromosome_scale_coordinates(tmp_path, route):
    from clairvoyante_amd import pileup
    from clairvoyante_amd.bam import BamFile
    k = K_CHROMOSOME
    ref, lines = P.inputs("long")
    bam = _bam_of(tmp_path, shifted(lines, k), k + len(ref), "shifted.bam")
    pileup.bam_decode_counts(reset=True)

    def feed(pl):
        bf = BamFile(bam, threads=3)
        pl.add_bam(bf, "ctgA", None, None, window=1 << 20, route=route)
        bf.close()
    got = both_passes(ref, k, feed, P.dense_centres(len(ref))[::2] + k, (FUSED_RANGE[0] + k, FUSED_RANGE[1] + k))
    cnt = pileup.bam_decode_counts(reset=True)
    print(route, cnt)
    same_but_shifted(got, k)
    if route == "device":
        assert cnt["device_views"] == 2 and cnt["handed_over_slabs"] == 0 and cnt["host_members"] == 0
        assert cnt["device_records"] == 2 * len(lines)
