"""Development probe: the labelled training set from a BAM -- the file recipe of dataPrepScripts/PrepDataBeforeDemo.sh run
with this project's own command lines against utils_v2.GetTrainingSetFromBam, on synthetic coordinate-sorted BAMs
written by tests/bam_writer.py (150 bp reads at ~30x, one truth row per 1 000 bp, a BED over two thirds of the contig,
the recipe's own sampling rate 2 * 7 000 000 / 3 000 000 000).

  python tools/gpu_bam_trainset_probe.py [rungs=20000,200000,2000000] [reps=5] [seed=1]

Per rung, after asserting that the routes give the same set, the median of `reps` runs of
  recipe    ExtractVariantCandidates --gen4Training --seed, CreateTensor twice, PairWithNonVariants --seed, tensor2Bin
  bin       tensor2Bin --bam_fn
  resident  GetTrainingSetFromBam(...).resident()
all with --samtools native, the seconds per phase of the device route, and the HIP-event times of the new kernels beside
evc_count / pileup_scatter."""
import argparse
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def opt(name, default):
    for a in sys.argv[1:]:
        if a.startswith(name + "="):
            return a.split("=", 1)[1]
    return default


def main():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import bamtrain_cases as bc
    import trainset_cases as cases
    from bam_writer import write_bam
    from clairvoyante_amd import CreateTensor, ExtractVariantCandidates, PairWithNonVariants, synth_pileup, tensor2Bin, utils_v2
    rungs = [int(x) for x in opt("rungs", "20000,200000,2000000").split(",") if x]
    reps, seed = int(opt("reps", "5")), int(opt("seed", "1"))
    tmp = tempfile.mkdtemp(prefix="cv_bamtrain_")
    for n in rungs:
        t0 = time.time()
        L = n * 5
        ref, text = synth_pileup.fast_alignments(n, L)
        bam, fa = os.path.join(tmp, "r%d.bam" % n), os.path.join(tmp, "r%d.fa" % n)
        write_bam(bam, text.decode().splitlines(), [("ctgA", L)])
        r = ref.decode()
        with open(fa, "w") as fh:
            fh.write(">ctgA\n" + "\n".join(r[i:i + 60] for i in range(0, len(r), 60)) + "\n")
        open(fa + ".fai", "w").write("ctgA\t%d\t6\t60\t61\n" % L)
        var_fn = bc.write_rows(os.path.join(tmp, "var%d.gz" % n), bc.truth_rows("ctgA", r, 3, L // 1000))
        bed_fn = bc.write_rows(os.path.join(tmp, "bed%d.gz" % n), bc.bed_rows("ctgA", L, 900))
        print("== 150 bp x %d reads, %d bp: BAM %.1f MB, inputs written in %.0f s" % (n, L, os.path.getsize(bam) / 1e6, time.time() - t0), flush=True)
        common = ["--bam_fn", bam, "--ref_fn", fa, "--ctgName", "ctgA", "--samtools", "native"]
        out = os.path.join(tmp, "o%d_" % n)

        def recipe():
            t = {}
            t1 = time.time()
            ExtractVariantCandidates.MakeCandidates(ExtractVariantCandidates.build_parser().parse_args(
                common + ["--can_fn", out + "can.gz", "--gen4Training", "--seed", str(seed)]))
            t["extract"] = time.time() - t1; t1 = time.time()
            for src, dst in ((var_fn, "tv.gz"), (out + "can.gz", "tc.gz")):
                CreateTensor.OutputAlnTensor(CreateTensor.build_parser().parse_args(common + ["--can_fn", src, "--tensor_fn", out + dst]))
            t["tensors"] = time.time() - t1; t1 = time.time()
            PairWithNonVariants.Pair(argparse.Namespace(tensor_can_fn=out + "tc.gz", tensor_var_fn=out + "tv.gz", bed_fn=bed_fn,
                                                        output_fn=out + "mix.gz", amp=2, seed=seed))
            t["pair"] = time.time() - t1; t1 = time.time()
            random.seed(seed)
            tensor2Bin.Run(tensor2Bin.build_parser().parse_args(["--tensor_fn", out + "mix.gz", "--var_fn", var_fn, "--bed_fn", bed_fn,
                                                                "--bin_fn", out + "recipe.bin"]))
            t["tensor2Bin"] = time.time() - t1
            return t

        def to_bin():
            random.seed(seed)
            tensor2Bin.Run(tensor2Bin.build_parser().parse_args(common + ["--var_fn", var_fn, "--bed_fn", bed_fn, "--seed", str(seed),
                                                                         "--bin_fn", out + "bam.bin"]))

        def resident():
            random.seed(seed)
            ts = utils_v2.GetTrainingSetFromBam([(bam, fa, "ctgA", None, None)], var_fn, bed_fn, seed=seed, samtools="native")
            ts.resident()
            torch.cuda.synchronize()
            return ts

        def timed(fn):
            torch.cuda.synchronize(); t1 = time.time()
            res = fn()
            torch.cuda.synchronize()
            return time.time() - t1, res
        recipe(); to_bin(); ts = resident()
        a, b = cases.arrays_of(utils_v2.LoadBin(out + "recipe.bin")), cases.arrays_of(utils_v2.LoadBin(out + "bam.bin"))
        same = a[:2] == b[:2] and a[4] == b[4] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        same = same and ts.keys() == a[4] and np.array_equal(ts.X.cpu().numpy().reshape(ts.total, -1).view(np.uint32), a[2])
        print("   the routes give the same set: %s (%d items; pairing %s)" % (same, a[0], ts.pairing), flush=True)
        assert same
        for name, fn in (("recipe", recipe), ("bin", to_bin), ("resident", resident)):
            runs = [timed(fn) for _ in range(reps)]
            secs = [x[0] for x in runs]
            med = runs[sorted(range(reps), key=lambda i: secs[i])[reps // 2]]
            print("   %-8s median %.3f s (all: %s)" % (name, med[0], " ".join("%.3f" % s for s in secs)), flush=True)
            if name == "recipe":
                print("            steps of the median run: " + ", ".join("%s %.3f" % kv for kv in med[1].items()), flush=True)
            if name == "resident":
                print("            phases of the median run: " + ", ".join("%s %.3f" % kv for kv in sorted(med[1].times.items()) if not kv[0].endswith("_ms")), flush=True)
        ts = utils_v2.GetTrainingSetFromBam([(bam, fa, "ctgA", None, None)], var_fn, bed_fn, seed=seed, samtools="native")
        t1 = time.time(); ts.blocks()
        print("            pack (blocks of the resident set): %.3f s" % (time.time() - t1), flush=True)
        kernels(bam, fa, var_fn, seed, ts)


def kernels(bam, fa, var_fn, seed, ts):
    """HIP-event times: the handle's own (evc_count, the sampling select, the union, pileup_scatter, finalize), torch
    events round the columns launch, and the pairing launches' event time of the set `ts` just built"""
    import torch
    from clairvoyante_amd.bam import BamFile, faidx
    from clairvoyante_amd.pileup import Pileup
    from clairvoyante_amd import utils_v2
    pl = Pileup(evc=True, retain=True, contig="ctgA")
    pl.set_reference(faidx(fa, "ctgA"), 0)
    bf = BamFile(bam)
    pl.add_bam(bf, "ctgA")
    s0 = pl.stats()
    pl.sample_candidates(seed, 2 * 7000000. / 3000000000)
    s1 = pl.stats()
    truth = sorted(set(int(r.split()[1]) for r in utils_v2._gz_lines(var_fn)))
    pl.adopt_union(truth)
    s2 = pl.stats()
    _x, depth, touched = pl.finish(subtract=True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(); pl.columns(depth, touched); ev[1].record()
    torch.cuda.synchronize()
    s3 = pl.stats()
    print("   kernels (ms): evc_count %.3f, sampling select %.3f, union (fill + sort + heads + scan + write) %.3f, pileup_scatter %.3f, "
          "finalize %.3f, bt_columns %.3f over %d centres, bt_pair_count + bt_pair_keep %.3f over %d truth + usable rows"
          % (s0["candidate_ms"], s1["candidate_ms"] - s0["candidate_ms"], s2["candidate_ms"] - s1["candidate_ms"], s3["scatter_ms"],
             s3["finalize_ms"], ev[0].elapsed_time(ev[1]), pl.n, ts.times["pair_kernels_ms"], ts.pairing["v"] + ts.pairing["c"]),
          flush=True)
    bf.close(); pl.close()


if __name__ == "__main__":
    main()
