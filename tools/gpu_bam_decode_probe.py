"""Development probe: the BAM front end on the host route and on the device route (csrc/cv_bam_dev.hip), on synthetic
coordinate-sorted BAMs written by tests/bam_writer.py -- a ladder of 150 bp reads at ~30x and one long-read shape.

  python tools/gpu_bam_decode_probe.py [rungs=20000,200000,2000000] [long=3000] [reps=5] [e2e=1] [parent=DIR]

Per rung, the median of `reps` runs of: Pileup.add_bam + extract_candidates + adopt + finish on both routes (the pileup
kernels' own event times and the device route's phases beside them), callVarBam --samtools native end to end on both
routes, and -- parent=DIR: a checkout of the parent commit, built -- the same host-route figures from that tree in a child
process.  Results are compared between the routes before anything is timed."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, os, sys, time, statistics
root, bam, fa, chk, reps, e2e = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6])
sys.path.insert(0, root)
import torch
from clairvoyante_amd.bam import BamFile, faidx
from clairvoyante_amd.pileup import Pileup
ref = faidx(fa, "ctgA")
def front():
    pl = Pileup(evc=True, retain=True, contig="ctgA", evc_minMQ=0)
    pl.set_reference(ref, 0)
    bf = BamFile(bam)
    torch.cuda.synchronize(); t0 = time.time()
    pl.add_bam(bf, "ctgA")
    res = pl.extract_candidates(0.06, 4)
    pl.adopt_candidates()
    pl.finish()
    torch.cuda.synchronize(); dt = time.time() - t0
    bf.close(); pl.close()
    return dt
front()
out = {"front_s": statistics.median(front() for _ in range(reps))}
if e2e:
    from clairvoyante_amd import callVarBam
    a = callVarBam.build_parser().parse_args(["--chkpnt_fn", chk, "--bam_fn", bam, "--ref_fn", fa, "--ctgName", "ctgA", "--call_fn",
                                              bam + ".parent.vcf", "--samtools", "native", "--threshold", "0.06"])
    def run():
        t0 = time.time(); callVarBam.Run(a); return time.time() - t0
    run()
    out["e2e_s"] = statistics.median(run() for _ in range(reps))
print("RESULT " + json.dumps(out))
"""


def opt(name, default):
    for a in sys.argv[1:]:
        if a.startswith(name + "="):
            return a.split("=", 1)[1]
    return default


def main():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from bam_writer import write_bam
    from clairvoyante_amd import pileup, synth_pileup
    from clairvoyante_amd.bam import BamFile
    from clairvoyante_amd.pileup import Pileup
    rungs = [int(x) for x in opt("rungs", "20000,200000,2000000").split(",") if x]
    n_long = int(opt("long", "3000"))
    reps = int(opt("reps", "5"))
    e2e = int(opt("e2e", "1"))
    parent = opt("parent", "")
    tmp = tempfile.mkdtemp(prefix="cv_bamdev_")
    chk = ""
    if e2e:
        import common
        from oracle import cv_oracle as O
        from clairvoyante_amd import clairvoyante_v3
        O.build()
        m = clairvoyante_v3.Clairvoyante(); m.init(); m.setParameters(common.bench_params(O, "full", seed=11))
        chk = os.path.join(tmp, "model-000001"); m.saveParameters(chk); m.close()
    shapes = [("150 bp x %d" % n, n, None) for n in rungs] + ([("~10 kbp x %d" % n_long, n_long, (8000, 12000))] if n_long else [])
    for label, n, read_len in shapes:
        t0 = time.time()
        if read_len is None:
            L = n * 5                                           # 150 bp at ~30x
            ref, text = synth_pileup.fast_alignments(n, L)
            lines = text.decode().splitlines()
        else:
            L = n * 10000 // 30
            ref, lines = synth_pileup.make_alignments(seed=5, ref_len=L, n_reads=n, read_len=read_len, profile=synth_pileup.NOISY_PROFILE)
            ref = ref.encode()
        bam = os.path.join(tmp, "r%d_%s.bam" % (n, "long" if read_len else "short"))
        write_bam(bam, lines, [("ctgA", L)])
        fa = bam + ".fa"
        r = ref.decode()
        with open(fa, "w") as fh:
            fh.write(">ctgA\n" + "\n".join(r[i:i + 60] for i in range(0, len(r), 60)) + "\n")
        open(fa + ".fai", "w").write("ctgA\t%d\t6\t60\t61\n" % L)
        size = os.path.getsize(bam)
        print("== %s: BAM %.1f MB, written in %.0f s" % (label, size / 1e6, time.time() - t0), flush=True)

        def front(route, keep=False):
            pl = Pileup(evc=True, retain=True, contig="ctgA", evc_minMQ=0)
            pl.set_reference(ref, 0)
            bf = BamFile(bam)
            torch.cuda.synchronize(); t1 = time.time()
            pl.add_bam(bf, "ctgA", route=route)
            t_add = time.time() - t1
            res = pl.extract_candidates(0.06, 4)
            pl.adopt_candidates()
            t, d, u = pl.finish()
            torch.cuda.synchronize(); dt = time.time() - t1
            st = pl.stats()
            out = dict(s=dt, add_s=t_add, scatter_ms=st["scatter_ms"], evc_ms=st["candidate_ms"], phases=pl.bam_device_ms(), kept=pl.reads_kept)
            if keep:
                out["res"] = (res["pos0"], res["late"], res["counts"], t.cpu().numpy(), d.cpu().numpy(), st["columns"], st["segments"])
            bf.close(); pl.close()
            return out
        pileup.bam_decode_counts(reset=True)
        a, b = front("host", True), front("device", True)
        cnt = pileup.bam_decode_counts(reset=True)
        same = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a["res"], b["res"])) and a["kept"] == b["kept"]
        print("   routes agree: %s; device run: %s" % (same, json.dumps(cnt)), flush=True)
        if not same or cnt["handed_over_slabs"] or cnt["host_members"]:
            print("   NOT TIMED: the device route did not take this input cleanly")
            continue
        for route in ("host", "device"):
            runs = [front(route) for _ in range(reps)]
            med = sorted(runs, key=lambda x: x["s"])[len(runs) // 2]
            print("   add_bam+extract+adopt+finish %-6s: median %.3f s (min %.3f max %.3f), add_bam %.3f s, %.2f M reads/s, %.0f MB/s of BAM; "
                  "evc_count+select %.2f ms, pileup_scatter %.2f ms%s" % (
                      route, med["s"], min(x["s"] for x in runs), max(x["s"] for x in runs), med["add_s"], n / med["s"] / 1e6, size / med["s"] / 1e6,
                      med["evc_ms"], med["scatter_ms"],
                      "; device phases (wall ms): " + ", ".join("%s %.2f" % kv for kv in med["phases"].items()) if route == "device" else ""),
                  flush=True)
            print("      all runs: " + " ".join("%.3f" % x["s"] for x in runs), flush=True)
        if e2e:
            from clairvoyante_amd import callVarBam
            vcfs = {}
            for route in ("host", "device"):
                os.environ["CV_BAM_DECODE"] = route
                args = callVarBam.build_parser().parse_args(["--chkpnt_fn", chk, "--bam_fn", bam, "--ref_fn", fa, "--ctgName", "ctgA", "--call_fn",
                                                             bam + "." + route + ".vcf", "--samtools", "native", "--threshold", "0.06"])
                callVarBam.Run(args)
                ts = []
                for _ in range(reps):
                    t1 = time.time(); callVarBam.Run(args); ts.append(time.time() - t1)
                vcfs[route] = open(args.call_fn, "rb").read()
                print("   callVarBam --samtools native %-6s: median %.3f s (all: %s)" % (route, statistics.median(ts), " ".join("%.3f" % x for x in ts)),
                      flush=True)
            os.environ.pop("CV_BAM_DECODE", None)
            print("   VCF bytes equal: %s (%d lines)" % (vcfs["host"] == vcfs["device"], vcfs["host"].count(b"\n")))
        if parent:
            p = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(parent), bam, fa, chk, str(reps), str(e2e)],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=os.path.abspath(parent))
            lines_out = p.stdout.decode("utf-8", "replace").splitlines()
            got = [l for l in lines_out if l.startswith("RESULT ")]
            print("   parent commit (host route, child process): %s" % (got[0][7:] if got else "FAILED: " + " | ".join(lines_out[-3:])), flush=True)


if __name__ == "__main__":
    main()
