"""Development probe: callVarBam's hop between the pileup and the call loop -- which centres give a row, their tensors and
their tokens -- on the host (the list comprehensions and PosBatch.from_columns) and on the device
(csrc/cv_callcols_dev.hip, CV_CALL_COLUMNS=device), on synthetic coordinate-sorted BAMs written by tests/bam_writer.py: a
ladder of 150 bp reads at ~30x and one long-read shape.

  python tools/gpu_call_columns_probe.py [rungs=20000,200000] [long=600] [runs=5] [parent=DIR]

Per rung, after one untimed run of everything, `runs` runs of each figure, every run printed:
  front end   add_bam + extract_candidates + adopt_candidates + finish, ended by a device synchronise
  hop         callVarBam.select_rows on either side behind that synchronise, ended by one; beside it the HIP-event time of
              the kernels of cv_pileup_call_columns alone and the pileup's own finalize_ms
  Run         callVarBam.Run(model=m) -- the model restored once, outside -- under CV_CALL_COLUMNS x CV_VCF_FORMAT, with
              Run's own split (front end, hop, call loop; a host clock, so the hop carries whatever the GPU still owed
              of the front end), and once per side a Run that restores the model itself
  parent=DIR  a checkout of the parent commit, built: its Run(model=m) and its Run() over the same files, in a child
              process in that tree, on both VCF routes
The VCF files of all sides are compared before anything is reported as a time."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, os, sys, time
root, bam, fa, chk, runs = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5])
sys.path.insert(0, root)
import torch
from clairvoyante_amd import callVarBam, clairvoyante_v3
m = clairvoyante_v3.Clairvoyante(); m.init(); m.restoreParameters(chk)
out = {}
for records in ("host", "device"):
    os.environ["CV_VCF_FORMAT"] = records
    a = callVarBam.build_parser().parse_args(["--chkpnt_fn", chk, "--bam_fn", bam, "--ref_fn", fa, "--ctgName", "ctgA", "--call_fn",
                                              bam + ".parent." + records + ".vcf", "--samtools", "native", "--threshold", "0.06"])
    def run(model):
        torch.cuda.synchronize(); t0 = time.time(); callVarBam.Run(a, model=model); torch.cuda.synchronize(); return time.time() - t0
    run(m)
    out["run_model_" + records] = [run(m) for _ in range(runs)]
    out["run_" + records] = [run(None) for _ in range(runs)]
m.close()
print("RESULT " + json.dumps(out))
"""


def opt(name, default):
    for a in sys.argv[1:]:
        if a.startswith(name + "="):
            return a.split("=", 1)[1]
    return default


def ms(values):
    return " ".join("%.2f" % (1e3 * v) for v in values)


def main():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import logging
    import numpy as np
    import torch
    import common
    from bam_writer import write_bam
    from oracle import cv_oracle as O
    from clairvoyante_amd import callVar, callVarBam, clairvoyante_v3, synth_pileup
    from clairvoyante_amd.bam import BamFile
    from clairvoyante_amd.pileup import Pileup
    logging.getLogger().setLevel(logging.WARNING)
    rungs = [int(x) for x in opt("rungs", "20000,200000").split(",") if x]
    n_long = int(opt("long", "600"))
    runs = int(opt("runs", "5"))
    parent = opt("parent", "")
    tmp = tempfile.mkdtemp(prefix="cv_callcols_")
    O.build()
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.setParameters(common.bench_params(O, "full", seed=11))
    chk = os.path.join(tmp, "model-000001"); m.saveParameters(chk)
    say = lambda s: print(s, flush=True)
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
        say("== %s: BAM %.1f MB, written in %.0f s" % (label, os.path.getsize(bam) / 1e6, time.time() - t0))

        # ---- the front end and the hop alone ----
        def front_and_hop(timed):
            pl = Pileup(evc=True, retain=True, contig="ctgA", evc_minMQ=0)
            pl.set_reference(ref, 0)
            bf = BamFile(bam)
            torch.cuda.synchronize(); t1 = time.time()
            pl.add_bam(bf, "ctgA")
            pl.extract_candidates(0.06, 4)
            pl.adopt_candidates()
            t, _d, touched = pl.finish(subtract=True)
            torch.cuda.synchronize(); front = time.time() - t1
            out = {"front": front, "n": pl.n, "finalize_ms": pl.stats()["finalize_ms"]}
            got = {}
            for side in (("host", "device") if timed % 2 == 0 else ("device", "host")):      # alternate who goes first
                torch.cuda.synchronize(); t1 = time.time()
                res = callVarBam.select_rows(pl, t, touched, "ctgA", ref, 0, side)
                torch.cuda.synchronize(); out[side] = time.time() - t1
                got[side] = res
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); pl.call_columns(touched, "ctgA"); e1.record(); torch.cuda.synchronize()
            out["kernels_ms"] = e0.elapsed_time(e1)             # (ends behind the fetch of the two integers: kernels + one 16-byte copy)
            h, d = got["host"], got["device"]
            (_s, _r, buf, meta), = d["pos"].pieces()
            (_s, _r, hbuf, hmeta), = h["pos"].pieces()
            out["same"] = (torch.equal(h["tensors"], d["tensors"]) and np.array_equal(h["centers"], d["centers"]) and h["seqs"] == d["seqs"]
                           and bytes(buf) == bytes(hbuf) and np.array_equal(meta, hmeta))
            out["rows"] = int(d["tensors"].shape[0])
            bf.close(); pl.close()
            return out
        first = front_and_hop(0)
        say("   %d centres, %d rows kept; host and device columns equal: %s" % (first["n"], first["rows"], first["same"]))
        if not first["same"]:
            say("   NOT TIMED: the sides disagree")
            continue
        rs = [front_and_hop(k) for k in range(runs)]
        say("   front end (add_bam .. finish), ms per run:      " + ms(x["front"] for x in rs))
        say("   hop on the host, ms per run:                    " + ms(x["host"] for x in rs))
        say("   hop on the device, ms per run:                  " + ms(x["device"] for x in rs))
        say("   cv_pileup_call_columns by HIP events, ms:       " + " ".join("%.3f" % x["kernels_ms"] for x in rs)
            + "   (pileup_finalize: " + " ".join("%.3f" % x["finalize_ms"] for x in rs) + ")")

        # ---- Run, end to end ----
        vcfs, times = {}, {}
        for records in ("host", "device"):
            for columns in ("host", "device"):
                os.environ["CV_CALL_COLUMNS"] = columns; os.environ["CV_VCF_FORMAT"] = records
                a = callVarBam.build_parser().parse_args(["--chkpnt_fn", chk, "--bam_fn", bam, "--ref_fn", fa, "--ctgName", "ctgA", "--call_fn",
                                                          bam + "." + columns + "." + records + ".vcf", "--samtools", "native", "--threshold", "0.06"])

                def run(model):
                    torch.cuda.synchronize(); t1 = time.time(); res = callVarBam.Run(a, model=model); torch.cuda.synchronize()
                    return time.time() - t1, res["times"]
                before = callVar.vcf_format_counts()
                run(m)
                after = callVar.vcf_format_counts()
                vcfs[columns, records] = open(a.call_fn, "rb").read()
                times[columns, records] = ([run(m) for _ in range(runs)], [run(None) for _ in range(runs)], after["handed_over"] - before["handed_over"])
        os.environ.pop("CV_CALL_COLUMNS", None); os.environ.pop("CV_VCF_FORMAT", None)
        same = all(v == vcfs["host", "host"] for v in vcfs.values())
        say("   VCF bytes equal on all four sides: %s (%d lines)" % (same, vcfs["host", "host"].count(b"\n")))
        if not same:
            say("   NOT TIMED: the VCF files differ")
            continue
        for (columns, records), (with_model, alone, handed) in times.items():
            say("   Run(model=m) columns %-6s records %-6s ms per run: %s   batches handed over: %d" % (columns, records, ms(x[0] for x in with_model), handed))
            say("      split (front | hop | call loop), ms:          " + "  ".join("%.1f|%.1f|%.1f" % (1e3 * s["front_s"], 1e3 * s["hop_s"], 1e3 * s["call_s"])
                                                                                for _t, s in with_model))
            say("      Run() restoring the model itself, ms per run:  %s   (model: %s)" % (ms(x[0] for x in alone), ms(s["model_s"] for _t, s in alone)))
        if parent:
            p = subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(parent), bam, fa, chk, str(runs)],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=os.path.abspath(parent))
            lines_out = p.stdout.decode("utf-8", "replace").splitlines()
            got = [l for l in lines_out if l.startswith("RESULT ")]
            if not got:
                say("   parent commit: FAILED: " + " | ".join(lines_out[-3:]))
                continue
            res = json.loads(got[0][7:])
            for records in ("host", "device"):
                pv = open(bam + ".parent." + records + ".vcf", "rb").read()
                say("   parent commit, records %-6s Run(model=m) ms per run: %s   Run(): %s   VCF equal: %s" % (
                    records, ms(res["run_model_" + records]), ms(res["run_" + records]), pv == vcfs["host", "host"]))
    m.close()


if __name__ == "__main__":
    main()
