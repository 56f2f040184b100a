"""Development probe: the candidate list, host loops against the opt-in device routes of the same tree.
    python tools/gpu_candidate_list_probe.py [rungs=20000,200000,2000000] [runs=5] [thr=0.03] [depth=30]
Per rung (reads of synth_pileup.fast_alignments at about `depth` fold over a contig sized to them):
  write  ExtractVariantCandidates.MakeCandidates end to end -- pileup, selection, rows, output -- under
         CV_CANDIDATE_ROWS=host and =device, for the plain selection (threshold `thr`, so that a position with one
         mismatching read is a candidate) and for --gen4Training --seed 5 (every position, 2 * 7e6 / 3e9 of them kept),
         into /dev/null (PIPE), into `gzip -c` and into --bgzf: seconds of every run (run 0 of each warms up and is not
         reported), whether the device route was ahead in EVERY run, and the device calls by HIP events (order,
         lengths, rows; milliseconds per run).  The alignments and the reference come from memory, not from samtools:
         both routes read them the same way.  The bytes of the two routes are compared once per line.
  read   CreateTensor.read_candidates over the plain selection's list as plain text, .gz and BGZF under
         CV_CANDIDATE_LIST=host and =device, the line pass by HIP events.
The host routes are the parent commit's code, so no child process is needed."""
import gzip
import os
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fmt(v, form="%.3f"):
    return " ".join(form % x for x in v)


def verdict(host, dev):
    return "device ahead in every run" if max(dev) < min(host) else "device NOT ahead in every run"


def evc_args(tmp, can_fn, thr, gen4, bgzf):
    return types.SimpleNamespace(bam_fn="memory", ref_fn=os.path.join(tmp, "ref.fa"), bed_fn=None, can_fn=can_fn, threshold=thr,
                                 minCoverage=4, minMQ=0, gen4Training=gen4, candidates=7000000, genomeSize=3000000000,
                                 ctgName="ctgA", ctgStart=None, ctgEnd=None, samtools="memory", seed=5 if gen4 else None, bgzf=bgzf)


def timed_write(route, tmp, sink, thr, gen4, runs):
    import torch
    from clairvoyante_amd import ExtractVariantCandidates as evc, pileup
    os.environ["CV_CANDIDATE_ROWS"] = route
    can_fn = "PIPE" if sink == "null" else os.path.join(tmp, "%s_%s.gz" % (route, sink))
    out, split, rows = [], {}, None
    for r in range(runs + 1):
        pileup.CANDROWS_TIMES = {} if route == "device" else None
        evc.candidate_row_counts(reset=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        rows = evc.MakeCandidates(evc_args(tmp, can_fn, thr, gen4, sink == "bgzf"))
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        c = evc.candidate_row_counts()
        assert c["device" if route == "host" else "host"] == 0, c
        if r:
            out.append(dt)
            for k, v in (pileup.CANDROWS_TIMES or {}).items():
                split.setdefault(k, []).append(v)
    pileup.CANDROWS_TIMES = None
    return out, split, rows if isinstance(rows, int) else len(rows), can_fn


def timed_read(route, fn, runs):
    import torch
    from clairvoyante_amd import CreateTensor
    os.environ["CV_CANDIDATE_LIST"] = route
    out, split, got = [], {}, None
    for r in range(runs + 1):
        CreateTensor.CAN_TIMES = {} if route == "device" else None
        CreateTensor.candidate_list_counts(reset=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        got = CreateTensor.read_candidates(types.SimpleNamespace(can_fn=fn, ctgName="ctgA"), None, None)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        c = CreateTensor.candidate_list_counts()
        assert (c["device_calls"], c["host_calls"]) == ((1, 0) if route == "device" else (0, 1)), c
        if r:
            out.append(dt)
            for k, v in (CreateTensor.CAN_TIMES or {}).items():
                split.setdefault(k, []).append(v)
    CreateTensor.CAN_TIMES = None
    return out, split, got


def main():
    opt = dict(a.split("=", 1) for a in sys.argv[1:])
    rungs = [int(v) for v in opt.get("rungs", "20000,200000,2000000").split(",") if v]
    runs, thr, depth = int(opt.get("runs", 5)), float(opt.get("thr", 0.03)), int(opt.get("depth", 30))
    from clairvoyante_amd import ExtractVariantCandidates as evc, synth_pileup as sp, utils_v2
    tmp = tempfile.mkdtemp(prefix="cv_candlist_")
    open(os.path.join(tmp, "ref.fa.fai"), "w").close()
    null = open(os.devnull, "wb")
    stdout = sys.stdout
    say = lambda s: (stdout.write(s + "\n"), stdout.flush())
    say("reads what sink rows | host route s per run | device route s per run | verdict | device calls by HIP events, ms per run")
    for n in rungs:
        ref, sam = sp.fast_alignments(n, max(n * 150 // depth, 2000))
        evc.load_reference = lambda *a: ref
        evc.stream_alignments = lambda args, pl, cs, ce, source=None: pl.add_sam(sam)
        plain_list = None
        for gen4 in (False, True):
            for sink in ("null", "gzip", "bgzf"):
                sys.stdout = types.SimpleNamespace(buffer=null, write=lambda s: None, flush=lambda: None)
                try:
                    host, _s, hrows, hfn = timed_write("host", tmp, sink, thr, gen4, runs)
                    dev, split, drows, dfn = timed_write("device", tmp, sink, thr, gen4, runs)
                finally:
                    sys.stdout = stdout
                assert hrows == drows, "the routes disagree on the rows"
                if sink != "null":
                    assert gzip.open(hfn, "rb").read() == gzip.open(dfn, "rb").read(), "the routes disagree"
                    if not gen4 and sink == "gzip":
                        plain_list = gzip.open(dfn, "rb").read()
                say("%8d %-9s %-5s %9d | %s | %s | %s | %s" % (n, "gen4+seed" if gen4 else "select", sink, drows, fmt(host), fmt(dev), verdict(host, dev),
                                                             "; ".join("%s %s" % (k, fmt(v, "%.2f")) for k, v in sorted(split.items()))))
        forms = {"plain": os.path.join(tmp, "list.can"), "gz": os.path.join(tmp, "list.can.gz"), "bgzf": os.path.join(tmp, "list.bgzf.gz")}
        open(forms["plain"], "wb").write(plain_list)
        with gzip.open(forms["gz"], "wb", compresslevel=1) as fh:
            fh.write(plain_list)
        with utils_v2.BgzfWriter(forms["bgzf"], level=1) as bg:
            bg.write(plain_list)
        for form, fn in forms.items():
            host, _s, hgot = timed_read("host", fn, runs)
            dev, split, dgot = timed_read("device", fn, runs)
            assert hgot.dtype == dgot.dtype and np.array_equal(hgot, dgot), "the routes disagree"
            say("%8d %-9s %-5s %9d | %s | %s | %s | %s" % (n, "read", form, len(hgot), fmt(host), fmt(dev), verdict(host, dev),
                                                         "; ".join("%s %s" % (k, fmt(v, "%.2f")) for k, v in sorted(split.items()))))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
