"""Development probe: callVar end to end over ONE tensor file under 1, 2 and 4 ranks -- the `lines` route (every rank reads
the whole file and parses its blocks of lines) against the `range` route (CV_SHARD=range: every rank reads only its byte
range, of a BGZF file only its members), plain text and BGZF.

  python tools/gpu_sharded_reader_probe.py [rungs=65536,262144,1000000] [ranks=1,2,4] [runs=5] [forms=plain,bgzf]
                                           [parent=DIR] [limit=600] [out=FILE]

The ranks are processes on the ONE GPU of the box (CV_SHARE_DEVICES=1, backend gloo, as tests/test_gpu_dp.py starts
them; never more than 4): what this shows is what a rank saves by not reading the rest of the file, NOT how the job scales
over GPUs -- the ranks share one device, one PCIe link and one page cache.  A run is the whole command -- `python -m
clairvoyante_amd.callVar` per rank, from the start of the first process to the exit of the last, model load included --,
each process under `timeout` of `limit` seconds; the probe ends at the first run that fails or whose VCF differs from the
first one written for the file.  parent=DIR: a built checkout of the parent commit, run in child processes in that tree
(it has the `lines` route only).  Every run is printed; `out` also gets the lines.

The rule the default follows (callVar.SHARD_RANGE_DEFAULT): a form takes the `range` route unasked only if it is ahead of
the `lines` route in EVERY run of EVERY rung at 2 and at 4 ranks; otherwise the probe says by how much it missed."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_rows(path, n, x):
    from clairvoyante_amd.pileup import format_rows
    k0 = x.shape[0]
    with open(path, "wb") as fh:                    # the same tensors at advancing coordinates until n rows are written
        for s in range(0, n, k0):
            k = min(k0, n - s)
            rows = format_rows("chr1", np.arange(100 + s, 100 + s + k), b"N" * 83 + b"ACGT" * ((n + 200) // 4 + 8), 0, x[:k])
            fh.write(b"\n".join(rows) + b"\n")


def run_ranks(tree, ws, route, tensor_fn, chk, call_fn, limit, port):
    """one run -> seconds, or None when a rank failed (the others are ended, nothing more is started)"""
    env = dict(os.environ, PYTHONPATH=tree, CV_SHARE_DEVICES="1")
    for k in ("CV_SHARD", "CV_TEXT_PARSE", "CV_VCF_FORMAT", "CV_TEXT_SLAB_BYTES", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    if route in ("lines", "range"):
        env["CV_SHARD"] = route
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "clairvoyante_amd.callVar", "--chkpnt_fn", chk,
           "--tensor_fn", tensor_fn, "--call_fn", call_fn, "--sampleName", "S"]
    t0 = time.perf_counter()
    procs = []
    for r in range(ws):
        e = dict(env)
        if ws > 1:
            e.update(RANK=str(r), WORLD_SIZE=str(ws), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CV_DIST_BACKEND="gloo")
        procs.append(subprocess.Popen(cmd, env=e, cwd=tree, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE))
    left, failed = set(range(ws)), None
    while left and failed is None:
        for i in sorted(left):
            try:
                code = procs[i].wait(timeout=0.02)
            except subprocess.TimeoutExpired:
                continue
            left.discard(i)
            if code != 0:
                failed = (i, code)
    dt = time.perf_counter() - t0
    if failed is not None:
        for i in left:
            procs[i].terminate()
        for i in left:
            try:
                procs[i].wait(timeout=15)
            except subprocess.TimeoutExpired:
                procs[i].kill(); procs[i].wait()
        err = procs[failed[0]].stderr.read().decode("utf-8", "replace").splitlines()[-3:]
        print("   rank %d of %d exited %s: %s" % (failed[0], ws, failed[1], " | ".join(err)), flush=True)
        return None
    for p in procs:
        p.stderr.close()
    return dt


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    rungs = [int(v) for v in opts.get("rungs", "65536,262144,1000000").split(",") if v]
    ranks = [int(v) for v in opts.get("ranks", "1,2,4").split(",") if v]
    runs, limit = int(opts.get("runs", "5")), int(opts.get("limit", "600"))
    forms = opts.get("forms", "plain,bgzf").split(",")
    parent = os.path.abspath(opts["parent"]) if opts.get("parent") else None
    if max(ranks) > 4:
        sys.exit("at most 4 ranks share the GPU")
    sink = open(opts["out"], "a") if opts.get("out") else None

    def say(s):
        print(s, flush=True)
        if sink:
            sink.write(s + "\n"); sink.flush()

    import common
    from oracle import cv_oracle as O
    from clairvoyante_amd import bgzf, clairvoyante_v3, synth
    tmp = tempfile.mkdtemp(prefix="cv_shard_")
    x = synth.make_candidates(min(max(rungs), 65536), seed=9, device="cuda").cpu().numpy()
    x[..., 1:] += x[..., 0:1]
    x = np.maximum(x, 0)
    O.build()
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.setParameters(common.bench_params(O, "full", seed=11))
    chk = os.path.join(tmp, "model-000001"); m.saveParameters(chk); m.close()
    say("# ranks = processes on ONE GPU (gloo): a rank's saving from reading less, not scaling over GPUs")
    say("# seconds per run = the whole command, model load included; rows/s = rows / median seconds")
    trees = [("this", ROOT)] + ([("parent", parent)] if parent else [])
    missed = {f: [] for f in forms}                 # (rung, ranks, worst lines / range ratio where range was not ahead)
    port = 29500 + os.getpid() % 300
    ok = True
    for n in rungs:
        txt = os.path.join(tmp, "t%d.txt" % n)
        write_rows(txt, n, x)
        files = {"plain": txt}
        if "bgzf" in forms:
            bgzf.reblock(txt, txt + ".bgzf.gz", level=1)
            files["bgzf"] = txt + ".bgzf.gz"
        for form in forms:
            fn, first = files[form], None
            say("== %d rows, %s, %.1f MB on disk" % (n, form, os.path.getsize(fn) / 1e6))
            times = {}
            for ws in ranks:
                for tree_name, tree in trees:
                    for route in (["one"] if ws == 1 else (["lines", "range"] if tree_name == "this" else ["unset"])):
                        key, secs = (tree_name, ws, route), []
                        for r in range(runs):
                            port += 1
                            call_fn = os.path.join(tmp, "out_%s_%d_%s.vcf" % (tree_name, ws, route))
                            dt = run_ranks(tree, ws, route, fn, chk, call_fn, limit, port)
                            if dt is None:
                                say("   %-6s %d rank(s) %-5s FAILED in run %d: the probe ends here" % (tree_name, ws, route, r))
                                ok = False
                                break
                            vcf = open(call_fn, "rb").read()
                            if first is None:
                                first = vcf
                            if vcf != first:
                                say("   %-6s %d rank(s) %-5s wrote ANOTHER VCF in run %d: the probe ends here" % (tree_name, ws, route, r))
                                ok = False
                                break
                            secs.append(dt)
                        if not ok:
                            break
                        times[key] = secs
                        say("   %-6s %d rank(s) %-5s s per run: %s   -> %.3g rows/s" % (
                            tree_name, ws, route, " ".join("%.2f" % v for v in secs), n / float(np.median(secs))))
                    if not ok:
                        break
                if not ok:
                    break
            if not ok:
                break
            for ws in ranks:
                if ws > 1:
                    a, b = times["this", ws, "lines"], times["this", ws, "range"]
                    ahead = max(b) < min(a)
                    say("   %d ranks: range %s ahead of lines in every run (slowest range %.2f s, fastest lines %.2f s; medians %.2f / %.2f)" % (
                        ws, "IS" if ahead else "is NOT", max(b), min(a), np.median(b), np.median(a)))
                    if not ahead and ws in (2, 4):
                        missed[form].append((n, ws, max(b) / min(a)))
            say("   VCF bytes equal in every run: True (%d lines)" % first.count(b"\n"))
            if form != "plain":
                os.unlink(fn)
        os.unlink(txt)
        if not ok:
            break
    if ok:
        for form in forms:
            if missed[form]:
                say("VERDICT %s: range stays opt-in -- not ahead in every run at: %s" % (
                    form, "; ".join("%d rows, %d ranks (slowest range run %.2f x the fastest lines run)" % t for t in missed[form])))
            else:
                say("VERDICT %s: range was ahead of lines in every run of every rung measured here (rungs %s, ranks %s, %d runs)" % (
                    form, rungs, [w for w in ranks if w > 1], runs))
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    if sink:
        sink.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
