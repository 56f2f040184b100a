"""Development probe: cv_forward against cv_forward_logits (the same pass with the logits epilogue on the kernel that
computes the heads), device tensors in and out.
    python tools/gpu_embeddings_probe.py [sizes=1000,16384,65536] [runs=5] [parent=DIR] [out=profiles/r25/embeddings.txt]
Per topology (full, slim) and size: microseconds per call as min / median / max over `runs` runs; a run is a window of
back-to-back calls between two device events (about 50 ms of work) after a warm-up window, the two entries one after
the other.  Every run is a child process of its own, so that a tree's runs differ by what differs between processes too.
parent=DIR names a built checkout of the PARENT commit: its cv_forward is timed the same way (the package of that tree),
the two trees alternating run by run, and the table says whether this tree's cv_forward lies inside the parent's
min..max and whether cv_forward_logits stays at or below the parent's maximum -- it does strictly less arithmetic than
the pass it mirrors.
The logits pass is compared with the softmax pass before a time is printed: the same base sigmoid, and softmax of the
logits within 1e-6 of the other three heads."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.environ.get("CV_PROBE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _model(arch):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim, synth
    m = clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()
    m.setParameters(synth.bench_params(arch, seed=1))
    return m


def _window(fn, reps):
    """microseconds per call of `reps` back-to-back calls between two device events"""
    import torch
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def _reps(fn):
    """calls per window: about 50 ms of work, measured on a first window that also warms up"""
    us = _window(fn, 20)
    return int(min(5000, max(20, 50000.0 / us)))


def measure(arch, sizes, runs, entries):
    """{n: {entry: [us per call] * runs}}; entries among "forward", "logits", one after the other in every run"""
    import torch
    from clairvoyante_amd import synth
    m = _model(arch)
    res = {}
    for n in sizes:
        x = synth.make_candidates(n, seed=9, device="cuda").contiguous()
        out = torch.empty((n, 16), dtype=torch.float32, device="cuda")
        fns = {"forward": lambda: m.predict_device(x, out)}
        if "logits" in entries:
            fns["logits"] = lambda: m.embeddings_device(x, out)
            soft = m.predict_device(x).clone(); lg = m.embeddings_device(x).clone()
            assert torch.equal(soft[:, :4], lg[:, :4]), "the base sigmoid differs between the two entries"
            for lo, hi in ((4, 6), (6, 10), (10, 16)):
                assert (torch.softmax(lg[:, lo:hi].double(), 1) - soft[:, lo:hi].double()).abs().max().item() < 1e-6
        reps = {k: _reps(f) for k, f in fns.items()}
        t = {k: [] for k in fns}
        for _ in range(runs):
            for k in entries:
                t[k].append(_window(fns[k], reps[k]))
        res[n] = t
    m.close()
    return res


def _run_child(tree, arch, sizes, entries):
    """one run of every size in a process of its own, the package of `tree` -> {n: {entry: us per call}}"""
    env = dict(os.environ, CV_PROBE_TREE=os.path.abspath(tree))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child=%s" % arch, "sizes=%s" % ",".join(map(str, sizes)),
                          "entries=%s" % ",".join(entries)], env=env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    got = json.loads([l for l in out.splitlines() if l.startswith("CHILD ")][-1][6:])
    return {int(n): {k: v[0] for k, v in t.items()} for n, t in got.items()}


def _fmt(v):
    return "%9.1f %9.1f %9.1f" % (min(v), float(np.median(v)), max(v))


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    sizes = [int(v) for v in opts.get("sizes", "1000,16384,65536").split(",")]
    runs = int(opts.get("runs", 5))
    if "child" in opts:
        print("CHILD " + json.dumps(measure(opts["child"], sizes, 1, tuple(opts["entries"].split(",")))), flush=True)
        return
    parent = opts.get("parent")
    lines = ["cv_forward and cv_forward_logits, microseconds per call (device events around windows of back-to-back calls),",
             "min / median / max of %d runs; parent = the parent commit's cv_forward%s" % (runs, "" if parent else " (not run)"),
             "%-5s %7s | %-29s | %-29s | %-29s | %s" % ("arch", "n", "parent cv_forward", "cv_forward", "cv_forward_logits", "verdict")]
    ok = True
    for arch in ("full", "slim"):
        par = {n: {"forward": []} for n in sizes} if parent else None
        mine = {n: {"forward": [], "logits": []} for n in sizes}
        for _ in range(runs):                       # one process on the GPU at a time, the trees alternating
            for tree, acc, entries in ((parent, par, ("forward",)), (ROOT, mine, ("forward", "logits"))):
                if tree:
                    sys.stderr.write("%s: a run of %s\n" % (arch, "the parent" if tree is parent else "this tree")); sys.stderr.flush()
                    for n, t in _run_child(tree, arch, sizes, entries).items():
                        for k, v in t.items():
                            acc[n][k].append(v)
        for n in sizes:
            f, l = mine[n]["forward"], mine[n]["logits"]
            verdict = "-"
            if par:
                p = par[n]["forward"]
                inside = min(p) <= float(np.median(f)) <= max(p)
                below = float(np.median(l)) <= max(p)
                ok = ok and inside and below
                verdict = "cv_forward median %s the parent's range (%d of %d runs inside), logits median %s its maximum (%d of %d runs)" % (
                    "inside" if inside else "OUTSIDE", sum(min(p) <= v <= max(p) for v in f), len(f),
                    "within" if below else "ABOVE", sum(v <= max(p) for v in l), len(l))
            lines.append("%-5s %7d | %s | %s | %s | %s" % (arch, n, _fmt(par[n]["forward"]) if par else " " * 29, _fmt(f), _fmt(l), verdict))
    if parent:
        lines.append("all rows hold" if ok else "NOT all rows hold: compare the kernels' resources (tools/kernel_resources.py) before anything else")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
