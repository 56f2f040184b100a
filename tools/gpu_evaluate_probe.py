"""Development probe: the evaluation report (evaluate.Test / train.PredictAndReport / evaluateListOfModels.Run) with its
arithmetic on the host (CV_EVAL=host: the loop every driver had before cv_eval_counts existed) against the device route,
with the set decoded once into HBM (utils_v2.resident_from_blocks) and streamed from its blocks.
    python tools/gpu_evaluate_probe.py ladder=16384,65536,200000,1000000 [runs=5] [parent=DIR] [list=200000] [kernel=65536]
Per rung, seconds of evaluate.Test (load the .bin, predict, report; the model exists already) as median and range over
`runs` runs after one warm-up, the modes alternating run by run: host, device with the set resident, device streamed, and
evaluate.Test as shipped (it decodes a set of one pass ahead and streams a larger one).
parent=DIR names a built checkout of the PARENT commit: its evaluate.Test is timed on the same files in a child process
(the package of that tree, one warm-up and `runs` runs), and its report must be the one this tree prints.
list=N: evaluateListOfModels.Run over three checkpoints on a set of N candidates, host against device (and the parent).
kernel=N: HIP-event times of cv_eval_counts beside the forward pass at N candidates.
Every mode's report lines are compared with the host's before a time is printed."""
import ctypes
import json
import logging
import os
import pickle
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.environ.get("CV_PROBE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _write_bin(tmp, n):
    """a .bin of n synthetic candidates with their labels (blocks of 500, X fp32, Y float64, as tensor2Bin writes them)"""
    import torch
    from clairvoyante_amd import synth, utils_v2
    k0 = min(n, 100000)
    xt, cls, rf, alt, il = synth.make_candidates(k0, seed=9, device="cuda", return_class=True)
    x = xt.cpu().numpy(); y = synth.make_labels(cls, rf, alt, il).cpu().numpy().astype(np.float64)
    del xt; torch.cuda.empty_cache()
    XC, YC = [], []
    for s in range(0, n + 1, 500):
        k = min(500, n - s)
        idx = np.arange(s, s + k) % k0
        XC.append(utils_v2.pack_array(np.ascontiguousarray(x[idx]) if k else np.array([])))
        YC.append(utils_v2.pack_array(np.ascontiguousarray(y[idx]) if k else np.array([])))
    fn = os.path.join(tmp, "e%d.bin" % n)
    with open(fn, "wb") as fh:
        pickle.dump(n, fh); pickle.dump(XC, fh); pickle.dump(YC, fh); pickle.dump([], fh)
    return fn


def _checkpoints(tmp, k):
    from clairvoyante_amd import clairvoyante_v3, synth
    m = clairvoyante_v3.Clairvoyante()
    out = []
    for seed in range(1, k + 1):
        m.setParameters(synth.bench_params("full", seed=seed))
        out.append(os.path.join(tmp, "model-%06d" % seed)); m.saveParameters(out[-1])
    m.close()
    return out


class _Lines(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, rec):
        msg = rec.getMessage()
        if "time elapsed" not in msg:
            self.lines.append(msg)


def _timed(fn):
    """-> (seconds, report lines) of fn(): host clock around work that ends in a device synchronise"""
    import torch
    h = _Lines(); root = logging.getLogger()
    root.addHandler(h); root.setLevel(logging.INFO)
    stream = [x for x in root.handlers if isinstance(x, logging.StreamHandler) and x is not h]
    for s in stream:
        root.removeHandler(s)
    try:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
    finally:
        root.removeHandler(h)
        for s in stream:
            root.addHandler(s)
    return dt, h.lines


def _args(binfn, **kw):
    return types.SimpleNamespace(bin_fn=binfn, tensor_fn=None, var_fn=None, bed_fn=None, v2=False, v3=True, slim=False, **kw)


def _set_mode(mode):
    from clairvoyante_amd import utils_v2
    os.environ["CV_EVAL"] = "host" if mode == "host" else "device"
    if mode == "default":
        del os.environ["CV_EVAL"]
    utils_v2.TRAINSET_FREE_BYTES = (1 << 20) if mode == "streamed" else None


def _test(mode, binfn, m):
    """evaluate.Test; "resident" decodes the set into HBM first whatever its size (evaluate.Test itself does so for a set
    of one pass only), "streamed" never (the free-memory override), "default" is evaluate.Test as a user runs it"""
    from clairvoyante_amd import evaluate, train, utils_v2
    if mode != "resident":
        return evaluate.Test(_args(binfn), m, utils_v2)
    total, XC, YC, _ = train.load_dataset(_args(binfn), utils_v2, m)
    XC, YC = train.resident_dataset(m, utils_v2, total, XC, YC)
    assert isinstance(XC, utils_v2.ResidentBlocks)
    train.PredictAndReport(m, utils_v2, total, XC, YC)


def _report(lines):
    return lines[lines.index("Version 2 model, evaluation on base change:"):]


def _fmt(v):
    v = np.array(v)
    return "%.4f (%.4f..%.4f)" % (np.median(v), v.min(), v.max())


def child(what, binfn, chk, runs):
    """the parent tree's own drivers on the same files -> one JSON line {"s": [...], "lines": [...]}"""
    from clairvoyante_amd import clairvoyante_v3, evaluate, evaluateListOfModels, utils_v2
    if what == "test":
        m = clairvoyante_v3.Clairvoyante(); m.init(); m.restoreParameters(chk)
        fn = lambda: evaluate.Test(_args(binfn), m, utils_v2)
    else:
        fn = lambda: evaluateListOfModels.Run(_args(binfn, chkpnt_list=chk))
    s, lines = [], None
    for r in range(runs + 1):
        dt, lines = _timed(fn)
        if r:
            s.append(dt)
    print("CHILD " + json.dumps({"s": s, "lines": lines}), flush=True)


def _run_child(parent, what, binfn, chk, runs):
    env = dict(os.environ, CV_PROBE_TREE=os.path.abspath(parent))
    env.pop("CV_EVAL", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child=%s" % what, "bin=%s" % binfn, "chk=%s" % chk,
                          "runs=%d" % runs], env=env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    got = json.loads([l for l in out.splitlines() if l.startswith("CHILD ")][-1][6:])
    return got["s"], got["lines"]


def ladder(sizes, runs, parent, tmp, chk):
    from clairvoyante_amd import clairvoyante_v3
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.restoreParameters(chk)
    modes = ("host", "resident", "streamed", "default")
    print("evaluate.Test, seconds, median (min..max) of %d runs" % runs)
    print("candidates | parent commit | host (CV_EVAL=host) | device, set resident | device, streamed | as shipped (CV_EVAL unset) | candidates/s host -> shipped", flush=True)
    for n in sizes:
        binfn = _write_bin(tmp, n)
        s = {k: [] for k in modes}; lines = {}
        for r in range(runs + 1):                   # run 0 warms up; the modes alternate
            for mode in modes:
                _set_mode(mode)
                dt, got = _timed(lambda: _test(mode, binfn, m))
                lines[mode] = _report(got)
                if r:
                    s[mode].append(dt)
        assert all(lines[k] == lines["host"] for k in modes), "the routes print different reports"
        par = "not run"
        if parent:
            ps, plines = _run_child(parent, "test", binfn, chk, runs)
            assert _report(plines) == lines["host"], "the parent commit prints a different report"
            par = _fmt(ps)
        print("%10d | %s | %s | %s | %s | %s | %.3g -> %.3g, as shipped %s every host run" %
              (n, par, _fmt(s["host"]), _fmt(s["resident"]), _fmt(s["streamed"]), _fmt(s["default"]), n / np.median(s["host"]),
               n / np.median(s["default"]), "beats" if max(s["default"]) < min(s["host"]) else "does NOT beat"), flush=True)
        print("           report: %s" % lines["host"][1], flush=True)
        os.unlink(binfn)
    _set_mode("default")
    m.close()


def model_list(n, runs, parent, tmp, chks):
    from clairvoyante_amd import evaluateListOfModels
    binfn = _write_bin(tmp, n)
    lst = os.path.join(tmp, "models.txt")
    with open(lst, "w") as fh:
        fh.write("".join(c + "\n" for c in chks))
    s = {"host": [], "resident": []}; lines = {}
    for r in range(runs + 1):
        for mode in s:
            _set_mode(mode)
            dt, lines[mode] = _timed(lambda: evaluateListOfModels.Run(_args(binfn, chkpnt_list=lst)))
            if r:
                s[mode].append(dt)
    assert lines["resident"] == lines["host"], "the routes print different reports"
    par = "not run"
    if parent:
        ps, plines = _run_child(parent, "list", binfn, lst, runs)
        assert plines == lines["host"], "the parent commit prints a different report"
        par = _fmt(ps)
    print("evaluateListOfModels.Run, %d checkpoints, %d candidates, seconds: parent commit %s | host %s | device %s" %
          (len(chks), n, par, _fmt(s["host"]), _fmt(s["resident"])), flush=True)
    os.environ.pop("CV_EVAL", None)
    os.unlink(binfn)


def kernel(n, chk):
    """cv_forward and cv_eval_counts (fp32 and float64 labels) at n candidates, HIP events"""
    import torch
    from clairvoyante_amd import _lib, clairvoyante_v3, synth
    lib = _lib.load()
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.restoreParameters(chk)
    xt, cls, rf, alt, il = synth.make_candidates(n, seed=9, device="cuda", return_class=True)
    y32 = synth.make_labels(cls, rf, alt, il).to(torch.float32).contiguous(); y64 = y32.to(torch.float64)
    out16 = m.predict_device(xt)
    counts = torch.zeros(64, dtype=torch.int64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def count(y):
        _lib.check(lib.cv_eval_counts(P(out16), P(y), int(y.dtype == torch.float64), n, P(counts), st))
    med = {}
    for name, fn in (("forward pass", lambda: m.predict_device(xt, out16)), ("cv_eval_counts, fp32 labels", lambda: count(y32)),
                     ("cv_eval_counts, float64 labels", lambda: count(y64))):
        ms = []
        for r in range(13):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            if r >= 3:
                ms.append(e0.elapsed_time(e1))
        med[name] = np.median(ms)
        print("%d candidates: %-32s %.4f ms median (%.4f..%.4f)" % (n, name, med[name], min(ms), max(ms)), flush=True)
    fwd = med["forward pass"]
    for name, b in (("cv_eval_counts, fp32 labels", 128), ("cv_eval_counts, float64 labels", 192)):
        print("%s: %.2f %% of the forward pass, %d bytes per candidate -> %.0f GB/s" %
              (name, 100 * med[name] / fwd, b, n * b / med[name] / 1e6), flush=True)
    m.close()


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    runs = int(opts.get("runs", 5))
    if "child" in opts:
        child(opts["child"], opts["bin"], opts["chk"], runs)
        return
    if not any(k in opts for k in ("ladder", "list", "kernel")):
        print(__doc__)
        return
    tmp = tempfile.mkdtemp(prefix="cv_eval_")
    try:
        chks = _checkpoints(tmp, 3)
        if "kernel" in opts:
            kernel(int(opts["kernel"]), chks[0])
        if "ladder" in opts:
            ladder([int(v) for v in opts["ladder"].split(",")], runs, opts.get("parent"), tmp, chks[0])
        if "list" in opts:
            model_list(int(opts["list"]), runs, opts.get("parent"), tmp, chks)
    finally:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
