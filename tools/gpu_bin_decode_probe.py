"""Development probe: the blocks of a .bin set decoded by the host threads (CV_BIN_DECODE=host: cv_blosc_unpack_blocks, then
2 112 bytes per candidate cross) against the device route (CV_BIN_DECODE=device: the compressed chunks cross,
cv_blosc_decode_dev + cv_blosc_unpack_dev write the batch), per layout of the set.
    python tools/gpu_bin_decode_probe.py ladder=16384,65536,200000,1000000 [runs=5] [layouts=cblosc,own,own64k]
                                         [kernels=65536] [parent=DIR]
Layouts: cblosc = the reference's (cv_blosc_compress_lz4_blocks with 1 MiB blocks: 4 byte-plane streams and a leftover
per X chunk), own = this project's default writer (ONE unsplit stream per chunk), own64k = 64 KiB blocks (68 streams).
Per layout and rung, seconds of evaluate.Test (load the .bin, predict, report; the model exists already) and of
utils_v2.resident_from_blocks as median and range over `runs` runs after one warm-up, the two routes alternating run by
run, and evaluate.Test as shipped (CV_BIN_DECODE unset).  "wins" = every device run is faster than every host run.
parent=DIR names a built checkout of the PARENT commit: its evaluate.Test is timed on the same files in a child process.
kernels=N: HIP-event times of the two kernels alone for one pass of N candidates beside that pass's forward time, and the
bytes that cross per pass on either route.  Every route's report lines are compared with the host's before a time is
printed."""
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

BLOCKSIZE = {"cblosc": 1 << 20, "own": None, "own64k": 65536}


def _write_bin(tmp, n, layout):
    import torch
    from clairvoyante_amd import synth, utils_v2
    k0 = min(n, 100000)
    xt, cls, rf, alt, il = synth.make_candidates(k0, seed=9, device="cuda", return_class=True)
    x = xt.cpu().numpy(); y = synth.make_labels(cls, rf, alt, il).cpu().numpy().astype(np.float64)
    del xt; torch.cuda.empty_cache()
    XC, YC = [], []
    memo = {}
    for s in range(0, n + 1, 500):
        k = min(500, n - s)
        key = (s % k0, k) if s % k0 + k <= k0 else None
        if key is None or key not in memo:
            idx = np.arange(s, s + k) % k0
            got = (utils_v2.pack_array(np.ascontiguousarray(x[idx]) if k else x[:0], BLOCKSIZE[layout]),
                   utils_v2.pack_array(np.ascontiguousarray(y[idx]) if k else y[:0], BLOCKSIZE[layout]))
            if key is not None:
                memo[key] = got
        else:
            got = memo[key]
        XC.append(got[0]); YC.append(got[1])
    fn = os.path.join(tmp, "%s_%d.bin" % (layout, n))
    with open(fn, "wb") as fh:
        pickle.dump(n, fh); pickle.dump(XC, fh); pickle.dump(YC, fh); pickle.dump([], fh)
    return fn, sum(len(c) for c in XC) + sum(len(c) for c in YC)


class _Lines(logging.Handler):
    def __init__(self):
        logging.Handler.__init__(self)
        self.lines = []

    def emit(self, rec):
        msg = rec.getMessage()
        if "time elapsed" not in msg:
            self.lines.append(msg)


def _timed(fn):
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


def _route(route):
    if route is None:
        os.environ.pop("CV_BIN_DECODE", None)
    else:
        os.environ["CV_BIN_DECODE"] = route


def _report(lines):
    return lines[lines.index("Version 2 model, evaluation on base change:"):]


def _fmt(v):
    v = np.array(v)
    return "%.4f (%.4f..%.4f)" % (np.median(v), v.min(), v.max())


def child(binfn, chk, runs):
    from clairvoyante_amd import clairvoyante_v3, evaluate, utils_v2
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.restoreParameters(chk)
    s, lines = [], None
    for r in range(runs + 1):
        dt, lines = _timed(lambda: evaluate.Test(_args(binfn), m, utils_v2))
        if r:
            s.append(dt)
    print("CHILD " + json.dumps({"s": s, "lines": lines}), flush=True)


def _run_child(parent, binfn, chk, runs):
    env = dict(os.environ, CV_PROBE_TREE=os.path.abspath(parent))
    env.pop("CV_BIN_DECODE", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child=test", "bin=%s" % binfn, "chk=%s" % chk,
                          "runs=%d" % runs], env=env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    got = json.loads([l for l in out.splitlines() if l.startswith("CHILD ")][-1][6:])
    return got["s"], got["lines"]


def ladder(sizes, runs, layouts, parent, tmp, chk):
    from clairvoyante_amd import clairvoyante_v3, evaluate, utils_v2
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.restoreParameters(chk)
    print("seconds, median (min..max) of %d runs; floors in the code: %s" % (runs, utils_v2.BIN_DECODE_FLOOR))
    print("layout | candidates | compressed MB | Test parent commit | Test host | Test device | Test as shipped | "
          "resident_from_blocks host | device | candidates/s Test host -> device", flush=True)
    for layout in layouts:
        for n in sizes:
            binfn, cbytes = _write_bin(tmp, n, layout)
            total, XC, YC, _ = utils_v2.LoadBin(binfn)

            def resident():
                X, Y = utils_v2.resident_from_blocks(total, XC, YC)
                assert isinstance(X, utils_v2.ResidentBlocks)
                del X, Y
            modes = (("host", "host"), ("device", "device"), ("shipped", None))
            s = {k: [] for k, _ in modes}; rs = {"host": [], "device": []}; lines = {}
            for r in range(runs + 1):                   # run 0 warms up; the routes alternate
                for key, route in modes:
                    _route(route)
                    dt, got = _timed(lambda: evaluate.Test(_args(binfn), m, utils_v2))
                    lines[key] = _report(got)
                    if r:
                        s[key].append(dt)
                for route in ("host", "device"):
                    _route(route)
                    dt, _l = _timed(resident)
                    if r:
                        rs[route].append(dt)
            assert all(lines[k] == lines["host"] for k, _ in modes), "the routes print different reports"
            par = "not run"
            if parent:
                ps, plines = _run_child(parent, binfn, chk, runs)
                assert _report(plines) == lines["host"], "the parent commit prints a different report"
                par = _fmt(ps)
            print("%s | %d | %.1f | %s | %s | %s | %s | %s | %s | %.3g -> %.3g; Test: device %s every host run; resident: device %s" %
                  (layout, n, cbytes / 1e6, par, _fmt(s["host"]), _fmt(s["device"]), _fmt(s["shipped"]), _fmt(rs["host"]),
                   _fmt(rs["device"]), n / np.median(s["host"]), n / np.median(s["device"]),
                   "WINS" if max(s["device"]) < min(s["host"]) else "does not win",
                   "WINS" if max(rs["device"]) < min(rs["host"]) else "does not win"), flush=True)
            os.unlink(binfn)
    _route(None)
    m.close()


def kernels(n, layouts, tmp, chk):
    """the device route's own time for one pass of n candidates (plan + gather + copy + both kernels + status fetch, host
    clock) and the two kernels alone (HIP events), beside the forward pass"""
    import ctypes
    import torch
    from clairvoyante_amd import _lib, clairvoyante_v3, utils_v2
    lib = _lib.load()
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.restoreParameters(chk)
    for layout in layouts:
        binfn, _cb = _write_bin(tmp, n, layout)
        total, XC, YC, _ = utils_v2.LoadBin(binfn)
        host, dev = [], []
        for r in range(6):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            xh = utils_v2.DecompressArray(XC, 0, n, total)[0]
            xd0 = torch.from_numpy(np.ascontiguousarray(xh)).cuda(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            xd = utils_v2.DecompressArrayDevice(XC, 0, n, total)[0]; torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r:
                host.append(t1 - t0); dev.append(t2 - t1)
            assert torch.equal(xd0, xd)
        # the kernels alone, on the buffers the route left behind
        blocks = XC[0:(n - 1) // 500 + 1]
        k = len(blocks)
        hold = [np.frombuffer(c, dtype=np.uint8) for c in blocks]
        src = (ctypes.c_void_p * k)(*[h.ctypes.data for h in hold])
        clen = (ctypes.c_int64 * k)(*[len(h) for h in hold])
        srows = np.empty((k * 4096, 5), dtype=np.int64); crows = np.zeros((k, 10), dtype=np.int64)
        ns, cb, sb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        assert lib.cv_blosc_plan(src, clen, k, 1 << 22, k * 4096, srows.ctypes.data_as(ctypes.c_void_p),
                                 crows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ns), ctypes.byref(cb), ctypes.byref(sb)) == 0
        ns, cb, sb = ns.value, cb.value, sb.value
        slab = np.zeros(cb + 16, dtype=np.uint8)
        for i in range(k):
            slab[crows[i, 8]:crows[i, 8] + len(hold[i])] = hold[i]
        comp = torch.from_numpy(slab).cuda(); sr = torch.from_numpy(srows[:ns].copy()).cuda(); cr = torch.from_numpy(crows).cuda()
        scratch = torch.empty(sb + 16, dtype=torch.uint8, device="cuda"); sst = torch.zeros(ns, dtype=torch.uint8, device="cuda")
        out = torch.empty(k * 500 * 2112, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(k, dtype=torch.int64, device="cuda"); st = torch.zeros(k, dtype=torch.int32, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        dec = lambda: _lib.check(lib.cv_blosc_decode_dev(comp.data_ptr(), cb, sr.data_ptr(), ns, scratch.data_ptr(), sb, sst.data_ptr(), stream))
        unp = lambda: _lib.check(lib.cv_blosc_unpack_dev(cr.data_ptr(), k, sst.data_ptr(), ns, scratch.data_ptr(), sb, out.data_ptr(),
                                                         500 * 2112, lens.data_ptr(), st.data_ptr(), stream))
        xin = xd[:n].contiguous()
        o16 = m.predict_device(xin)
        seqs = "%d streams" % ns
        for name, fn in (("cv_blosc_decode_dev", dec), ("cv_blosc_unpack_dev", unp), ("forward pass", lambda: m.predict_device(xin, o16))):
            ms = []
            for r in range(8):
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                if r >= 2:
                    ms.append(e0.elapsed_time(e1))
            print("%s, %d candidates (%s): %-22s %.3f ms median (%.3f..%.3f)" % (layout, n, seqs, name, np.median(ms), min(ms), max(ms)), flush=True)
        assert int(st.sum()) == 0 and int((sst != 1).sum()) == 0
        print("%s, %d candidates: X batch on the host route %.2f ms (decode + copy of %.1f MB), on the device route %.2f ms "
              "(plan + gather + copy of %.1f MB + kernels + status)" % (layout, n, 1e3 * np.median(host), n * 2112 / 1e6,
                                                                       1e3 * np.median(dev), cb / 1e6), flush=True)
        os.unlink(binfn)
    m.close()


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    runs = int(opts.get("runs", 5))
    if "child" in opts:
        child(opts["bin"], opts["chk"], runs)
        return
    if not any(k in opts for k in ("ladder", "kernels")):
        print(__doc__)
        return
    layouts = opts.get("layouts", "cblosc,own,own64k").split(",")
    tmp = tempfile.mkdtemp(prefix="cv_bin_")
    try:
        from clairvoyante_amd import clairvoyante_v3, synth
        m = clairvoyante_v3.Clairvoyante()
        m.setParameters(synth.bench_params("full", seed=1))
        chk = os.path.join(tmp, "model-000001"); m.saveParameters(chk); m.close()
        if "kernels" in opts:
            kernels(int(opts["kernels"]), layouts, tmp, chk)
        if "ladder" in opts:
            ladder([int(v) for v in opts["ladder"].split(",")], runs, layouts, opts.get("parent"), tmp, chk)
    finally:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
