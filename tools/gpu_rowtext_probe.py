"""Development probe: the text rows of CreateTensor made by the host loop (pileup.format_rows: one call per row) against
the device route (pileup.format_rows_device: cv_tensor_rows_text_dev writes them in HBM, one block of bytes per batch),
and what then bounds each sink of OutputAlnTensor.
    python tools/gpu_rowtext_probe.py rungs=16384,65536,262144,1000000 [runs=5] [sink_rows=65536] [parent=DIR] [log=FILE]
The tensors come from synth_pileup.fast_alignments through the pileup itself (a candidate at every position, depth 30).
Per rung, seconds as median (min..max) over `runs` runs, the routes alternating run by run in ONE process after one
warm-up of each: the rows made and joined (nothing written), and OutputAlnTensor's write loop into /dev/null; the two
kernel launches of a batch by HIP events beside the pileup's own finalize kernel.  "wins" = every device run is faster
than every host run.  At sink_rows rows (the compressing sinks run at one core's rate whatever the size): the write loop
into `gzip -c`, into BGZF with threads=1 and with the default pool, on either route.  parent=DIR names a built checkout of
the PARENT commit: its write loop (two writes per row) and its BgzfWriter are timed on the same tensors in a child
process.  The device route's text is compared with the host's byte for byte before a time is printed."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("CV_PROBE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CTG = "chr21"
_log = None


def say(text):
    print(text, flush=True)
    if _log:
        with open(_log, "a") as fh:
            fh.write(text + "\n")


def tensors(n):
    """-> (centres [n] int64, reference bytes, tensors [n,33,4,4] fp32 in HBM, finalize ms of the pileup)"""
    from clairvoyante_amd import synth_pileup as sp
    from clairvoyante_amd.pileup import Pileup
    ref_len = n + 400
    ref, sam = sp.fast_alignments(ref_len // 5, ref_len, seed=11, ctg=CTG)
    pl = Pileup()
    pl.set_reference(ref, 0)
    pl.set_candidates(np.arange(100, 100 + n, dtype=np.int64))
    for s in range(0, len(sam), 8 << 20):
        pl.add_sam(sam[s:s + (8 << 20)])
    t, _d, _u = pl.finish()
    ms = pl.stats()["finalize_ms"]
    centres = pl.centers.copy()
    pl.close()
    return centres, ref, t, ms


def _fmt(v):
    v = np.array(v)
    return "%.4f (%.4f..%.4f)" % (np.median(v), v.min(), v.max())


def _rate(n, v):
    return "%.0f rows/s" % (n / np.median(np.array(v)))


def blocks(route, centres, ref, t):
    """the rows of one call as blocks, by the named route -> list of bytes"""
    from clairvoyante_amd import pileup
    os.environ["CV_ROW_FORMAT"] = route
    return list(pileup.format_row_blocks(CTG, centres, ref, 0, t))


def parent_loop(write, centres, ref, t):
    """OutputAlnTensor's loop as the parent commit runs it: one call and two writes per row"""
    from clairvoyante_amd.pileup import format_rows
    for s in range(0, len(centres), 32768):
        host = t[s:s + 32768].cpu().numpy()
        for row in format_rows(CTG, centres[s:s + 32768], ref, 0, host):
            write(row)
            write(b"\n")


def write_loop(route, sink, centres, ref, t):
    """OutputAlnTensor's write loop into a sink -> seconds, sink closed and waited for"""
    import torch
    from clairvoyante_amd import pileup, utils_v2
    os.environ["CV_ROW_FORMAT"] = route
    torch.cuda.synchronize(); t0 = time.perf_counter()
    null = open(os.devnull, "wb")
    proc = None
    if sink == "null":
        out = null
    elif sink == "gzip":
        proc = subprocess.Popen(["gzip", "-c"], stdin=subprocess.PIPE, stdout=null, bufsize=8388608)
        out = proc.stdin
    else:
        out = utils_v2.BgzfWriter(null, threads=1) if sink == "bgzf1" else utils_v2.BgzfWriter(null)
    for block in pileup.format_row_blocks(CTG, centres, ref, 0, t):
        out.write(block)
    if out is not null:
        out.close()
    if proc is not None:
        proc.wait()
    null.close()
    return time.perf_counter() - t0


def kernel_ms(centres, ref, t):
    """HIP-event ms of the length-only call and of the writing call (which runs the lengths again) over all batches"""
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = t.device
    rf = torch.from_numpy(np.frombuffer(ref, dtype=np.uint8).copy()).to(dev)
    need = ctypes.c_int64(0)
    _lib.check(lib.cv_tensor_rows_text_workspace(32768, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    cb = CTG.encode()
    tot = [0.0, 0.0]
    nbytes = 0
    for s in range(0, len(centres), 32768):
        n = min(32768, len(centres) - s)
        cen = torch.from_numpy(centres[s:s + n]).to(dev)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        args = (cb, len(cb), cen.data_ptr(), n, rf.data_ptr(), 0, rf.numel(), t[s:s + n].data_ptr(), off.data_ptr(), status.data_ptr())
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _lib.check(lib.cv_tensor_rows_text_dev(*args, None, 0, ws.data_ptr(), need.value, st))
        ev[1].record()
        total = int(off[n].item())
        text = torch.empty(total, dtype=torch.uint8, device=dev)
        ev[2].record()
        _lib.check(lib.cv_tensor_rows_text_dev(*args, text.data_ptr(), total, ws.data_ptr(), need.value, st))
        ev[3].record()
        torch.cuda.synchronize()
        tot[0] += ev[0].elapsed_time(ev[1]); tot[1] += ev[2].elapsed_time(ev[3])
        nbytes += total
    return tot[0], tot[1], nbytes


def child(n, runs, sink_rows):
    """the PARENT commit's loop, in its own tree (CV_PROBE_TREE)"""
    import torch
    from clairvoyante_amd import utils_v2
    centres, ref, t, _ms = tensors(n)
    null = open(os.devnull, "wb")
    s_null, s_bgzf = [], []
    for r in range(runs + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        parent_loop(null.write, centres, ref, t)
        if r:
            s_null.append(time.perf_counter() - t0)
        print("  parent commit, %d rows, run %d: %.2f s" % (n, r, time.perf_counter() - t0), file=sys.stderr, flush=True)
    if n == sink_rows:
        for r in range(runs):
            t0 = time.perf_counter()
            w = utils_v2.BgzfWriter(null)
            parent_loop(w.write, centres, ref, t)
            w.close()
            s_bgzf.append(time.perf_counter() - t0)
    print("CHILD " + json.dumps({"null": s_null, "bgzf": s_bgzf}), flush=True)


def _run_child(parent, n, runs, sink_rows):
    env = dict(os.environ, CV_PROBE_TREE=os.path.abspath(parent))
    env.pop("CV_ROW_FORMAT", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child=1", "n=%d" % n, "runs=%d" % runs, "sink_rows=%d" % sink_rows],
                         env=env, stdout=subprocess.PIPE, check=True, timeout=900).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("CHILD ")][-1][6:])


def rung(n, runs, sink_rows, parent, warm):
    import torch
    from clairvoyante_amd import _lib, pileup
    centres, ref, t, fin_ms = tensors(n)
    assert len(centres) == n
    if warm:
        blocks("host", centres[:4096], ref, t[:4096])
    dev = blocks("device", centres, ref, t)                     # (warms the device route up, and is the text compared)
    pileup.row_format_counts(reset=True)
    s = {"host": [], "device": []}
    w = {"host": [], "device": []}
    digest = {}
    for r in range(runs):
        for route in ("host", "device"):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            b = blocks(route, centres, ref, t)
            s[route].append(time.perf_counter() - t0)
            if r == 0:
                h = hashlib.sha256()
                for x in b:
                    h.update(x)
                digest[route] = (h.hexdigest(), sum(len(x) for x in b))
            del b
            w[route].append(write_loop(route, "null", centres, ref, t))
            print("  %d rows, run %d, %s: %.3f s made, %.3f s written" % (n, r, route, s[route][-1], w[route][-1]), file=sys.stderr, flush=True)
    del dev
    assert digest["host"] == digest["device"], "the device route's text is not the host's"
    counts = pileup.row_format_counts()
    assert counts == {"host": 2 * runs * n, "device": 2 * runs * n}, counts
    k = [kernel_ms(centres, ref, t) for _ in range(runs + 1)][1:]
    par = None
    if parent:
        par = _run_child(parent, n, runs, sink_rows)
    wins = max(s["device"]) < min(s["host"]) and max(w["device"]) < min(w["host"]) and (par is None or max(w["device"]) < min(par["null"]))
    say("%d rows, %.1f MB of text | rows made: host %s [%s], device %s [%s] | write loop into /dev/null: parent commit %s, host %s, device "
        "%s [%s] | kernels ms: lengths %.3f, lengths + write %.3f, pileup_finalize %.3f | device %s every host run" %
        (n, digest["host"][1] / 1e6, _fmt(s["host"]), _rate(n, s["host"]), _fmt(s["device"]), _rate(n, s["device"]),
         _fmt(par["null"]) if par else "not run", _fmt(w["host"]), _fmt(w["device"]), _rate(n, w["device"]),
         np.median([a for a, _b, _c in k]), np.median([b for _a, b, _c in k]), fin_ms, "WINS" if wins else "does not win"))
    if n == sink_rows:
        for sink in ("gzip", "bgzf1", "bgzf"):
            z = {"host": [], "device": []}
            for r in range(runs):
                for route in ("host", "device"):
                    z[route].append(write_loop(route, sink, centres, ref, t))
            name = {"gzip": "gzip -c", "bgzf1": "BGZF threads=1", "bgzf": "BGZF threads=%d" % min(16, _lib.usable_cores())}[sink]
            extra = " | parent commit (its loop, its serial writer) %s" % _fmt(par["bgzf"]) if par and sink == "bgzf" else ""
            say("  sink %s, %d rows: host route %s [%s], device route %s [%s]%s" %
                (name, n, _fmt(z["host"]), _rate(n, z["host"]), _fmt(z["device"]), _rate(n, z["device"]), extra))
    del t
    torch.cuda.empty_cache()
    return wins


def main():
    global _log
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    runs = int(kv.get("runs", 5))
    sink_rows = int(kv.get("sink_rows", 65536))
    if "child" in kv:
        return child(int(kv["n"]), runs, sink_rows)
    import torch
    from clairvoyante_amd import _lib
    assert torch.cuda.is_available(), "the probe needs the GPU"
    _log = kv.get("log")
    say("seconds, median (min..max) of %d runs; %d usable cores" % (runs, _lib.usable_cores()))
    sizes = [int(v) for v in kv.get("rungs", "16384,65536,262144,1000000").split(",")]
    verdict = [(n, rung(n, runs, sink_rows, kv.get("parent"), i == 0)) for i, n in enumerate(sizes)]
    first = next((n for i, (n, _w) in enumerate(verdict) if all(w for _n, w in verdict[i:])), None)
    say("ROWTEXT_DEVICE_MIN_ROWS by these runs: %s" % ("None (the device route wins from no rung on)" if first is None else
                                                       "0 (it wins from the first rung)" if first == sizes[0] else first))


if __name__ == "__main__":
    main()
