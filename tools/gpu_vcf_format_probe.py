"""Development probe: callVar's VCF records written by the host threads (cv_format_vcf behind ResultFetcher.fetch) against
the device route (cv_vcf_records_dev behind cv_call_postproc, CV_VCF_FORMAT=device).
    python tools/gpu_vcf_format_probe.py rungs=65536,262144,1000000 [runs=5] [parent=DIR] [log=FILE]
Per rung a plain text tensor file of that many rows is written once; callVar.Test runs over it behind a loaded model,
without and with --showRef, the routes alternating run by run in ONE process after one warm-up of each: seconds as median
(min..max) over `runs` runs, each ending in a device synchronise.  The VCF of the device route is compared with the
host's byte for byte before a time is printed, and vcf_format_counts must show that the device took every batch.
"wins" = every device run is faster than every host run.  parent=DIR names a built checkout of the PARENT commit: the same
runs in a child process in that tree.  Then, for one batch of 65 536 rows: the kernels of cv_vcf_records_dev by HIP events
beside cv_call_postproc and the forward pass, and the bytes that cross PCIe per batch on either side -- computed from the
shapes of what either route copies (callVar.ResultFetcher.fetch, fetch_text, enqueue_records), not observed."""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.environ.get("CV_PROBE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
_log = None


def say(text):
    print(text, flush=True)
    if _log:
        with open(_log, "a") as fh:
            fh.write(text + "\n")


def _fmt(v):
    v = np.array(v)
    return "%.3f (%.3f..%.3f)" % (np.median(v), v.min(), v.max())


def rows_array(n):
    """raw counts of n candidates (matrix 0 added back, nothing negative), as the text rows hold them"""
    from clairvoyante_amd import synth
    x = synth.make_candidates(n, seed=9, device="cuda").cpu().numpy()
    x[..., 1:] += x[..., 0:1]
    return np.maximum(x, 0)


def write_rows(path, n, x):
    from clairvoyante_amd.pileup import format_rows
    ref = b"N" * 83 + b"ACGT" * ((n + 200) // 4 + 8)
    with open(path, "wb") as fh:
        for s in range(0, n, len(x)):
            k = min(len(x), n - s)
            fh.write(b"\n".join(format_rows("chr1", np.arange(100 + s, 100 + s + k), ref, 0, x[:k])) + b"\n")


def model():
    import common
    from oracle import cv_oracle as O
    from clairvoyante_amd import clairvoyante_v3
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.setParameters(common.bench_params(O, "full", seed=11))
    return m


def timed(m, fn, out, show_ref, route):
    """one callVar.Test -> seconds"""
    import torch
    from clairvoyante_amd import callVar, utils_v2
    if route is None:
        os.environ.pop("CV_VCF_FORMAT", None)
    else:
        os.environ["CV_VCF_FORMAT"] = route
    a = types.SimpleNamespace(tensor_fn=fn, chkpnt_fn=None, call_fn=out, qual=None, sampleName="S", ref_fn=None, threads=None,
                              showRef=show_ref, v3=True, v2=False, slim=False)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    callVar.Test(a, m, utils_v2)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def child(fn, runs):
    """the PARENT commit over the same file, in its own tree (CV_PROBE_TREE): no route to choose"""
    m = model()
    out = fn + ".parent.vcf"
    res = {}
    for show_ref in (False, True):
        res[str(show_ref)] = [timed(m, fn, out, show_ref, None) for _ in range(runs + 1)][1:]
    os.unlink(out)
    print("CHILD " + json.dumps(res), flush=True)


def _run_child(parent, fn, runs):
    env = dict(os.environ, CV_PROBE_TREE=os.path.abspath(parent))
    env.pop("CV_VCF_FORMAT", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child=1", "fn=" + fn, "runs=%d" % runs], env=env,
                         stdout=subprocess.PIPE, check=True, timeout=900).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("CHILD ")][-1][6:])


def rung(m, tmp, n, x, runs, parent):
    from clairvoyante_amd import callVar
    fn = os.path.join(tmp, "t%d.txt" % n)
    write_rows(fn, n, x)
    par = _run_child(parent, fn, runs) if parent else None
    verdicts = []
    for show_ref in (False, True):
        out = {r: os.path.join(tmp, r + ".vcf") for r in ("host", "device")}
        for r in ("host", "device"):
            timed(m, fn, out[r], show_ref, r)                         # warm-up, and the text compared
        vcf = open(out["host"], "rb").read()
        assert open(out["device"], "rb").read() == vcf, "the device route's VCF is not the host's"
        before = callVar.vcf_format_counts()
        s = {"host": [], "device": []}
        for _ in range(runs):
            for r in ("host", "device"):
                s[r].append(timed(m, fn, out[r], show_ref, r))
        grew = {k: v - before[k] for k, v in callVar.vcf_format_counts().items()}
        assert grew["handed_over"] == 0 and grew["host"] == grew["device"] > 0, grew
        wins = max(s["device"]) < min(s["host"])
        verdicts.append(wins)
        say("%d rows, %s, %d records, %.1f MB of VCF | host %s s [%.0f rows/s] | device %s s [%.0f rows/s] | parent commit %s | device %s "
            "every host run" % (n, "--showRef" if show_ref else "variants only", sum(1 for l in vcf.splitlines() if not l.startswith(b"#")), len(vcf) / 1e6, _fmt(s["host"]),
                                n / np.median(s["host"]), _fmt(s["device"]), n / np.median(s["device"]),
                                _fmt(par[str(show_ref)]) + " s" if par else "not run", "WINS" if wins else "does not win"))
    os.unlink(fn)
    return verdicts


def one_batch(m, x, n=65536):
    """the kernels of one batch by HIP events, and the bytes that cross per batch on either side, computed from the shapes"""
    import torch
    from clairvoyante_amd import _lib, callVar
    from clairvoyante_amd.utils_v2 import PosBatch
    lib = _lib.load()
    raw = x[np.arange(n) % len(x)].copy()
    raw[..., 1:] -= raw[..., 0:1]
    xd = torch.from_numpy(raw).cuda()
    pos = PosBatch.from_columns("chr1", np.arange(100, 100 + n), [b"ACGTACGTACGTACGTACGTACGTACGTACGTA"] * n)
    _s, _r, buf, meta = pos.pieces()[0]
    tok = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).copy()).cuda()
    up_tok, up_meta = callVar._packed_tokens(buf, meta)             # what enqueue_records uploads for a batch whose tokens are on the host
    meta_d = torch.from_numpy(meta).cuda()
    need = ctypes.c_int64()
    _lib.check(lib.cv_vcf_records_workspace(n, ctypes.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    small = torch.empty(4 + n + 1, dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    cap = n * (int(meta[:, 1].max()) + 160)
    text = torch.empty(cap, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for show_ref in (0, 1):
        ms = {"forward": [], "postproc": [], "records": []}
        for _ in range(6):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            out = m.predict_device(xd)
            ev[1].record()
            call = torch.empty((n, 8), dtype=torch.int32, device="cuda"); qual = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            _lib.check(lib.cv_call_postproc(m._h, p(xd), p(out), n, p(call), p(qual), m._stream()))
            ev[2].record()
            _lib.check(lib.cv_vcf_records_dev(p(call), p(qual), n, p(xd), None, p(tok), p(meta_d), None, show_ref, 0, 0,
                                              ctypes.c_void_p(small.data_ptr() + 32), p(status), p(small), p(text), cap, p(ws), need.value,
                                              m._stream()))
            ev[3].record()
            torch.cuda.synchronize()
            for k, name in enumerate(("forward", "postproc", "records")):
                ms[name].append(ev[k].elapsed_time(ev[k + 1]))
        info = small[:4].cpu().numpy()
        kept = n if show_ref else int((call[:, 0] != 0).sum().item())
        say("one batch of %d rows, %s: kernels ms (median of 5 behind a warm-up): forward %.3f, cv_call_postproc %.3f, cv_vcf_records_dev "
            "(lengths, scan, write) %.3f | %d records, %d bytes of text | bytes crossing (computed from the shapes, not observed): host "
            "route %d down (call + qual %d, %d rows of 2 112) + %d up (their indices); device route %d down (info + text) + %d up (tokens + meta; none when the parser left them in HBM)"
            % (n, "--showRef" if show_ref else "variants only", np.median(ms["forward"][1:]), np.median(ms["postproc"][1:]),
               np.median(ms["records"][1:]), info[1], info[0], n * 48 + kept * 2112, n * 48, kept, kept * 8, 32 + info[0],
               up_tok.nbytes + up_meta.nbytes))
        assert info[2] == 0


def main():
    global _log
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    runs = int(kv.get("runs", 5))
    if "child" in kv:
        return child(kv["fn"], runs)
    import torch
    from clairvoyante_amd import _lib
    assert torch.cuda.is_available(), "the probe needs the GPU"
    _log = kv.get("log")
    say("seconds of callVar.Test, median (min..max) of %d runs; %d usable cores" % (runs, _lib.usable_cores()))
    sizes = [int(v) for v in kv.get("rungs", "65536,262144,1000000").split(",")]
    tmp = tempfile.mkdtemp(prefix="cv_vcfdev_")
    x = rows_array(min(max(sizes), 200000))
    m = model()
    verdict = [(n, rung(m, tmp, n, x, runs, kv.get("parent"))) for n in sizes]
    one_batch(m, x)
    say("the device route wins on: %s" % (", ".join("%d rows%s" % (n, "" if all(w) else " (--showRef only)" if w[1] else " (variants only)")
                                                    for n, w in verdict if any(w)) or "no rung"))
    m.close()
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
