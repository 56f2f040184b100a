"""Development probe: TrainingSet.blocks() of a resident synthetic set with the X blocks packed by the host threads
(CV_BIN_PACK=host: every row crosses, 2 112 bytes per candidate, then byte shuffle + LZ4 on 16 threads) against the device
route (CV_BIN_PACK=device: cv_blosc_pack_dev writes the chunks in HBM, the compressed form crosses).
    python tools/gpu_bin_pack_probe.py kernels=65536 ladder=16384,65536,200000,1000000 [runs=5] [parent=DIR]
Per rung, seconds of blocks() and of its "pack" part as median and range over `runs` runs after one warm-up, the two
routes alternating run by run in ONE process, and the bytes of the X blocks (and of all blocks) either route writes.  The
host route is timed in the layout it writes by default (one stream per chunk) and in the device route's (blocks of
65 536 bytes).  "wins" = every device run is faster than every host run.  parent=DIR names a built checkout of the PARENT
commit: its blocks() is timed on the same set in a child process.  kernels=N: HIP-event times of the three phases of
cv_blosc_pack_dev for N candidates, beside cv_trainset_gather over as many rows, and the bytes that cross on either
route.  The device route's X is compared with the set bit for bit before a time is printed."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.environ.get("CV_PROBE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _resident(n):
    """-> (X, Y, key_ctg, key_pos) in HBM: n synthetic candidates (100 000 distinct ones, repeated)"""
    import torch
    from clairvoyante_amd import synth
    k0 = min(n, 100000)
    xt, cls, rf, alt, il = synth.make_candidates(k0, seed=9, device="cuda", return_class=True)
    yt = synth.make_labels(cls, rf, alt, il)
    idx = torch.arange(n, device="cuda") % k0
    X, Y = xt[idx].contiguous(), yt[idx].contiguous()
    return X, Y, (idx % 3).to(torch.int32), torch.arange(n, device="cuda", dtype=torch.int64) * 3 + 1


def _set(res):
    from clairvoyante_amd import utils_v2
    X, Y, kc, kp = res
    return utils_v2.TrainingSet(int(X.shape[0]), X, Y, "device", names=[b"chr1", b"chr2", b"chrX"], key_ctg=kc, key_pos=kp)


def _blocks(res, route, blocksize=None):
    """-> (seconds of blocks(), seconds of its pack part, the blocks)"""
    import torch
    from clairvoyante_amd import utils_v2
    if route is None:
        os.environ.pop("CV_BIN_PACK", None)
    else:
        os.environ["CV_BIN_PACK"] = route
    utils_v2.PACK_BLOCKSIZE = blocksize
    ts = _set(res)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    b = ts.blocks()
    dt = time.perf_counter() - t0
    utils_v2.PACK_BLOCKSIZE = None
    return dt, ts.times["pack"], b


def _fmt(v):
    v = np.array(v)
    return "%.4f (%.4f..%.4f)" % (np.median(v), v.min(), v.max())


def child(n, runs):
    res = _resident(n)
    s = []
    for r in range(runs + 1):
        dt, _p, b = _blocks(res, None)
        if r:
            s.append(dt)
    print("CHILD " + json.dumps({"s": s, "xbytes": sum(len(c) for c in b[1])}), flush=True)


def _run_child(parent, n, runs):
    env = dict(os.environ, CV_PROBE_TREE=os.path.abspath(parent))
    env.pop("CV_BIN_PACK", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child=blocks", "n=%d" % n, "runs=%d" % runs], env=env,
                         stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    return json.loads([l for l in out.splitlines() if l.startswith("CHILD ")][-1][6:])


def ladder(sizes, runs, parent):
    import torch
    from clairvoyante_amd import utils_v2
    print("seconds, median (min..max) of %d runs" % runs)
    print("candidates | blocks() parent commit | blocks() host | host, 64 KiB blocks | device | pack part host | host 64 KiB | device | "
          "X MB host | host 64 KiB | device | all blocks MB host | device | X chunks of the timed device runs packed by the device/by the host", flush=True)
    for n in sizes:
        res = _resident(n)
        modes = (("host", "host", None), ("host64k", "host", 65536), ("device", "device", None))
        s = {k: [] for k, _r, _b in modes}; p = {k: [] for k, _r, _b in modes}; size = {}
        for r in range(runs + 1):                       # run 0 warms up; the routes alternate
            if r == 1:
                before = utils_v2.bin_pack_counts()     # (the chunk counts are the timed runs')
            for key, route, bsz in modes:
                dt, pk, b = _blocks(res, route, bsz)
                if r:
                    s[key].append(dt); p[key].append(pk)
                size[key] = (sum(len(c) for c in b[1]), sum(len(c) for lst in b[1:] for c in lst))
                if r == 0 and key == "device":
                    got = utils_v2.DecompressArray(b[1], 0, n, n)[0]
                    assert torch.equal(torch.from_numpy(np.ascontiguousarray(got)).cuda().view(torch.int32), res[0].view(torch.int32)), \
                        "the device route's X is not the set"
                del b
        after = utils_v2.bin_pack_counts()
        par = "not run"
        if parent:
            got = _run_child(parent, n, runs)
            assert got["xbytes"] == size["host"][0], "the parent commit writes other X blocks"
            par = _fmt(got["s"])
        print("%d | %s | %s | %s | %s | %s | %s | %s | %.1f | %.1f | %.1f | %.1f | %.1f | %d/%d; blocks(): device %s every host run" %
              (n, par, _fmt(s["host"]), _fmt(s["host64k"]), _fmt(s["device"]), _fmt(p["host"]), _fmt(p["host64k"]), _fmt(p["device"]),
               size["host"][0] / 1e6, size["host64k"][0] / 1e6, size["device"][0] / 1e6, size["host"][1] / 1e6, size["device"][1] / 1e6,
               after["device"] - before["device"], after["host"] - before["host"],
               "WINS" if max(s["device"]) < min(s["host"]) else "does not win"), flush=True)
        del res
        torch.cuda.empty_cache()


def kernels(n):
    """HIP-event times of the three phases for the full chunks of n candidates, in pieces as the route cuts them, beside
    cv_trainset_gather over as many rows"""
    import torch
    from clairvoyante_amd import _lib, utils_v2
    lib = _lib.load()
    X, Y = _resident(n)[:2]
    bs, row = 500, 2112
    chunks_all = n // bs
    head, tail = utils_v2.pickle_envelope((bs, 33, 4, 4), np.float32)
    piece = utils_v2.PACK_PIECE_CHUNKS
    ws_b, bound = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.cv_blosc_pack_workspace(piece, len(head) + bs * row + len(tail), 4, 65536, ctypes.byref(ws_b), ctypes.byref(bound)))
    ws = torch.empty(ws_b.value, dtype=torch.uint8, device="cuda")
    slab = torch.empty(bound.value, dtype=torch.uint8, device="cuda")
    state = torch.empty(12 * piece + 32, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = {0: [], 1: [], 2: [], "all": [], "gather": []}
    comp = 0
    for r in range(6):
        tot = {k: 0.0 for k in times}
        comp = 0
        for c0 in range(0, chunks_all, piece):
            k = min(piece, chunks_all - c0)
            args = (X.data_ptr() + c0 * bs * row, k, bs * row)
            tail_args = (4, 65536, slab.data_ptr(), bound.value, state.data_ptr(), state.data_ptr() + 8 * (k + 1), ws.data_ptr(), ws_b.value, st)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            _lib.check(lib.cv_blosc_pack_dev(*args, head, len(head), tail, len(tail), *tail_args))
            ev[1].record()
            for ph in range(3):
                _lib.check(lib.cv_blosc_pack_phase_dev(ph, *args, len(head), len(tail), *tail_args))
                ev[2 + ph].record()
            torch.cuda.synchronize()
            tot["all"] += ev[0].elapsed_time(ev[1])
            for ph in range(3):
                tot[ph] += ev[1 + ph].elapsed_time(ev[2 + ph])
            comp += int(state[8 * k:8 * (k + 1)].view(torch.int64).item())
        # the gather that leaves the set where blocks() finds it: as many rows through cv_trainset_gather
        m = chunks_all * bs
        src = torch.arange(m, device="cuda", dtype=torch.int64)
        perm = torch.randperm(m, device="cuda")
        xo, yo = torch.empty_like(X[:m]), torch.empty((m, 16), dtype=torch.float32, device="cuda")
        ys = Y[:m].to(torch.float32).contiguous()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.cv_trainset_gather(X.data_ptr(), ys.data_ptr(), src.data_ptr(), perm.data_ptr(), m, xo.data_ptr(), yo.data_ptr(), st))
        e1.record(); torch.cuda.synchronize()
        tot["gather"] = e0.elapsed_time(e1)
        if r:
            for k2 in times:
                times[k2].append(tot[k2])
    med = {k: float(np.median(v)) for k, v in times.items()}
    print("kernels, %d candidates (%d chunks in pieces of %d), ms, median of 5: encode %.3f | layout %.3f | assemble %.3f | the three in one "
          "call %.3f | cv_trainset_gather %.3f || bytes to the host: host route %.1f MB, device route %.1f MB" %
          (chunks_all * bs, chunks_all, piece, med[0], med[1], med[2], med["all"], med["gather"], chunks_all * bs * row / 1e6, comp / 1e6), flush=True)


def main():
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    runs = int(kv.get("runs", 5))
    if "child" in kv:
        return child(int(kv["n"]), runs)
    import torch
    assert torch.cuda.is_available(), "the probe needs the GPU"
    if "kernels" in kv:
        kernels(int(kv["kernels"]))
    if "ladder" in kv:
        ladder([int(v) for v in kv["ladder"].split(",")], runs, kv.get("parent"))


if __name__ == "__main__":
    main()
