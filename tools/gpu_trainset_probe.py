"""Development probe: the labelled training set from text tensors (utils_v2.GetTrainingArray / GetTrainingSetDevice), host
loop against the device route, plain and BGZF input.
    python tools/gpu_trainset_probe.py ladder=16384,65536,200000,1000000 [runs=5] [hostruns=5] [hostmax=200000]
Per rung and form: the host loop (CV_TEXT_PARSE=host: the loop GetTrainingArray had before the device route existed),
the device route to a resident set, the device route to blocks with its parts (read + parse, tokens + join, finish +
gather, shuffle, keys, pack), rows/s as median and range; above `hostmax` rows the host loop is timed `hostruns` times
only (it takes about a minute per million rows).  The last column says whether the device route to blocks beat the host
loop in every run.
    python tools/gpu_trainset_probe.py kernels=200000
HIP-event times of the new kernels beside the parse kernels of the same rows (one slab)."""
import ctypes
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def _write(tmp, n):
    """n rows on three contigs in runs, a truth file (every 50th site) and a BED file that keeps ~90 % of the rows"""
    import gzip
    import torch
    from clairvoyante_amd import bgzf, synth
    from clairvoyante_amd.pileup import format_rows
    k0 = min(n, 100000)
    x = synth.make_candidates(k0, seed=9, device="cuda").cpu().numpy()
    x[..., 1:] += x[..., 0:1]
    x = np.maximum(x, 0)
    torch.cuda.empty_cache()
    txt = os.path.join(tmp, "t%d.txt" % n)
    ref = b"N" * 83 + b"ACGT" * ((n + 200) // 4 + 8)
    truth, per = [], (n + 2) // 3
    with open(txt, "wb") as fh:
        for c, ctg in enumerate(("chr1", "chr10", "chr2")):
            lo, hi = c * per, min((c + 1) * per, n)
            for s in range(lo, hi, k0):
                k = min(k0, hi - s)
                fh.write(b"\n".join(format_rows(ctg, np.arange(100 + s, 100 + s + k), ref, 0, x[:k])) + b"\n")
            truth += ["%s %d A C 0 1" % (ctg, p) for p in range(100 + lo, 100 + hi, 50)]
    var, bed = txt + ".var.gz", txt + ".bed.gz"
    with gzip.open(var, "wt") as fh:
        fh.write("\n".join(truth) + "\n")
    with gzip.open(bed, "wt") as fh:
        fh.write("".join("%s %d %d\n" % (ctg, s, s + 900) for ctg in ("chr1", "chr10", "chr2") for s in range(0, n + 1000, 1000)))
    bgzf.reblock(txt, txt + ".bgzf.gz", level=1)
    return {"plain": txt, "bgzf": txt + ".bgzf.gz"}, var, bed


def _fmt(v):
    v = np.array(v)
    return "%.3g (%.3g..%.3g)" % (np.median(v), v.min(), v.max())


def ladder(sizes, runs, hostruns, hostmax):
    import torch
    from clairvoyante_amd import utils_v2
    tmp = tempfile.mkdtemp(prefix="cv_trainset_")
    print("rows form bytes | host rows/s | device->resident rows/s | device->blocks rows/s | verdict", flush=True)
    for n in sizes:
        t0 = time.time()
        forms, var, bed = _write(tmp, n)
        print("# wrote %d rows in %.0f s" % (n, time.time() - t0), flush=True)
        for form, fn in forms.items():
            host, res, blk, parts, total = [], [], [], {}, None
            nh = runs if n <= hostmax else hostruns
            for r in range(runs + 1):                           # run 0 warms up
                if (0 if n <= hostmax else 1) <= r <= nh:          # (no warm-up run of the host loop above hostmax)
                    os.environ["CV_TEXT_PARSE"] = "host"
                    random.seed(1); t0 = time.perf_counter()
                    got = utils_v2.GetTrainingArray(fn, var, bed)
                    dt = time.perf_counter() - t0
                    total = got[0]; del got
                    if r:
                        host.append(n / dt)
                    print("#   host run %d: %.2f s" % (r, dt), flush=True)
                random.seed(1); torch.cuda.synchronize(); t0 = time.perf_counter()
                ts = utils_v2.GetTrainingSetDevice(fn, var, bed)
                torch.cuda.synchronize(); t1 = time.perf_counter()
                ts.blocks()
                t2 = time.perf_counter()
                assert ts.route == "device" and total in (None, ts.total), (ts.route, ts.reason, ts.total, total)
                if r:
                    res.append(n / (t1 - t0)); blk.append(n / (t2 - t0))
                    for k, v in ts.times.items():
                        parts.setdefault(k, []).append(v * 1e3)
                del ts
            wins = len(host) > 0 and min(blk) > max(host)
            print("%8d %-5s %11d | %s [%d runs] | %s | %s | %s" % (n, form, os.path.getsize(fn), _fmt(host or [0.0]), len(host), _fmt(res), _fmt(blk),
                                                                    "device wins every run" if wins else "device does not win every run"), flush=True)
            print("         parts of the device route, ms median: " + ", ".join("%s %.1f" % (k, np.median(v)) for k, v in parts.items()), flush=True)
            os.unlink(fn)
        os.unlink(var); os.unlink(bed)
    os.environ.pop("CV_TEXT_PARSE", None)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


def kernels(n):
    """one slab of n rows: index + parse, then tokens, join, finish, gather (HIP events)"""
    import torch
    from clairvoyante_amd import _lib, utils_v2
    lib = _lib.load()
    tmp = tempfile.mkdtemp(prefix="cv_trainset_")
    forms, var, bed = _write(tmp, n)
    text = open(forms["plain"], "rb").read()
    tree, Y = utils_v2._read_bed_truth(var, bed)
    names, t = utils_v2._trainset_tables(tree, Y, True)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    P = lambda x: ctypes.c_void_p(x.data_ptr()) if x.numel() else None
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    need = ctypes.c_int64()
    _lib.check(lib.cv_parse_tensor_text_dev_workspace(len(text), n, ctypes.byref(need)))
    buf = torch.cat([torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda(), torch.zeros(64, dtype=torch.uint8, device="cuda")])
    xd, meta, status, info = E((n, 528), torch.float32), E((n, 6), torch.int64), E(n, torch.uint8), E(4, torch.int64)
    ws = E(need.value, torch.uint8)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pos, run, ctg, truth = E(n, torch.int64), E(n, torch.int32), E(n, torch.int32), E(n, torch.int32)
    digits, centre, flags, keep = (E(n, torch.uint8) for _ in range(4))
    _lib.check(lib.cv_trainset_tokens_workspace(n, ctypes.byref(need))); ws_t = E(need.value, torch.uint8); need_t = need.value
    _lib.check(lib.cv_trainset_finish_workspace(n, ctypes.byref(need))); ws_f = E(need.value, torch.uint8); need_f = need.value
    tab = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
    run_ctg = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    rank = torch.from_numpy(utils_v2.contig_ranks(names)).cuda()
    src, ys, total = E(n, torch.int64), E((n, 16), torch.float32), E(1, torch.int64)
    xo, yo = E((n, 528), torch.float32), E((n, 16), torch.float32)

    def parse():
        _lib.check(lib.cv_parse_tensor_text_dev(P(buf), len(text), n, P(xd), P(meta), P(status), P(info), P(ws), ws.numel(), st))

    def tokens():
        _lib.check(lib.cv_trainset_tokens(P(buf), P(meta), None, n, P(pos), P(digits), P(centre), P(flags), P(run), P(ws_t), need_t, st))

    def join():
        _lib.check(lib.cv_trainset_join(n, P(run), P(run_ctg), 3, P(pos), len(names), 1, P(tab["bed_off"]), P(tab["bed_begin"]), P(tab["bed_emax"]),
                                        P(tab["truth_off"]), P(tab["truth_pos"]), P(ctg), P(keep), P(truth), st))

    def finish():
        _lib.check(lib.cv_trainset_finish(n, P(ctg), P(pos), P(digits), P(centre), P(keep), P(truth), P(rank), len(names), P(tab["labels"]),
                                          len(t["labels"]), P(src), P(ys), P(total), P(ws_f), need_f, st))

    def gather():
        _lib.check(lib.cv_trainset_gather(P(xd), P(ys), P(src), None, int(total.item()), P(xo), P(yo), st))

    for name, fn in (("index + parse", parse), ("tokens", tokens), ("join", join), ("finish (keys, sort, entries, labels)", finish),
                     ("gather", gather)):
        ms = []
        for r in range(8):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            if r >= 3:
                ms.append(e0.elapsed_time(e1))
        print("%d rows, %.1f MB of text: %-40s %.3f ms median (%.3f..%.3f)" % (n, len(text) / 1e6, name, np.median(ms), min(ms), max(ms)), flush=True)
    assert int(run.max().item()) == 2 and int(flags.cpu().numpy().astype(np.int64).sum()) == 3
    print("%d rows kept of %d" % (int(total.item()), n))


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    if "kernels" in opts:
        kernels(int(opts["kernels"]))
    if "ladder" in opts:
        ladder([int(v) for v in opts["ladder"].split(",")], int(opts.get("runs", 5)), int(opts.get("hostruns", 5)), int(opts.get("hostmax", 200000)))
    if "kernels" not in opts and "ladder" not in opts:
        print(__doc__)


if __name__ == "__main__":
    main()
