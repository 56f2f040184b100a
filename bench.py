#!/usr/bin/env python
"""bench.py -- candidate tensors/sec of the v3 inference hot path on MI355X.

A "step" is one pass of the hot path (conv1..conv3 + pools, fc4, fc5, four heads) over one
batch of 65 536 synthetic [33,4,4] pileup tensors that are already resident in HBM
(BASELINE.json configs[1]: "v3 inference, 4M synthetic tensors, batch 65536, 1 MI355X";
64 steps = the 4 194 304-tensor set).  With --gpus N every rank runs the same number of
steps on its own shard (candidates are independent: no data-path collective) and the value
is the whole-job rate.  One JSON line is printed by rank 0.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line.  What else the line can carry
(the slim and training legs, the training parity check, the host legs, the CPU baselines and the parity block; in
--mode pileup the CPU leg) runs only with --full, outside every timed region.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCH = 65536
FLOP_EXACT = {"full": 6768960, "slim": 2583264}
# algorithmic FLOP per candidate of each kernel stage (exact, padding taps excluded)
STAGE_FLOP = {   # 2 x exact MACs (SAME-padding taps excluded) of conv1, conv2, conv3, fc4, fc5, heads
    "full": [2 * 25344, 2 * 350208, 2 * 1400832, 2 * 1548288, 2 * 56448, 2 * 3360],
    "slim": [2 * 12672, 2 * 148992, 2 * 976896, 2 * 152064, 2 * 648, 2 * 360],
}
STAGE_NAMES = ["conv1+pool1", "conv1+pool1+conv2+pool2 (fused)", "conv3+pool3", "fc4", "fc5", "heads"]
PEAK_FP32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md (f32-in MFMA = vector rate)
PEAK_HBM_GBS = 8000.0


def usable_cores():
    from clairvoyante_amd._lib import usable_cores as f
    return f()


def cpu_baseline(arch, P, x_sample, target_s=12.0):
    """The oracle (C restatement, OpenMP) timed on this box's host cores on a bounded sample:
    whole passes over the sample until ~target_s seconds of CPU work have been done."""
    from oracle import cv_oracle as O
    cores = usable_cores()
    O.predict(arch, P, x_sample[:4096], nthreads=cores)            # warm-up (thread pool, page faults)
    t0 = time.time(); out = O.predict(arch, P, x_sample, nthreads=cores); dt = time.time() - t0
    passes, total = 1, dt
    while total < target_s and passes < 64:
        t0 = time.time(); O.predict(arch, P, x_sample, nthreads=cores); total += time.time() - t0
        passes += 1
    n = x_sample.shape[0]
    return {"value": n * passes / total, "unit": "candidates/s", "cores": cores, "kind": "port",
            "sample": "%d pass(es) over the first %d candidates of the timed set, oracle/cv_oracle.c, "
                      "%d OpenMP threads, %.1f s" % (passes, n, cores, total)}, out, n


def cpu_torch_line(arch, P, x_sample, ref_out, hip_out=None, target_s=6.0):
    """Second CPU line: the same network in stock torch CPU ops (oneDNN convolutions / GEMMs,
    fp32) -- the closest stand-in available here for the reference's TensorFlow-CPU kernels.  Not bit-identical
    to the oracle (library summation order); its distance to the oracle is reported, and -- the nearest thing to
    north_star's "argmax agreement vs TF-CPU" this image allows -- the per-head argmax agreement of the HIP output
    with THIS library's fp32 results (another summation order, as TF-Eigen's is).  -> (dict, its outputs)"""
    import numpy as np
    import torch
    import torch_ref
    import common
    cores = usable_cores()
    torch.set_num_threads(cores)
    bs = 8192
    with torch.no_grad():
        torch_ref.forward(arch, P, x_sample[:bs], dtype=torch.float32)                 # warm-up
        t0 = time.time(); done = 0; outs = []
        while time.time() - t0 < target_s and done < len(x_sample):
            outs.append(torch_ref.forward(arch, P, x_sample[done:done + bs], dtype=torch.float32)["out"].numpy())
            done += bs
        dt = time.time() - t0
    got = np.concatenate(outs)
    n = got.shape[0]
    line = {"value": n / dt, "unit": "candidates/s", "cores": cores, "kind": "torch CPU ops (oneDNN), fp32 -- a "
            "stand-in for TF-CPU, not the reference", "sample": "first %d candidates of the timed set, %.1f s" % (n, dt),
            "max_abs_dprob_vs_oracle": float(np.abs(got - ref_out[:n]).max())}
    if hip_out is not None:
        line["n"] = n
        line["argmax_match_per_head"] = common.argmax_match(hip_out[:n], got)      # HIP path vs this library, all n
        line["max_abs_dprob_vs_hip"] = float(np.abs(got - hip_out[:n]).max())
    return line, got


def relaunch_under_torchrun(args, argv):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks here (one process per GPU,
    torch.distributed.run on 127.0.0.1) with the same arguments and pass their output and exit code through."""
    import socket
    import subprocess
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    sys.exit(subprocess.call(cmd, env=env))


_REAL_STDOUT = [None]      # the process's real stdout: ONLY the JSON line goes there
_CAPTURE = [None]          # what libraries write to file descriptor 1 meanwhile (RCCL's banner and INFO log) lands here


def protect_stdout():
    """The driver reads ONE JSON line from rank 0's stdout.  Libraries write there too (RCCL prints its version banner
    and, at NCCL_DEBUG=INFO, its log to fd 1), so fd 1 is pointed at a scratch file for the whole run: emit() writes the
    line to the saved descriptor, release_stdout() forwards the captured chatter to stderr."""
    import tempfile
    if _REAL_STDOUT[0] is not None:
        return
    sys.stdout.flush()
    real = os.dup(1)
    cap = tempfile.NamedTemporaryFile(prefix="cv_bench_fd1_", suffix=".log", delete=False)
    os.dup2(cap.fileno(), 1)
    cap.close()
    _REAL_STDOUT[0] = os.fdopen(real, "w")
    _CAPTURE[0] = cap.name


def _flush_c_stdio():
    """RCCL prints through C stdio, which buffers fully when fd 1 is a file: push it out before the capture is read"""
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def emit(line):
    out = _REAL_STDOUT[0] or sys.stdout
    out.write(json.dumps(line) + "\n")
    out.flush()


def release_stdout():
    fn = _CAPTURE[0]
    if not fn:
        return
    try:
        sys.stdout.flush()
        _flush_c_stdio()
        with open(fn, errors="replace") as f:
            text = f.read()
        if text.strip():
            sys.stderr.write(text if len(text) < 20000 else text[:20000] + "\n[... %d more bytes of library output]\n" % (len(text) - 20000))
        os.remove(fn)
    except OSError:
        pass
    _CAPTURE[0] = None


def rccl_logging():
    """Before the process group exists: ask RCCL for its INFO log (init, topology graph; with CV_RCCL_TUNING_LOG=1 also the
    per-collective algorithm / protocol choice); it arrives on fd 1, i.e. in the capture file, and rank 0 says ONCE in
    the line what the exchange ran on (rccl_summary).  Nothing is touched when the user set NCCL_DEBUG, the backend is not RCCL, or there is one rank."""
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    if (ws <= 1 and not os.environ.get("CV_FORCE_DIST")) or "NCCL_DEBUG" in os.environ:
        return
    if (os.environ.get("CV_DIST_BACKEND") or "nccl") != "nccl":
        return
    os.environ["NCCL_DEBUG"] = "INFO"
    # INIT + GRAPH are written once, when the communicator is built (version, channels, rings / trees, transports).  TUNING
    # adds one line per collective CALL (algorithm / protocol / predicted time) -- inside the timed loop too, so it is
    # opt-in: CV_RCCL_TUNING_LOG=1 for a run whose purpose is to read those choices, not to be timed.
    os.environ["NCCL_DEBUG_SUBSYS"] = "INIT,GRAPH,TUNING" if os.environ.get("CV_RCCL_TUNING_LOG") else "INIT,GRAPH"


def rccl_summary(max_lines=8):
    """-> dict from this process's RCCL INFO log (None if there is none): library version, channel counts, transports
    between peers, and the distinct (collective, bytes, algorithm, protocol) choices it logged."""
    import re
    fn = _CAPTURE[0]
    if not fn or not os.path.exists(fn):
        return None
    try:
        sys.stdout.flush()
        _flush_c_stdio()
        text = open(fn, errors="replace").read()
    except OSError:
        return None
    if "NCCL" not in text and "RCCL" not in text:
        return None
    out = {"log_bytes": len(text)}
    mo = re.search(r"(RCCL|NCCL) version\s*:?\s*([^\n]+)", text)
    if mo:
        out["version"] = mo.group(0).strip()[:120]
    mo = re.search(r"(\d+) coll channels[^\n]*", text)
    if mo:
        out["channels"] = mo.group(0).strip()[:160]
    tr = {}
    for mo in re.finditer(r" via ([A-Za-z0-9_/ ]+?)(?:\n|$|\s+comm)", text):
        k = mo.group(1).strip()
        tr[k] = tr.get(k, 0) + 1
    if tr:
        out["transports"] = tr
    seen, choices = set(), []
    for ln in text.splitlines():
        low = ln.lower()
        if "algo" in low and "proto" in low:
            body = re.sub(r"^.*?(NCCL|RCCL) INFO ", "", ln)
            key = re.sub(r"time [-0-9.e+]+", "", body)
            if key not in seen:
                seen.add(key); choices.append(body.strip()[:200])
    if choices:
        out["algo_proto"] = choices[:max_lines]
        out["algo_proto_distinct"] = len(choices)
    return out


def init_ranks(args):
    """-> (rank, world size, local rank).  A line whose n_gpus is not --gpus is never printed: mismatch = exit 2."""
    from clairvoyante_amd import parallel
    rccl_logging()
    rank, ws, local = parallel.init_from_env()
    if os.environ.get("CV_SHARE_DEVICES"):       # functional test on a box with fewer GPUs than ranks (backend gloo): ranks share devices
        import torch
        local %= max(torch.cuda.device_count(), 1)
    if ws != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but %d rank(s) are running (WORLD_SIZE); refusing to report a line whose "
                  "n_gpus differs from the request" % (args.gpus, ws), file=sys.stderr)
        finish_ranks()
        sys.exit(2)
    verify_ranks(args, rank, ws, local)
    return rank, ws, local


_RANK_CHECK = {}


def verify_ranks(args, rank, ws, local):
    """BEFORE anything is timed: the ranks count themselves with one all-reduce (must be --gpus) and compare the devices they
    sit on -- N ranks on fewer than N devices is not an N-GPU measurement (exit 2) unless CV_SHARE_DEVICES says the run is
    the functional rehearsal on one GPU.  What was found travels in the line (rank_info: counted_ranks, distinct_devices)."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        _RANK_CHECK.update(counted_ranks=1, distinct_devices=1)
        return
    on_gpu = torch.cuda.is_available() and not args.dry
    dev = "cuda:%d" % local if dist.get_backend() == "nccl" else "cpu"
    t = torch.ones(1, dtype=torch.int64, device=dev)
    dist.all_reduce(t)
    counted = int(t.item())
    ident = "%s/%s" % (os.uname().nodename, (getattr(torch.cuda.get_device_properties(local), "uuid", None) or local) if on_gpu else "cpu%d" % rank)
    idents = [None] * ws
    dist.all_gather_object(idents, ident)
    distinct = len(set(idents))
    _RANK_CHECK.update(counted_ranks=counted, distinct_devices=distinct)
    bad = counted != args.gpus or (on_gpu and distinct != ws and not os.environ.get("CV_SHARE_DEVICES"))
    if bad:
        if rank == 0:
            print("bench.py: --gpus %d: %d rank(s) answered the all-reduce on %d distinct device(s) %s; refusing to time it"
                  % (args.gpus, counted, distinct, sorted(set(idents))), file=sys.stderr)
        finish_ranks()
        sys.exit(2)


def rank_info(ws):
    """what actually ran: number of ranks of the process group and its backend ("nccl" = RCCL on ROCm)"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        info = {"rccl_ranks": dist.get_world_size(), "backend": dist.get_backend()}
        info.update(_RANK_CHECK)
        if os.environ.get("CV_SHARE_DEVICES"):
            info["shared_devices"] = True         # a functional rehearsal: the ranks share GPUs, no number of this line is an N-GPU number
        if dist.get_backend() == "nccl":
            info["rccl_log"] = rccl_summary()
        return info
    return {"rccl_ranks": ws, "backend": None}


def finish_ranks():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def dry_main(args):
    """--dry: no GPU work; the ranks rendezvous, count themselves with one all-reduce and rank 0 prints the line
    skeleton.  Shows (also on a CPU box with CV_DIST_BACKEND=gloo) that `--gpus N` alone starts N ranks."""
    import torch
    import torch.distributed as dist
    rank, ws, local = init_ranks(args)
    n = 1
    if dist.is_available() and dist.is_initialized():
        dev = "cuda:%d" % local if dist.get_backend() == "nccl" else "cpu"
        t = torch.ones(1, dtype=torch.int64, device=dev)
        dist.all_reduce(t)
        n = int(t.item())
    if rank == 0:
        line = {"dry": True, "mode": args.mode, "n_gpus": ws, "counted_ranks": n}
        line.update(rank_info(ws))
        emit(line)
    finish_ranks()


def pileup_main(args):
    """--mode pileup: a step = one device pass of the BAM front end over alignments already in HBM:
    candidate counters (evc_count) + selection + tensor scatter + finalize; value = alignment columns/s.
    Workload per rank: 2 000 000 reads x 150 bp (30x over a 10 Mbp contig, 1 % substitutions); ranks hold
    different contigs (weak scaling, no collective).  Parsing the SAM text on the host is reported
    beside it (`host_inclusive`), never as `value`."""
    import torch
    import torch.distributed as dist
    from clairvoyante_amd import parallel, synth_pileup
    from clairvoyante_amd.pileup import Pileup
    rank, ws, local = init_ranks(args)
    torch.cuda.set_device(local)
    n_reads, L, read_len = 2000000, 10000000, 150
    thr, mincov = 0.06, 4
    ref, text = synth_pileup.fast_alignments(n_reads, L, read_len, seed=3 + rank)
    pl = Pileup(evc=True, retain=True, contig="ctgA")
    pl.set_reference(ref, 0)
    t0 = time.perf_counter()
    for s in range(0, len(text), 64 << 20):
        pl.add_sam(text[s:s + (64 << 20)])          # 64 MiB pieces, like a pipe reader would hand them over
    pl.extract_candidates(thr, mincov)
    centers = pl.adopt_candidates()
    tens, depth, touched = pl.finish(subtract=True)
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    base = pl.stats()
    check = (int(len(centers)), float(tens.sum().item()), int(depth.sum().item()))
    steps = args.steps

    def one_pass():
        _lib_check(pl.lib.cv_pileup_recount(pl.h, pl._stream()))
        pl.extract_candidates(thr, mincov)
        pl.adopt_candidates()
        return pl.finish(subtract=True)

    from clairvoyante_amd._lib import check as _lib_check
    for _ in range(args.warmup):
        one_pass()
    torch.cuda.synchronize()
    use_dist = dist.is_available() and dist.is_initialized()
    if use_dist:
        dist.barrier()
    s0 = pl.stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        tens, depth, touched = one_pass()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    s1 = pl.stats()
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    same = check == (int(pl.n), float(tens.sum().item()), int(depth.sum().item()))
    columns = n_reads * read_len
    if rank == 0:
        ms = {k: (s1[k] - s0[k]) / steps for k in ("candidate_ms", "scatter_ms", "finalize_ms")}
        # Algorithmic HBM bytes per pass: every kernel reads the segments once (1 SEQ byte + 20/64 segment bytes per
        # column); the candidate pass also writes the 36-byte counter row of every position, the scatter the
        # 1 188-byte counter block of every candidate.  `roofline` is the slower of the two.
        stream_bytes = columns * (1 + 20.0 / 64)
        kernels = {"evc_count + select (candidate pass)": (ms["candidate_ms"], stream_bytes + L * 36.0),
                   "pileup_scatter (tensor pass)": (ms["scatter_ms"], stream_bytes + columns / 64.0 + pl.n * 1188.0)}
        kname = max(kernels, key=lambda k: kernels[k][0])
        kern_ms, alg_bytes = kernels[kname]
        traffic = None
        try:        # HBM bytes per pass from the committed PMC passes (same workload), see profiles/pmc_traffic.json
            pm = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_traffic.json")))["pileup"]
            traffic = pm["evc_count" if kname.startswith("evc") else "pileup_scatter"]["hbm_bytes_per_pass"]
        except Exception:
            pass
        roof = {"bound": "hbm", "kernel": kname, "achieved": alg_bytes / (kern_ms * 1e-3) / 1e9,
                "peak": 8000.0, "unit": "GB/s", "frac": alg_bytes / (kern_ms * 1e-3) / 1e9 / 8000.0, "traffic": traffic,
                "algorithmic_bytes": alg_bytes, "avg_pass_ms": kern_ms, "note": "latency-bound candidate lookups per column (bucket table -> candidate list), "
                "counters privatised in LDS; far from the HBM roof by construction: %.0f G columns/s" % (
                    columns / (kern_ms * 1e-3) / 1e9),
                "candidate_ms": ms["candidate_ms"], "scatter_ms": ms["scatter_ms"], "finalize_ms": ms["finalize_ms"],
                "finalize_GBps": pl.n * (33 * 9 * 4 + 33 * 64) / (ms["finalize_ms"] * 1e-3) / 1e9}
        cpu = None
        if args.full and not args.no_cpu and ws == 1:          # the CPU leg runs at N = 1 only
            from oracle import create_tensor as oct_, extract_candidates as oec
            lines = text[:100000 * (len(text) // n_reads)].decode().splitlines()        # first 100 000 reads
            span = int(lines[-1].split("\t")[3]) + read_len
            refs = ref[:span + 64].decode()
            tc = time.perf_counter()
            rows = oec.candidates("ctgA", refs, lines, minCoverage=mincov, threshold=thr)
            cands = [int(r.split()[1]) for r in rows]
            oct_.pileup(refs, None, lines, cands)
            cs = time.perf_counter() - tc
            cpu = {"value": len(lines) * read_len / cs, "unit": "alignment columns/s", "cores": 1, "kind": "port",
                   "sample": "first %d reads of the timed set through oracle/extract_candidates.py + oracle/create_tensor.py "
                             "(CPython restatement of the reference scripts), %.1f s" % (len(lines), cs)}
        emit({"rccl_ranks": rank_info(ws)["rccl_ranks"], "backend": rank_info(ws)["backend"],
                          "metric": "alignment columns/sec (candidates + tensors)", "value": ws * steps * columns / dt,
                          "unit": "columns/s", "n_gpus": ws, "steps": steps, "warmup": args.warmup,
                          "ms_per_step": dt / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                          "dtype": "i32", "data": "synthetic",
                          "config": {"workload": "pileup front end: %d reads x %d bp over a %d bp contig per GPU, candidate "
                                                 "threshold %.2f, min coverage %d; %d candidates" % (n_reads, read_len, L, thr,
                                                                                                       mincov, pl.n)},
                          "roofline": roof, "cpu_baseline": cpu,
                          "host_inclusive": {"seconds": host_s, "sam_MB_per_s": len(text) / host_s / 1e6,
                                             "columns_per_s": columns / host_s},
                          "parity": {"repeat_passes_identical": bool(same)}})
    pl.close()
    finish_ranks()


def run_train(arch, gb, steps, warmup, rank, ws, dev, sync_loss=False, options=None):
    """`steps` optimizer steps (forward, backward, gradient exchange over the ranks, Adam) on a GLOBAL batch of `gb`
    synthetic labelled tensors split over the ranks; barrier + synchronize on both sides, MAX over ranks.
    -> dict(value, ms_per_step, roofline, final_loss, ...)."""
    import torch
    import torch.distributed as dist
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim, parallel, synth
    m = clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()
    m._seed_rng.seed(1234)
    m.init()
    parallel.broadcast_parameters(m)
    lo, hi = parallel.shard_range(gb, rank, ws)
    xt, cls, rf, alt, il = synth.make_candidates(gb, seed=synth.BASE_SEED, device=dev, return_class=True)
    y = synth.make_labels(cls, rf, alt, il)[lo:hi].contiguous(); x = xt[lo:hi].contiguous()
    use_dist = dist.is_initialized()
    exchange_plan = parallel.plan_exchange(m, gb) if use_dist else None      # what train.run_epoch does
    for k, v in (options or {}).items():
        if v is not None:
            m.setOption(k, v)
    step = m.train if sync_loss else m.trainDeferred     # deferred: no host round trip per step (train.run_epoch's way)
    for _ in range(warmup):
        step(x, y)
    m.readLosses()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        r = step(x, y)
    loss = r[0] if sync_loss else m.readLosses()[0][5] / steps       # one read for the whole run, inside the timed region
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    exchange = exchange_timing(m, step, x, y, steps, dt / steps * 1e3, dev) if use_dist else None
    m.close()
    # whole step against the matrix-core roof: forward + data gradients + weight gradients = 3 x the forward
    # FLOPs per candidate; the step is a chain of ~40 kernels, no single one dominates
    tf = steps * gb / dt / ws * 3 * FLOP_EXACT[arch] / 1e12
    traffic, note = train_traffic(arch, hi - lo)
    roof = {"bound": "mfma", "kernel": "whole step (forward, data gradients, weight gradients, Adam)",
            "achieved": tf, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": tf / PEAK_FP32_MFMA_TFLOPS,
            "traffic": traffic, "traffic_source": note}
    res = {"value": steps * gb / dt, "unit": "candidates/s", "ms_per_step": dt / steps * 1e3, "steps": steps,
           "global_batch": gb, "per_rank_batch": hi - lo, "roofline": roof, "final_loss": float(loss)}
    if exchange:
        res.update(exchange)
        res["exchange_plan"] = exchange_plan
    return res


def exchange_timing(m, step, x, y, steps, step_ms, dev):
    """What the gradient exchange costs and how much of it the backward pass hides, measured AFTER the timed region on
    the same model (N > 1 only):
      exchange_ms          the in-place bucket all-reduce(s) of one step alone (parallel.exchange_bucket as planned for
                           this batch: one collective, or the dense 95 % on the communication stream + the rest in
                           stream order), 20 iterations, no compute;
      compute_ms_per_step  the same optimizer steps with the exchange suspended (every rank applies its own shard's
                           gradient -- measurement only, the replicas diverge, the model is closed afterwards);
      exchange_hidden_frac 1 - (ms_per_step - compute_ms_per_step) / exchange_ms, clipped to [0, 1].
    Each is barrier + synchronize bracketed and the MAX over ranks."""
    import torch
    import torch.distributed as dist
    from clairvoyante_amd import parallel

    def timed(fn, k):
        torch.cuda.synchronize(); dist.barrier()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize(); dist.barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) / k * 1e3

    comm = parallel.comm_stream(m)
    m._bucket.zero_()                      # sums of zeros: the bucket cannot overflow over the iterations
    timed(lambda: parallel.exchange_bucket(m, comm), 3)
    ex_ms = timed(lambda: parallel.exchange_bucket(m, comm), 20)
    with parallel.exchange_suspended():
        timed(lambda: step(x, y), 2)
        comp_ms = timed(lambda: step(x, y), steps)
    m.readLosses()
    hidden = 1.0 - (step_ms - comp_ms) / ex_ms if ex_ms > 0 else None
    nbytes = int(m._bucket.numel()) * 4
    ws = dist.get_world_size()
    algbw = nbytes / (ex_ms * 1e-3) / 1e9 if ex_ms > 0 else None
    res = {"exchange_ms": ex_ms, "compute_ms_per_step": comp_ms,
           "exchange_hidden_frac": None if hidden is None else max(0.0, min(1.0, hidden)),
           "exchange_bytes": nbytes,
           # the step's own exchange as a bandwidth: bytes of the bucket / exchange_ms, and the bus bandwidth a ring moves
           # for it (x 2 (N - 1) / N: what --mode exchange prints per piece; one xGMI link is ~153 GB/s)
           "exchange_algbw_GBps": algbw,
           "exchange_busbw_GBps": None if algbw is None else algbw * 2.0 * (ws - 1) / max(ws, 1)}
    # the same steps under the OTHER plan (one collective behind the step <-> the dense part under the backward pass), so
    # that the first run on real links says which one the batch wants; the model's plan is restored afterwards
    if not os.environ.get("CV_EXCHANGE"):
        mine = parallel.exchange_mode(m)
        other = "one" if mine == "split" else "split"
        try:
            m._exchange_mode = other
            timed(lambda: step(x, y), 2)
            res["other_plan"] = {"plan": other, "ms_per_step": timed(lambda: step(x, y), steps)}
        finally:
            m._exchange_mode = mine
        m.readLosses()
    return res


def train_parity(arch, gb, dev):
    """The benchmarked training batch against the CPU oracle (checker only, outside every timed region; N = 1): one
    optimizer step of a fresh model on the batch the timed leg runs (same generator seed, same initial weights, default
    options, dropout 0.5), the keep mask the device drew handed to oracle/cv_oracle.c -- the five loss parts and all 18
    gradients.  The full set of sizes lives in tests/test_gpu_train_parity.py."""
    import numpy as np
    import torch
    from oracle import cv_oracle as O
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim, synth, _lib
    t0 = time.perf_counter()
    m = clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()
    m._seed_rng.seed(1234)
    m.init()
    P = m.getParameters()
    xt, cls, rf, alt, il = synth.make_candidates(gb, seed=synth.BASE_SEED, device=dev, return_class=True)
    y = synth.make_labels(cls, rf, alt, il)
    lam, rate = m.l2RegularizationLambdaVal, m.dropoutRateFC4Val
    loss, summ = m.train(xt, y)
    keep = (m.getActivation(6, gb) != 0).to(torch.float32).cpu().numpy()
    g = torch.empty(m.numParameters, device=dev)
    _lib.check(m._lib.cv_flat_copy(m._h, 1, ctypes.c_void_p(g.data_ptr()), 0, None))
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    m.close()
    l_or, parts, g_or = O.loss_grad(arch, P, xt.cpu().numpy(), y.cpu().numpy(), lam=lam, mask4=keep, rate4=rate)
    rel = [abs(summ[k] - ref) / max(1.0, abs(ref)) for k, ref in zip(("loss1", "loss2", "loss3", "loss4", "lossL2"), parts)]
    worst, off = 0.0, 0
    for name in O.PARAM_NAMES:
        gref = g_or[name] - (lam * P[name] if "bias" not in name else 0)
        sz = gref.size
        worst = max(worst, float(np.abs(g[off:off + sz].reshape(gref.shape) - gref).max() / (np.abs(gref).max() + 1e-30)))
        off += sz
    return {"n": gb, "arch": arch, "dropout": rate, "lambda": lam, "loss": float(loss), "loss_oracle": l_or,
            "loss_rel_err": abs(float(loss) - l_or) / abs(l_or), "loss_parts_max_rel_err": max(rel),
            "grad_max_err_rel_to_max": worst, "keep_fraction": float(keep.mean()),
            "checker": "oracle/cv_oracle.c cvo_loss_grad under the device's keep mask", "seconds": time.perf_counter() - t0}


def train_traffic(arch, per_rank):
    """HBM bytes of one optimizer step from the committed rocprofv3 --pmc passes (profiles/pmc_traffic.json, section
    "train"), keyed by arch and per-rank batch; None when no pass was taken at this size."""
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get("train", {})
        ent = tj.get("%s_%d" % (arch, per_rank))
        if ent:
            return ent["hbm_bytes_per_step"], "rocprofv3 --pmc passes at git %s" % tj.get("_git_head")
    except Exception as e:
        return None, "profiles/pmc_traffic.json unreadable: %s" % e
    return None, "profiles/pmc_traffic.json has no train entry for %s at %d candidates per rank" % (arch, per_rank)


def exchange_main(args):
    """--mode exchange: ONLY the gradient exchange of the data-parallel step -- in-place all-reduce(SUM) of the bucket
    (loss header + 1 631 496 gradients = 6.5 MB) and of its pieces, no compute: what xGMI / RCCL deliver at these sizes.
    A step = one all-reduce of the whole bucket; value = its bus bandwidth (algorithm bandwidth x 2 (N - 1) / N, the
    figure rccl-tests quotes), per size also the time and algorithm bandwidth; `rccl_log` carries the algorithm /
    protocol RCCL chose per size (NCCL_DEBUG_SUBSYS TUNING is switched on in this mode: reading those choices is its
    purpose).  Runs on any backend (gloo: functional test) and with one rank under CV_FORCE_DIST=1."""
    import torch
    import torch.distributed as dist
    from clairvoyante_amd import clairvoyante_v3
    os.environ.setdefault("CV_RCCL_TUNING_LOG", "1")
    rank, ws, local = init_ranks(args)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    m = clairvoyante_v3.Clairvoyante(); m.init()
    bucket = m._ensure_bucket()
    d = m._bucket_dense
    m.close()
    nfl = int(bucket.numel())
    use_dist = dist.is_available() and dist.is_initialized()
    staged = use_dist and dist.get_backend() == "gloo"
    steps = args.steps
    pieces = [("whole bucket (the tiny-share plan: one collective per step)", 0, nfl),
              ("dense part: fc4 / fc5 / heads gradients (under the convolution backward pass)", d, nfl),
              ("convolution gradients + loss header (behind the step)", 0, d),
              ("a fifth of the bucket", 0, nfl // 5)]
    buf = torch.zeros(nfl, dtype=torch.float32, device=dev)
    rows = []
    for label, lo, hi in pieces:
        t = buf[lo:hi]

        def one():
            if not use_dist:
                return
            if staged:
                h = t.cpu(); dist.all_reduce(h); t.copy_(h)
            else:
                dist.all_reduce(t)
        for _ in range(max(args.warmup, 3)):
            one()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        dt = time.perf_counter() - t0
        if use_dist:
            tt = torch.tensor([dt], dtype=torch.float64, device="cpu" if staged else dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        nbytes = (hi - lo) * 4
        alg = nbytes / (dt / steps) / 1e9
        rows.append({"piece": label, "bytes": nbytes, "ms": dt / steps * 1e3, "algbw_GBps": alg,
                     "busbw_GBps": alg * 2.0 * (ws - 1) / ws})
    if rank == 0:
        line = {"metric": "gradient bucket all-reduce bus bandwidth", "value": rows[0]["busbw_GBps"], "unit": "GB/s",
                "n_gpus": ws, "steps": steps, "warmup": max(args.warmup, 3), "ms_per_step": rows[0]["ms"],
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {"workload": "in-place all-reduce(SUM) of the training step's gradient bucket, %d bytes, no compute" % (nfl * 4),
                           "parallelism": "dp%d" % ws},
                "pieces": rows,
                "xgmi_ring_ceiling_note": "a ring over point-to-point xGMI is bound by one link (~153 GB/s per direction): "
                                          "busbw of a large message approaches that figure; at 6.5 MB latency dominates"}
        line.update(rank_info(ws))
        emit(line)
    finish_ranks()


def train_main(args):
    """--mode train: a step = one optimizer step (forward, backward, all-reduce, Adam) on a global batch of
    param.trainBatchSize = 10 000 synthetic labelled tensors (strong scaling: the batch is split)."""
    import torch
    import torch.distributed as dist
    from clairvoyante_amd import parallel, param
    rank, ws, local = init_ranks(args)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    gb = param.trainBatchSize if args.batch == BATCH else args.batch      # --batch: another global batch (default: the reference's)
    steps = args.steps
    r = run_train(args.arch, gb, steps, args.warmup, rank, ws, dev, sync_loss=args.sync_loss,
                  options=dict({"train_overlap": args.overlap, "train_tiny_groups": args.tiny, "train_ksplit": args.ksplit,
                                "train_side_streams": args.sides, "train_sched": args.sched},
                               **{"dbg" + kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.dbg.split(",") if kv},
                               **{kv.split("=")[0]: int(kv.split("=")[1]) for kv in args.opt.split(",") if kv}))
    if rank == 0:
        line = {"metric": "training candidate tensors/sec", "value": r["value"], "unit": "candidates/s",
                "n_gpus": ws, "steps": steps, "warmup": args.warmup, "ms_per_step": r["ms_per_step"],
                "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32",
                "data": "synthetic",
                "config": {"workload": "v3 %s training, Adam step on a global batch of %d synthetic labelled "
                                       "[33,4,4] tensors, dropout 0.5, lambda 1e-3" % (args.arch, gb),
                           "arch": args.arch, "global_batch": gb, "parallelism": "dp%d" % ws,
                           "losses": "read every step" if args.sync_loss else "accumulated on the device, read once",
                           "weight_gradients": "side stream" if (args.overlap is None or args.overlap) else "stream order",
                           "dbg": args.dbg + (" sides=%d" % args.sides if args.sides is not None else "") +
                                  (" ksplit=%d" % args.ksplit if args.ksplit is not None else "")},
                "roofline": r["roofline"], "final_loss": r["final_loss"]}
        for k in ("exchange_ms", "compute_ms_per_step", "exchange_hidden_frac", "exchange_bytes", "exchange_algbw_GBps", "exchange_busbw_GBps",
                  "exchange_plan", "other_plan"):
            if k in r:
                line[k] = r[k]
        line.update(rank_info(ws))
        emit(line)
    finish_ranks()


def run_infer(arch, batch, steps, warmup, rank, ws, dev, variant=None, batches=None):
    """`steps` passes of the inference hot path over batches resident in HBM; barrier + synchronize on both sides,
    MAX over ranks.  -> (result dict, model, parameters, batches, output of the last step); the caller closes the model."""
    import torch
    import torch.distributed as dist
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim, synth, _lib
    m = clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()
    P = synth.bench_params(arch)          # identical seeded weights on every rank (nothing from oracle/ in the timed function)
    m.setParameters(P)
    if variant is not None:
        m.setOption("variant", variant)
    # synthetic pileup tensors, generated straight into HBM (seed = 20260927 + rank)
    nbuf = max(1, min(steps, 64))
    if batches is None:
        batches = [synth.make_candidates(batch, seed=synth.BASE_SEED + rank + 1000 * b, device=dev) for b in range(nbuf)]
    nbuf = len(batches)
    out = torch.empty((batch, 16), dtype=torch.float32, device=dev)
    use_dist = dist.is_initialized()

    def barrier():
        if use_dist:
            dist.barrier()

    for i in range(warmup):
        m.predict_device(batches[i % nbuf], out)
    torch.cuda.synchronize()
    m.setOption("profile", 1)
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        m.predict_device(batches[i % nbuf], out)
    torch.cuda.synchronize(); barrier()
    dt = time.perf_counter() - t0
    m.setOption("profile", 0)
    ms = (ctypes.c_double * 6)(); cnt = (ctypes.c_int64 * 6)()
    _lib.check(m._lib.cv_kernel_times(m._h, ms, cnt))
    per_rank = None
    if use_dist:
        # every rank's own time for its steps (min / max over ranks: a straggler is visible), then the MAX is the job's time
        mine = torch.zeros(ws, dtype=torch.float64, device=dev)
        mine[rank] = dt
        dist.all_reduce(mine, op=dist.ReduceOp.SUM)
        allms = [float(v) / steps * 1e3 for v in mine.cpu()]
        per_rank = {"min": min(allms), "max": max(allms), "argmax_rank": int(max(range(ws), key=lambda r: allms[r]))}
        dt = max(float(v) for v in mine.cpu())

    value = steps * batch * ws / dt
    chunk = ctypes.c_int64(); _lib.check(m._lib.cv_get_option(m._h, b"chunk", ctypes.byref(chunk)))
    per_launch = min(batch, chunk.value)
    stages = []
    for s in range(6):
        if cnt[s] == 0:
            continue
        avg_ms = ms[s] / cnt[s]
        flop = STAGE_FLOP[arch][s] + (STAGE_FLOP[arch][0] if (s == 1 and cnt[0] == 0) else 0)
        if s == 2 and cnt[3] == 0:          # conv3 and fc4 as one kernel (slim, variant bit 8)
            flop += STAGE_FLOP[arch][3]
            if cnt[4] == 0 and cnt[5] == 0:             # ... with fc5 and the heads on its tail (variant bit 10)
                flop += STAGE_FLOP[arch][4] + STAGE_FLOP[arch][5]
        if s == 4 and cnt[5] == 0:          # the heads ride on the fc5 kernel (variant bit 9)
            flop += STAGE_FLOP[arch][5]
        if s == 3 and cnt[4] == 0 and cnt[5] == 0:      # fc5 and the heads ride on the fc4 kernel (variant bit 10)
            flop += STAGE_FLOP[arch][4] + STAGE_FLOP[arch][5]
        tf = flop * per_launch / (avg_ms * 1e-3) / 1e12
        kn = ctypes.c_char_p()
        _lib.check(m._lib.cv_kernel_name(m._h, s, ctypes.byref(kn)))
        label = STAGE_NAMES[s] + (" + fc4 (fused)" if (s == 2 and cnt[3] == 0) else "") + \
            (" + fc5 + heads" if (s == 2 and cnt[3] == 0 and cnt[4] == 0 and cnt[5] == 0) else "") + \
            (" + heads (fused)" if (s == 4 and cnt[5] == 0) else "") + \
            (" + fc5 + heads (fused)" if (s == 3 and cnt[4] == 0 and cnt[5] == 0 and arch == "full") else "")
        stages.append({"kernel": label, "kernel_name": kn.value.decode() if kn.value else None,
                       "avg_ms": avg_ms, "launches": int(cnt[s]), "tflops": tf,
                       "share": ms[s] / max(sum(ms), 1e-12)})
    dom = max(stages, key=lambda r: r["avg_ms"]) if stages else None
    # HBM bytes per launch from the separate rocprofv3 --pmc passes (tools/pmc_traffic.py -> profiles/): a counter
    # run cannot share a process with the timed run, so the file is matched against the kernels THIS binary ran --
    # an entry counts only if its template instance is the one the stage launched and the launch size is the same
    traffic, traffic_path, traffic_note = None, None, "profiles/pmc_traffic.json has no entry for the kernels of this run"
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get(arch, {})

        def entry(st):
            ent = tj.get(st["kernel"])
            ok = ent and ent.get("kernel_name") == st["kernel_name"] and ent.get("candidates_per_launch") == per_launch
            return ent if ok else None
        if dom and entry(dom):
            traffic = entry(dom)["hbm_bytes_per_launch"]
            traffic_note = "rocprofv3 --pmc passes at git %s, kernel %s" % (tj.get("_git_head"), dom["kernel_name"])
        if stages and all(entry(st) for st in stages):
            tot = sum(entry(st)["hbm_bytes_per_launch"] for st in stages)
            traffic_path = {"hbm_bytes_per_launch": tot, "compulsory_bytes_per_launch": 2176 * per_launch,
                            "ratio_to_compulsory": tot / (2176.0 * per_launch),
                            "per_kernel": {st["kernel"]: entry(st)["hbm_bytes_per_launch"] for st in stages}}
    except Exception as e:
        traffic_note = "profiles/pmc_traffic.json unreadable: %s" % e
    roof = None
    if dom:
        roof = {"bound": "mfma", "kernel": dom["kernel"], "achieved": dom["tflops"], "peak": PEAK_FP32_MFMA_TFLOPS,
                "unit": "TFLOP/s", "frac": dom["tflops"] / PEAK_FP32_MFMA_TFLOPS, "traffic": traffic,
                "traffic_source": traffic_note, "traffic_whole_path": traffic_path,
                "avg_launch_ms": dom["avg_ms"], "candidates_per_launch": per_launch,
                "whole_path_tflops": value / ws * FLOP_EXACT[arch] / 1e12,
                "whole_path_frac": value / ws * FLOP_EXACT[arch] / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                "hbm_frac_compulsory": value / ws * 2176 / 1e9 / PEAK_HBM_GBS}
    res = {"value": value, "unit": "candidates/s", "ms_per_step": dt / steps * 1e3, "steps": steps,
           "roofline": roof, "kernels": stages, "per_rank_ms": per_rank}
    return res, m, P, batches, out


DUMP_BYTES = 64 << 20


def dump_outputs(dirname, out16):
    """--dump-outputs DIR: what the timed path returned in its last step, predict_device's [batch, 16] float32
    probabilities (base 0..3, zygosity 4..5, variant type 6..9, indel length 10..15), as DIR/out16.npy -- rank 0's own
    shard.  The inputs are seeded, so two builds given the same arguments can be compared file for file.  An output
    larger than DUMP_BYTES is written as a fixed, seeded sample of its rows, their indices beside it as
    DIR/out16_rows.npy (float64)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    a = out16.cpu().numpy()
    rows_fn = os.path.join(dirname, "out16_rows.npy")
    budget = DUMP_BYTES - 4096                   # (room for the two .npy headers)
    if a.nbytes > budget:
        k = budget // (a.shape[1] * a.itemsize + 8)
        rows = np.sort(np.random.default_rng(0).choice(a.shape[0], size=k, replace=False))
        np.save(rows_fn, rows.astype(np.float64))
        a = a[rows]
    elif os.path.exists(rows_fn):
        os.remove(rows_fn)                       # (left by an earlier, larger run)
    np.save(os.path.join(dirname, "out16.npy"), np.ascontiguousarray(a, dtype=np.float32))


def host_legs(dev, rows=1000000, train_items=600000):
    """The reference's own API and loops at the CURRENT tree, outside every timed region of the headline (rank 0, N = 1):
    SURVEY 8 a11 (`predict` on caller-owned numpy batches, v3.py:257-267: 65 536 candidates and the reference's
    predictBatchSize of 1 000), a14 + a16 + a17 (`callVar.Run` over a text-tensor file of `rows` synthetic rows written to
    /dev/shm: GetTensor -> predict -> Output -> VCF, callVar.py:180-216), a15 + a18 (`train.TrainAll` over a synthetic
    .bin of `train_items` candidates, blosc blocks -> DecompressArray -> training step, train.py:63-160; the second epoch).
    Each leg names its workload; a leg that fails reports its error instead of taking the line down."""
    import logging
    import pickle
    import shutil
    import tempfile
    import types
    import numpy as np
    import torch
    from clairvoyante_amd import callVar, clairvoyante_v3, param, synth, train, utils_v2
    from clairvoyante_amd.pileup import format_rows
    out = {}
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="cv_bench_host_", dir=base)
    try:
        m = clairvoyante_v3.Clairvoyante(); m.setParameters(synth.bench_params("full"))
        # ---- predict(numpy)
        pn = {}
        for n in (65536, 1000):
            x = synth.make_candidates(n, seed=synth.BASE_SEED + 7, device=dev).cpu().numpy()
            for _ in range(3):
                m.predict(x)
            reps = 10 if n > 4096 else 200
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(reps):
                    m.predict(x)
                best = min(best, (time.perf_counter() - t0) / reps)
            pn[str(n)] = {"candidates_per_s": n / best, "ms_per_call": best * 1e3}
        out["predict_numpy"] = dict(pn, workload="model.predict(x) on a caller-owned pageable numpy batch [n,33,4,4] -> four numpy arrays "
                                                 "(host-to-device copy, pass, copy back inside the call)")
        chk = os.path.join(tmp, "model-000001"); m.saveParameters(chk); m.close()
        # ---- callVar over a text-tensor file
        try:
            nsrc = min(rows, 200000)
            x = synth.make_candidates(nsrc, seed=synth.BASE_SEED + 9, device=dev).cpu().numpy()
            x[..., 1:] += x[..., 0:1]; x = np.maximum(x, 0)          # back to raw counts: the reader subtracts matrix 0 again
            txt = os.path.join(tmp, "t.txt")
            refseq = b"N" * 83 + b"ACGT" * ((rows + 200) // 4 + 8)
            with open(txt, "wb") as fh:
                for s0 in range(0, rows, nsrc):
                    k = min(nsrc, rows - s0)
                    fh.write(b"\n".join(format_rows("chr1", np.arange(100 + s0, 100 + s0 + k), refseq, 0, x[:k])) + b"\n")
            a = types.SimpleNamespace(tensor_fn=txt, chkpnt_fn=chk, call_fn=os.path.join(tmp, "out.vcf"), qual=None, sampleName="S",
                                      ref_fn=None, threads=None, showRef=False, v3=True, v2=False, slim=False)
            best = 1e9
            for _ in range(2):                                    # (the second pass finds the file in the page cache)
                t0 = time.perf_counter(); callVar.Run(a); best = min(best, time.perf_counter() - t0)
            nrec = sum(1 for l in open(a.call_fn) if not l.startswith("#"))
            out["callvar_text"] = {"rows_per_s": rows / best, "seconds": best, "rows": rows, "vcf_records": nrec,
                                   "file_MB": os.path.getsize(txt) / 1e6,
                                   "workload": "callVar.Run on an uncompressed text-tensor file in %s (model load + GetTensor + "
                                               "predict + Output + VCF), %d rows" % (base or "the temp dir", rows)}
            os.unlink(txt)
        except BaseException as e:
            out["callvar_text"] = {"error": "%s: %s" % (type(e).__name__, e)}
        # ---- train.TrainAll over a .bin
        try:
            xt, cls, rf, alt, il = synth.make_candidates(train_items, seed=synth.BASE_SEED + 11, device=dev, return_class=True)
            X = xt.cpu().numpy(); Y = synth.make_labels(cls, rf, alt, il).cpu().numpy().astype(np.float64)
            XC = [utils_v2.pack_array(X[s0:s0 + 500]) for s0 in range(0, train_items + 1, 500)]
            YC = [utils_v2.pack_array(Y[s0:s0 + 500]) for s0 in range(0, train_items + 1, 500)]
            fn = os.path.join(tmp, "t.bin")
            with open(fn, "wb") as fh:
                pickle.dump(train_items, fh); pickle.dump(XC, fh); pickle.dump(YC, fh); pickle.dump([], fh)
            del X, Y, XC, YC
            times = []

            class H(logging.Handler):
                def emit(self, rec):
                    msg = rec.getMessage()
                    if msg.startswith("Epoch time elapsed"):
                        times.append(float(msg.split(":")[1].split()[0]))
            h = H(); lg = logging.getLogger(); lvl = lg.level
            lg.addHandler(h); lg.setLevel(logging.INFO)
            old_epochs = param.maxEpoch
            param.maxEpoch = 4                                    # three epochs
            try:
                m2 = clairvoyante_v3.Clairvoyante(); m2.init()
                a = types.SimpleNamespace(bin_fn=fn, tensor_fn=None, var_fn=None, bed_fn=None, chkpnt_fn=None, learning_rate=1e-3,
                                          lambd=1e-3, ochk_prefix=None, olog_dir=None, v2=False, v3=True, slim=False)
                train.TrainAll(a, m2, utils_v2)
                m2.close()
            finally:
                param.maxEpoch = old_epochs; lg.removeHandler(h); lg.setLevel(lvl)
            ep = min(times[1:]) if len(times) > 1 else times[0]
            out["trainall"] = {"candidates_per_s": train_items / ep, "epoch_seconds": ep, "epochs_timed": len(times), "items": train_items,
                               "workload": "train.TrainAll on a synthetic .bin (blosc blocks of 500, 90 %% trained in batches of %d, "
                                           "10 %% validated), best epoch after the first (the log prints hundredths of a second)"
                                           % param.trainBatchSize}
        except BaseException as e:
            out["trainall"] = {"error": "%s: %s" % (type(e).__name__, e)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def float64_outputs(arch, P, xs, dev=None, chunk=16384):
    """The independent float64 torch formulation (tests/torch_ref.py; no oracle/ in the loop) over xs, with stock torch
    ops on `dev` (the GPU: 262 144 candidates take a second or two) or, when the device refuses a float64 op, on the
    host over the first 16 384.  -> float64 [m, 16], m <= len(xs)"""
    import numpy as np
    import torch
    import torch_ref
    with torch.no_grad():
        if dev is not None:
            try:
                return np.concatenate([torch_ref.forward(arch, P, xs[i:i + chunk], dtype=torch.float64, device=dev)["out"].cpu().numpy()
                                       for i in range(0, len(xs), chunk)])
            except Exception as e:
                print("bench.py: float64 formulation on %s failed (%s: %s); host, first 16 384 candidates" % (dev, type(e).__name__, e), file=sys.stderr)
        return torch_ref.forward(arch, P, xs[:16384], dtype=torch.float64)["out"].numpy()


def margin_mask(want64, eps=1e-5):
    """-> bool [m, 4]: per head, the float64 margin between the two best classes is below eps -- where two correct fp32
    implementations (each within ~5e-6 of float64 on every probability) may legitimately order the classes differently."""
    import numpy as np
    import common
    close = []
    for lo, hi in common.HEADS:
        srt = np.sort(want64[:, lo:hi], axis=1)
        close.append((srt[:, -1] - srt[:, -2]) < eps)
    return np.stack(close, 1)


def order_sensitivity(got, want64, other=None):
    """Summation-order sensitivity of the argmax, from the float64 formulation: `got` = HIP outputs [m, 16], `other` =
    another fp32 implementation's outputs on the first len(other) of the same candidates.
      margin_below_1e-5_frac          share of the candidates with a float64 top-2 margin < 1e-5 on ANY head = the upper
                                      bound on argmax disagreement between the HIP path and any correct fp32 implementation
                                      (TF-CPU included);
      ..._per_head                    the same per head (base, zygosity, type, length);
      argmax_match_vs_float64_where_margin_ge_1e-5   HIP vs float64 outside that set, per head (must be 1.0);
      other_argmax_match_where_margin_ge_1e-5        HIP vs `other` outside that set, per head (must be 1.0);
      other_argmax_mismatches_in_margin_set          candidates x heads inside the set where the two fp32 orders differ."""
    import numpy as np
    import common
    m = want64.shape[0]
    close = margin_mask(want64)
    res = {"n": int(m), "margin_below_1e-5_frac": float(close.any(1).mean()),
           "margin_below_1e-5_frac_per_head": [float(v) for v in close.mean(0)],
           "max_abs_dprob_vs_float64": float(np.abs(got[:m].astype(np.float64) - want64).max())}
    agree = []
    for h, (lo, hi) in enumerate(common.HEADS):
        ok = ~close[:, h]
        agree.append(float(np.mean(np.argmax(got[:m, lo:hi], 1)[ok] == np.argmax(want64[:, lo:hi], 1)[ok])) if ok.any() else 1.0)
    res["argmax_match_vs_float64_where_margin_ge_1e-5"] = agree
    if other is not None:
        k = min(m, other.shape[0])
        out_ok, inside = [], 0
        for h, (lo, hi) in enumerate(common.HEADS):
            same = np.argmax(got[:k, lo:hi], 1) == np.argmax(other[:k, lo:hi], 1)
            ok = ~close[:k, h]
            out_ok.append(float(same[ok].mean()) if ok.any() else 1.0)
            inside += int((~same[~ok]).sum())
        res["other_n"] = int(k)
        res["other_argmax_match_where_margin_ge_1e-5"] = out_ok
        res["other_argmax_mismatches_in_margin_set"] = inside
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default: infer 64, train 20, pileup 20, exchange 50)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--arch", default="full", choices=["full", "slim"])
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run what else the line can carry: infer mode: the slim / training legs, "
                         "the training parity check, the host legs, the CPU baselines and the parity block; pileup mode: the "
                         "CPU leg")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the cpu_baseline leg")
    ap.add_argument("--no-extras", action="store_true", help="--full, infer mode: skip the slim / training legs (configs 4, 5)")
    ap.add_argument("--no-host", action="store_true", help="--full, infer mode: skip the host legs (predict(numpy), callVar over a text file, TrainAll over a .bin)")
    ap.add_argument("--dry", action="store_true", help="start the ranks, count them, print the skeleton; no GPU work")
    ap.add_argument("--sync-loss", action="store_true", help="train mode: read the losses back after every step (m.train)")
    ap.add_argument("--variant", type=int, default=None, help="infer mode: option variant (kernel selection, A/B)")
    ap.add_argument("--overlap", type=int, default=None, help="train mode: option train_overlap (A/B)")
    ap.add_argument("--tiny", type=int, default=None, help="train mode: option train_tiny_groups (A/B)")
    ap.add_argument("--ksplit", type=int, default=None, help="train mode: option train_ksplit (A/B)")
    ap.add_argument("--sides", type=int, default=None, help="train mode: option train_side_streams (A/B)")
    ap.add_argument("--dbg", default="", help="train mode: development switches, e.g. 0=3,2=1 sets options dbg0=3, dbg2=1")
    ap.add_argument("--opt", default="", help="train mode: any library option, e.g. dense_rag=13,infer_flat=0 (A/B)")
    ap.add_argument("--sched", type=int, default=None, help="train mode: option train_sched (bits of the re-cut step schedule, A/B)")
    ap.add_argument("--mode", default="infer", choices=["infer", "train", "pileup", "exchange"],
                    help="infer (default, the headline metric) or train: Adam steps on the reference's global "
                         "batch of 10 000 split over the ranks, one RCCL gradient all-reduce per step "
                         "(BASELINE.json configs[3]); pileup: candidate extraction + tensor generation over "
                         "alignments resident in HBM (SURVEY.md 8f N4); exchange: only the all-reduce of the step's "
                         "gradient bucket and of its pieces (time, algorithm / bus bandwidth, RCCL's algorithm choice)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="infer mode: after the timed steps, write what the last step computed to DIR (dump_outputs)")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = {"infer": 64, "train": 20, "pileup": 20, "exchange": 50}[args.mode]
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.mode != "infer" or args.dry):
        ap.error("--dump-outputs writes the outputs of the inference path: --mode infer, without --dry")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args, sys.argv[1:])          # does not return
    protect_stdout()          # from here on only emit() reaches the real stdout
    import atexit
    atexit.register(release_stdout)
    if args.dry:
        return dry_main(args)
    if args.mode == "train":
        return train_main(args)
    if args.mode == "pileup":
        return pileup_main(args)
    if args.mode == "exchange":
        return exchange_main(args)

    import numpy as np
    import torch
    import common
    from clairvoyante_amd import param

    rank, ws, local = init_ranks(args)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    res, m, P, batches, out = run_infer(args.arch, args.batch, args.steps, args.warmup, rank, ws, dev, variant=args.variant)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    line = {"metric": "candidate tensors/sec", "value": res["value"], "unit": "candidates/s", "n_gpus": ws,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": res["ms_per_step"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "v3 %s inference, synthetic [33,4,4] pileup tensors resident in HBM, "
                                   "batch %d x %d steps per GPU" % (args.arch, args.batch, args.steps),
                       "arch": args.arch, "batch": args.batch, "parallelism": "shard%d" % ws},
            "roofline": res["roofline"], "kernels": res["kernels"]}
    if res.get("per_rank_ms"):
        line["per_rank_ms"] = res["per_rank_ms"]          # ms per step of the fastest / slowest rank (N > 1)
    line.update(rank_info(ws))

    # Configs 5 and 4 under the same clock, OUTSIDE the headline's timed region: slim inference at the same batch, and
    # optimizer steps on train.py's global batch of 10 000 split over the ranks (one gradient all-reduce per step) --
    # at N = 1 also at 1 250, one rank's share of that batch on 8 GPUs; at N > 1 also at 10 000 PER rank.
    if args.full and not args.no_extras and args.arch == "full" and args.variant is None:
        t_extra = time.perf_counter()
        sres, sm, _sp, _sb, _so = run_infer("slim", args.batch, 32, 4, rank, ws, dev, batches=batches[:16])
        sm.close()
        line["slim"] = {"value": sres["value"], "unit": "candidates/s", "ms_per_step": sres["ms_per_step"], "steps": 32,
                        "kernels": [{"kernel_name": k["kernel_name"], "avg_ms": k["avg_ms"]} for k in sres["kernels"]],
                        "workload": "v3 slim inference, batch %d per GPU (BASELINE.json configs[4])" % args.batch,
                        "roofline": {k: sres["roofline"][k] for k in ("kernel", "frac", "achieved", "peak", "unit",
                                                                      "whole_path_frac", "traffic")}}
        gb = param.trainBatchSize
        tr = {}
        sizes = [(str(gb), gb)] + ([("1250", gb // 8)] if ws == 1 else [("%d_per_rank" % gb, gb * ws)])
        # (50 steps behind 5 warm-up steps, as `--mode train` in the validation script: with 20 behind 3 the 10 000 leg read
        # 2.084 ms where its own line on the same box reads 2.046 -- a 40 ms timed region still carries first-use costs)
        for key, g in sizes:
            tr[key] = run_train("full", g, 50, 5, rank, ws, dev)
        tr["slim_%d" % gb] = run_train("slim", gb, 50, 5, rank, ws, dev)
        line["train"] = tr
        line["extras_seconds"] = time.perf_counter() - t_extra
        if rank == 0 and ws == 1 and not args.no_cpu:
            try:
                tr["parity"] = train_parity("full", gb, dev)
            except Exception as e:      # the checker must not take the line down
                tr["parity"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if rank == 0 and ws == 1 and not args.no_host:
            t_host = time.perf_counter()
            try:
                line["host"] = host_legs(dev)
            except BaseException as e:
                line["host"] = {"error": "%s: %s" % (type(e).__name__, e)}
            line["host"]["seconds"] = time.perf_counter() - t_host

    if rank == 0:
        if args.full and not args.no_cpu and ws == 1:          # the CPU leg (and the parity block it feeds) runs at N = 1 only
            xs = torch.cat([b_ for b_ in batches[:4]])[:262144].cpu().numpy()
            cb, ref, n = cpu_baseline(args.arch, P, xs)
            got = m.predict_device(torch.from_numpy(xs[:n]).to(dev)).cpu().numpy()
            line["cpu_baseline"] = cb
            got_t = None
            try:
                line["cpu_baseline_torch"], got_t = cpu_torch_line(args.arch, P, xs, ref, hip_out=got)
            except Exception as e:      # informational only
                line["cpu_baseline_torch"] = {"error": str(e)}
            line["parity"] = {"n": n, "argmax_match_per_head": common.argmax_match(got, ref),
                              "max_abs_dprob": float(np.abs(got - ref).max()),
                              "bitwise_equal_frac": common.bitwise_frac(got, ref)}
            # Summation-order sensitivity (north_star: "100 % per-head argmax agreement vs TF-CPU"; TF cannot run here):
            # the float64 formulation over ALL timed candidates of the sample bounds the set on which any two correct
            # fp32 implementations may differ; outside it the HIP path must agree with float64 and with the oneDNN leg.
            try:
                w64 = float64_outputs(args.arch, P, xs[:n], dev)
                sens = order_sensitivity(got, w64, got_t)
                line["parity"]["max_abs_dprob_vs_float64"] = sens.pop("max_abs_dprob_vs_float64")
                line["parity"]["float64_n"] = sens.pop("n")
                line["parity"]["margin_below_1e-5_frac"] = sens["margin_below_1e-5_frac"]
                line["parity"]["margin_below_1e-5_frac_per_head"] = sens["margin_below_1e-5_frac_per_head"]
                line["parity"]["argmax_match_vs_float64_where_margin_gt_1e-5"] = sens["argmax_match_vs_float64_where_margin_ge_1e-5"]
                if "other_n" in sens and "error" not in line["cpu_baseline_torch"]:
                    line["cpu_baseline_torch"]["argmax_match_where_float64_margin_ge_1e-5"] = sens["other_argmax_match_where_margin_ge_1e-5"]
                    line["cpu_baseline_torch"]["argmax_mismatches_in_margin_set"] = sens["other_argmax_mismatches_in_margin_set"]
                from clairvoyante_amd import synth
                xst = (synth.make_stress(8192, seed=synth.BASE_SEED).numpy() * np.float32(0.25)).astype(np.float32)
                gst = m.predict_device(torch.from_numpy(xst).to(dev)).cpu().numpy()
                with torch.no_grad():
                    import torch_ref
                    tst = torch_ref.forward(args.arch, P, xst, dtype=torch.float32)["out"].numpy()
                st = order_sensitivity(gst, float64_outputs(args.arch, P, xst, dev), tst)
                line["parity"]["stress"] = {"n": st["n"], "margin_below_1e-5_frac": st["margin_below_1e-5_frac"],
                                            "max_abs_dprob_vs_float64": st["max_abs_dprob_vs_float64"],
                                            "argmax_match_vs_float64_where_margin_gt_1e-5": st["argmax_match_vs_float64_where_margin_ge_1e-5"],
                                            "torch_fp32_argmax_match_where_margin_ge_1e-5": st["other_argmax_match_where_margin_ge_1e-5"],
                                            "torch_fp32_argmax_mismatches_in_margin_set": st["other_argmax_mismatches_in_margin_set"]}
            except Exception as e:
                line["parity"]["max_abs_dprob_vs_float64"] = None
                line["parity"]["float64_error"] = "%s: %s" % (type(e).__name__, e)
        emit(line)
    m.close()
    finish_ranks()


if __name__ == "__main__":
    main()
