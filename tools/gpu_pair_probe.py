"""Development probe: PairWithNonVariants, the host loop against CV_PAIR=device over the same synthetic files.
    python tools/gpu_pair_probe.py [rungs=16384,65536,262144,1000000] [forms=plain,gz,bgzf] [sinks=gzip,bgzf,bgzf_device] [runs=5]
                                   [bed=100000] [parent=DIR]
Per rung (that many candidate rows and a third as many variant rows, tensor-shaped rows of about 2.3 KB over 22 contigs,
sorted; a BED of `bed` intervals), per form of the two input files (plain, ordinary .gz, BGZF) and per sink (the `gzip -c`
child, --bgzf, --bgzf with CV_BGZF_DEFLATE=device): seconds of every run of Pair_host and of the device route (run 0 of
each warms up and is not reported) as min..max, whether the device route was ahead in EVERY run, and the device calls split
by HIP events (line pass, join, draw, copy; the rest is the reader and the sink).  The inflated output and the returned
dict of the two routes are compared once per combination.
parent=DIR: a checkout of the parent commit (its clairvoyante_amd package importable from DIR, the library built): its
Pair_host runs the same combination in a child process, timed there.  Without it that column says so.
No floor follows from this probe: nothing makes the device route the default."""
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTIGS = ["chr%d" % c for c in range(1, 23)]
SPAN = 40000000
SEED, AMP = 7, 2


def write_bed(tmp, nbed):
    """nbed intervals over the contigs that cover about half of SPAN"""
    per = nbed // len(CONTIGS) + 1
    step = max(SPAN // per, 2)
    rows = ["%s\t%d\t%d" % (c, s, s + step // 2 + 1) for c in CONTIGS for s in range(0, per * step, step)][:nbed]
    fn = os.path.join(tmp, "conf_%d.bed" % nbed)
    with open(fn, "w") as fh:
        fh.write("\n".join(rows) + "\n")
    return fn


def write_rows(tmp, name, n, seed):
    """n tensor-shaped rows (contig, position, 33 bases, 528 values printed with %0.1f) sorted per contig -> {form: file}"""
    from clairvoyante_amd import utils_v2
    rng = np.random.RandomState(seed)
    per = n // len(CONTIGS) + 1
    pool = np.array(["0.0", "1.0", "12.0", "3.0", "104.0", "57.0", "-6.0", "-23.0"])
    out = {"plain": os.path.join(tmp, "%s_%d.txt" % (name, n)), "gz": os.path.join(tmp, "%s_%d.gz" % (name, n)),
           "bgzf": os.path.join(tmp, "%s_%d.bgzf.gz" % (name, n))}
    left = n
    with open(out["plain"], "wb") as plain, gzip.open(out["gz"], "wb", compresslevel=1) as gz, utils_v2.BgzfWriter(out["bgzf"], level=1) as bg:
        for ctg in CONTIGS:
            k = min(per, left)
            left -= k
            pos = np.sort(rng.randint(1, SPAN, k))
            for lo in range(0, k, 4096):
                part = pos[lo:lo + 4096]
                vals = pool[rng.randint(0, len(pool), (len(part), 528))]
                text = ("\n".join("%s %d ACGTACGTACGTACGTACGTACGTACGTACGTA %s" % (ctg, p, " ".join(v)) for p, v in zip(part.tolist(), vals)) + "\n").encode()
                for fh in (plain, gz, bg):
                    fh.write(text)
    return out


def args_of(var, can, bed, out, sink):
    import argparse
    return argparse.Namespace(tensor_var_fn=var, tensor_can_fn=can, bed_fn=bed, output_fn=out, amp=AMP, seed=SEED, bgzf=sink != "gzip")


def inflated_digest(fn):
    import hashlib
    import zlib
    h, n = hashlib.sha256(), 0
    with open(fn, "rb") as fh:
        d = zlib.decompressobj(31)
        while True:
            data = fh.read(1 << 24)
            if not data:
                break
            while data:                                      # member by member: an ordinary .gz has one, BGZF many
                piece = d.decompress(data)
                h.update(piece); n += len(piece)
                data = d.unused_data if d.eof else b""
                if d.eof:
                    d = zlib.decompressobj(31)
    return n, h.hexdigest()


def timed(route, var, can, bed, out, sink, runs):
    """-> (seconds per run, (dict, bytes and digest of the inflated output), ms of the device calls per run)"""
    import torch
    from clairvoyante_amd import PairWithNonVariants as pw, bed_items
    os.environ["CV_PAIR"] = route
    os.environ["CV_BGZF_DEFLATE"] = "device" if sink == "bgzf_device" else "host"
    secs, got, split = [], None, {}
    for r in range(runs + 1):
        pw.counts(reset=True)
        bed_items.TIMES = {} if route == "device" else None
        torch.cuda.synchronize(); t0 = time.perf_counter()
        d = pw.Pair(args_of(var, can, bed, out, sink))
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        c = pw.counts()
        assert (c["device_calls"], c["handed_over_calls"], c["host_calls"]) == ((1, 0, 0) if route == "device" else (0, 0, 1)), c
        if r:
            secs.append(dt)
            for k, v in (bed_items.TIMES or {}).items():
                split.setdefault(k, []).append(v)
        else:
            got = (d, inflated_digest(out))
    bed_items.TIMES = None
    return secs, got, split


PARENT_CHILD = """
import argparse, json, sys, time
sys.path.insert(0, sys.argv[1])
from clairvoyante_amd import PairWithNonVariants as pw
var, can, bed, out, bgzf, runs, seed, amp = sys.argv[2:10]
secs = []
for r in range(int(runs) + 1):
    a = argparse.Namespace(tensor_var_fn=var, tensor_can_fn=can, bed_fn=bed, output_fn=out, amp=float(amp), seed=int(seed), bgzf=bgzf == "1")
    t0 = time.perf_counter(); d = pw.Pair_host(a, int(seed)); dt = time.perf_counter() - t0
    if r:
        secs.append(dt)
print("RESULT " + json.dumps({"secs": secs, "o2": d["o2"]}))
"""


def timed_parent(parent, var, can, bed, out, sink, runs):
    """the parent commit's Pair_host in a child process -> seconds per run, or None"""
    if not parent:
        return None
    env = dict(os.environ, CV_BGZF_DEFLATE="host")
    env.pop("CV_PAIR", None)
    p = subprocess.run([sys.executable, "-c", PARENT_CHILD, parent, var, can, bed, out, "1" if sink != "gzip" else "0", str(runs), str(SEED), str(AMP)],
                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env)
    for line in p.stdout.decode().splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])["secs"]
    return None


def span(v):
    return "%.3f..%.3f" % (min(v), max(v)) if v else "-"


def main():
    opt = dict(a.split("=", 1) for a in sys.argv[1:])
    rungs = [int(v) for v in opt.get("rungs", "16384,65536,262144,1000000").split(",") if v]
    forms = [v for v in opt.get("forms", "plain,gz,bgzf").split(",") if v]
    sinks = [v for v in opt.get("sinks", "gzip,bgzf,bgzf_device").split(",") if v]
    runs, nbed, parent = int(opt.get("runs", 5)), int(opt.get("bed", 100000)), opt.get("parent")
    tmp = tempfile.mkdtemp(prefix="cv_pair_")
    bed = write_bed(tmp, nbed)
    out = os.path.join(tmp, "mix.gz")
    print("candidates form sink | host loop s, min..max of %d runs | device route s | parent's host loop s | verdict | device calls by HIP events, "
          "ms min..max" % runs, flush=True)
    for n in rungs:
        t0 = time.time()
        can, var = write_rows(tmp, "can", n, 3), write_rows(tmp, "var", n // 3, 4)
        print("# wrote %d candidate and %d variant rows in %.1f s (plain: %d + %d bytes); BED %d intervals"
              % (n, n // 3, time.time() - t0, os.path.getsize(can["plain"]), os.path.getsize(var["plain"]), nbed), flush=True)
        for form in forms:
            for sink in sinks:
                host, hgot, _s = timed("host", var[form], can[form], bed, out, sink, runs)
                dev, dgot, split = timed("device", var[form], can[form], bed, out, sink, runs)
                assert dgot == hgot, "the routes disagree: %r against %r" % (dgot, hgot)
                par = timed_parent(parent, var[form], can[form], bed, out, sink, runs)
                print("%8d %-5s %-11s | %s | %s | %s | %s | %s; o2 %d of c %d" % (
                    n, form, sink, span(host), span(dev), span(par) if par else "not run", "device ahead in every run" if max(dev) < min(host)
                    else "device NOT ahead in every run", "; ".join("%s %s" % (k, span(v)) for k, v in sorted(split.items())), hgot[0]["o2"], hgot[0]["c"]),
                    flush=True)
        for fn in list(can.values()) + list(var.values()):
            os.unlink(fn)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
