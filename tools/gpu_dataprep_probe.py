"""Development probe: the dataPrepScripts helpers (clairvoyante_amd/bed_items.py), host loop against device route over the
same synthetic files.
    python tools/gpu_dataprep_probe.py [rungs=16384,65536,262144,1000000] [ranges=1000000,46700000,250000000] [runs=5] [bed=100000]
choose / count: per rung (tensor-shaped item rows of about 2.3 KB over 22 contigs, sorted) and per form of the item file
(plain, ordinary .gz, BGZF), against a BED of `bed` intervals: seconds of every run of the host loop and of the device
route (run 0 of each warms up and is not reported), whether the device route was ahead in EVERY run, and the device calls
split by HIP events (line pass, keep kernels; the rest is the reader: upload, inflate, the copies back).  The bytes and
counts of the two routes are compared once per rung and form.
sampling: per range of positions, with and without that BED's intervals of one contig: the same for sample_positions.
The parent commit has no counterpart: the only baseline is the host loop of the same tree."""
import gzip
import io
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTIGS = ["chr%d" % c for c in range(1, 23)]
SPAN = 40000000                                              # positions per contig the items and the BED spread over


def write_bed(tmp, nbed):
    """nbed intervals over the contigs that cover about half of SPAN"""
    per = nbed // len(CONTIGS) + 1
    step = max(SPAN // per, 2)
    rows = ["%s\t%d\t%d" % (c, s, s + step // 2 + 1) for c in CONTIGS for s in range(0, per * step, step)][:nbed]
    fn = os.path.join(tmp, "conf_%d.bed" % nbed)
    with open(fn, "w") as fh:
        fh.write("\n".join(rows) + "\n")
    return fn


def write_items(tmp, n):
    """n tensor-shaped rows (contig, position, 33 bases, 528 values printed with %0.1f) sorted per contig -> {form: file}"""
    from clairvoyante_amd import utils_v2
    rng = np.random.RandomState(3)
    per = n // len(CONTIGS) + 1
    pool = np.array(["0.0", "1.0", "12.0", "3.0", "104.0", "57.0", "-6.0", "-23.0"])
    out = {"plain": os.path.join(tmp, "items_%d.txt" % n), "gz": os.path.join(tmp, "items_%d.gz" % n),
           "bgzf": os.path.join(tmp, "items_%d.bgzf.gz" % n)}
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


def timed_items(route, fn, bed, runs, count):
    import torch
    from clairvoyante_amd import bed_items
    os.environ["CV_BED_ITEMS"] = route
    out, got, split = [], None, {}
    for r in range(runs + 1):
        bed_items.counts(reset=True)
        bed_items.TIMES = {} if route == "device" else None
        sink = None if count else io.BytesIO()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        tally = bed_items.count_items(fn, bed) if count else bed_items.choose_items(fn, bed, sink)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        c = bed_items.counts()
        assert (c["device_calls"], c["handed_over_calls"], c["host_calls"]) == ((1, 0, 0) if route == "device" else (0, 0, 1)), c
        got = (tally, None if count else sink.getvalue())
        if r:
            out.append(dt)
            for k, v in (bed_items.TIMES or {}).items():
                split.setdefault(k, []).append(v)
    bed_items.TIMES = None
    return out, got, split


def timed_sample(route, start, end, intervals, runs):
    import torch
    from clairvoyante_amd import bed_items
    os.environ["CV_BED_ITEMS"] = route
    out, got, split = [], None, {}
    for r in range(runs + 1):
        bed_items.TIMES = {} if route == "device" else None
        torch.cuda.synchronize(); t0 = time.perf_counter()
        got = bed_items.sample_positions("chr1", start, end, 7000000 * 2. / 3000000000, intervals, 7)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        if r:
            out.append(dt)
            for k, v in (bed_items.TIMES or {}).items():
                split.setdefault(k, []).append(v)
    bed_items.TIMES = None
    return out, got, split


def fmt(v, form="%.3f"):
    return " ".join(form % x for x in v)


def verdict(host, dev):
    return "device ahead in every run" if max(dev) < min(host) else "device NOT ahead in every run"


def main():
    opt = dict(a.split("=", 1) for a in sys.argv[1:])
    rungs = [int(v) for v in opt.get("rungs", "16384,65536,262144,1000000").split(",") if v]
    ranges = [int(v) for v in opt.get("ranges", "1000000,46700000,250000000").split(",") if v]
    runs, nbed = int(opt.get("runs", 5)), int(opt.get("bed", 100000))
    from clairvoyante_amd.ExtractVariantCandidates import read_bed
    tmp = tempfile.mkdtemp(prefix="cv_dataprep_")
    bed = write_bed(tmp, nbed)
    print("rows form what | host loop s per run | device route s per run | verdict | device calls by HIP events, ms per run", flush=True)
    for n in rungs:
        t0 = time.time()
        forms = write_items(tmp, n)
        print("# wrote %d item rows in %.1f s: %s; BED %d intervals" % (n, time.time() - t0, ", ".join(
            "%s %d bytes" % (k, os.path.getsize(v)) for k, v in forms.items()), nbed), flush=True)
        for form, fn in forms.items():
            for count in (False, True):
                host, hgot, _s = timed_items("host", fn, bed, runs, count)
                dev, dgot, split = timed_items("device", fn, bed, runs, count)
                assert dgot == hgot, "the routes disagree"
                print("%8d %-5s %-6s | %s | %s | %s | %s" % (n, form, "count" if count else "choose", fmt(host), fmt(dev), verdict(host, dev),
                                                           "; ".join("%s %s" % (k, fmt(v, "%.2f")) for k, v in sorted(split.items()))), flush=True)
        for fn in forms.values():
            os.unlink(fn)
    intervals = read_bed(bed, "chr1")
    for span in ranges:
        for iv in (None, intervals):
            host, hgot, _s = timed_sample("host", 1, 1 + span, iv, runs)
            dev, dgot, split = timed_sample("device", 1, 1 + span, iv, runs)
            assert np.array_equal(hgot, dgot), "the routes disagree"
            print("%10d positions %-3s -> %d kept | %s | %s | %s | %s" % (span, "bed" if iv else "-", len(hgot), fmt(host), fmt(dev), verdict(host, dev),
                                                                        "; ".join("%s %s" % (k, fmt(v, "%.2f")) for k, v in sorted(split.items()))), flush=True)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
