"""Development probe: utils_v2.truth_tables, host route against device route over the same synthetic files.
    python tools/gpu_truth_tables_probe.py rungs=20000,200000,1000000,4000000 [runs=5] [parent=DIR] [e2e=ROWS]
Per rung (truth rows over 22 contigs, a BED of a tenth as many intervals) and per form of the truth list (plain, ordinary
.gz, BGZF; the same rows as a truth VCF in BGZF read for four sources; the BED as plain text), with and without the BED: seconds of every run of the host route and of the device
route (run 0 of each warms up and is not reported), and whether the device route was ahead in EVERY run.  The tables
of the two routes are compared once per rung.
parent=DIR: a checkout of the parent commit; `_trainset_tables(*_read_bed_truth(...))` is timed there in a child process
over the .gz form (that commit has no other reader).
e2e=ROWS: GetTrainingSetDevice end to end under both routes over a BGZF tensor file of ROWS rows (0 = skip).
At the end the kernels of the largest rung by HIP events: the line pass over the whole plain text as one slab, the two
table passes."""
import ctypes
import gzip
import os
import random
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTIGS = ["chr%d" % c for c in range(1, 23)]


def write_files(tmp, n):
    """n truth rows (sorted per contig, one key in 50 twice) -> {form: truth list}, BED (n // 10 intervals that keep ~90 %)"""
    from clairvoyante_amd import utils_v2
    rng = np.random.RandomState(3)
    per = n // len(CONTIGS) + 1
    alts = ("A C 0 1", "G T 1 1", "A ACG 0 1", "ATTT A 1 1", "C CTTTTTT 0 1", "T G 0 1")
    rows, bed, left = [], [], n
    for ctg in CONTIGS:
        k = min(per, left)
        left -= k
        pos = np.cumsum(rng.randint(1, 900, k)) + 10000
        pos[50::50] = pos[49::50][:len(pos[50::50])]                     # a key twice, the rows side by side
        kinds = rng.randint(0, len(alts), k)
        rows += ["%s %d %s" % (ctg, p, alts[a]) for p, a in zip(pos.tolist(), kinds.tolist())]
        span = int(pos[-1]) + 1000 if k else 20000
        step = max(span // max(k // 10, 1), 2)
        bed += ["%s\t%d\t%d" % (ctg, s, s + max(step * 9 // 10, 1)) for s in range(0, span, step)]
    text = ("\n".join(rows) + "\n").encode()
    out = {"plain": os.path.join(tmp, "truth_%d.txt" % n), "gz": os.path.join(tmp, "truth_%d.gz" % n), "bgzf": os.path.join(tmp, "truth_%d.bgzf.gz" % n)}
    with open(out["plain"], "wb") as fh:
        fh.write(text)
    with gzip.open(out["gz"], "wb", compresslevel=6) as fh:
        fh.write(text)
    with utils_v2.BgzfWriter(out["bgzf"], level=6) as fh:
        fh.write(text)
    # the same rows as a truth VCF (BGZF, what truth VCFs are): a header, genotypes in both spellings, one row in 40 a
    # 1|2 call on two ALT alleles
    vcf = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS"]
    for k, r in enumerate(rows):
        ctg, p, ref, alt, g1, g2 = r.split()
        if k % 40 == 7:
            alt, g1, g2 = alt + ",G" + alt, "1", "2"
        vcf.append("\t".join((ctg, p, ".", ref, alt, "50", "PASS", ".", "GT:DP", g1 + "/|"[k & 1] + g2 + ":30")))
    out["vcf"] = os.path.join(tmp, "truth_%d.vcf.gz" % n)
    with utils_v2.BgzfWriter(out["vcf"], level=6) as fh:
        fh.write(("\n".join(vcf) + "\n").encode())
    bed_fn = os.path.join(tmp, "conf_%d.bed" % n)
    with open(bed_fn, "w") as fh:
        fh.write("\n".join(bed) + "\n")
    return out, bed_fn, len(bed)


VCF_SOURCES = (("-", "-", "chr1", None, None), ("-", "-", "chr2", 10000, 2000000), ("-", "-", "chr2", 1000000, 900000000),
               ("-", "-", "chr7", None, None))


def timed(route, var, bed, runs, vcf=None):
    import torch
    from clairvoyante_amd import utils_v2
    os.environ["CV_TRUTH_TABLES"] = route
    out, got = [], None
    for r in range(runs + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        got = utils_v2.truth_tables(var, bed, want_every=True, vcf_fn=vcf, sources=VCF_SOURCES if vcf else None)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        assert got.route == route, (got.route, got.reason)
        if r:
            out.append(dt)
    return out, got


PARENT_CHILD = """
import sys, time
sys.path.insert(0, sys.argv[1])
from clairvoyante_amd import utils_v2
var, bed, runs = sys.argv[2], (sys.argv[3] or None), int(sys.argv[4])
for r in range(runs + 1):
    t0 = time.perf_counter()
    utils_v2._trainset_tables(*utils_v2._read_bed_truth(var, bed), bed is not None)
    if r:
        print("%.4f" % (time.perf_counter() - t0), flush=True)
"""


def same(a, b):
    ta, tb = a.cpu(), b.cpu()
    ok = a.names == b.names and all(ta[k].dtype == tb[k].dtype and np.array_equal(ta[k], tb[k]) for k in tb)
    return ok and sorted(a.every) == sorted(b.every) and all(np.array_equal(a.every[k], b.every[k]) for k in b.every)


def kernels(var_plain, bed_fn):
    """HIP-event times of cv_truth_lines_dev (one slab = the whole file), cv_bed_table_dev, cv_truth_tables_dev"""
    import torch
    from clairvoyante_amd import _lib, utils_v2
    lib = _lib.load()
    dev = torch.device("cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    E = lambda shape, dt=torch.int64: torch.empty(shape, dtype=dt, device=dev)
    need = ctypes.c_int64()

    def event_ms(fn, reps=5):
        ms = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms[1:]

    cols = {}
    for fmt, fn in ((utils_v2.TRUTH_FORMAT_BED, bed_fn), (utils_v2.TRUTH_FORMAT_VAR, var_plain)):
        raw = np.fromfile(fn, dtype=np.uint8)
        text = torch.from_numpy(raw).to(dev)
        n = int((raw == 10).sum()) + 1
        _lib.check(lib.cv_truth_lines_workspace(len(raw), n, ctypes.byref(need)))
        ws, wsn = E(need.value, torch.uint8), need.value
        bed = fmt == utils_v2.TRUTH_FORMAT_BED
        pos, end, label = E(n), E(n) if bed else None, None if bed else E((n, 16), torch.float32)
        run, tok, info = E(n, torch.int32), E((n, 2)), E(8)
        call = lambda: _lib.check(lib.cv_truth_lines_dev(P(text), len(raw), fmt, None, 0, 0, 0, 0, n, P(pos), P(end), P(label), P(run), P(tok), P(info), P(ws), wsn, st))
        ms = event_ms(call)
        i = info.cpu().tolist()
        print("kernels  cv_truth_lines_dev %s: %d bytes, %d lines, %d rows, %d runs: %s ms (%.1f GB/s)"
              % ("BED" if bed else "VAR", len(raw), i[1], i[2], i[5], " ".join("%.3f" % m for m in ms), len(raw) / np.median(ms) / 1e6), flush=True)
        cols[fmt] = (pos, end if bed else label, run, i[2], i[5])
    # (the files are sorted by contig: run k is contig k)
    pos, end, run, nb, runs = cols[utils_v2.TRUTH_FORMAT_BED]
    rc = torch.arange(max(runs, 1), dtype=torch.int32, device=dev)
    bed_off, bed_begin, bed_emax = E(runs + 1), E(nb), E(nb)
    _lib.check(lib.cv_bed_table_workspace(nb, ctypes.byref(need)))
    ws, wsn = E(need.value, torch.uint8), need.value
    ms = event_ms(lambda: _lib.check(lib.cv_bed_table_dev(nb, P(pos), P(end), P(run), P(rc), runs, runs, P(bed_off), P(bed_begin), P(bed_emax), P(ws), wsn, st)))
    print("kernels  cv_bed_table_dev: %d intervals: %s ms" % (nb, " ".join("%.3f" % m for m in ms)), flush=True)
    pos, label, run, n, nruns = cols[utils_v2.TRUTH_FORMAT_VAR]
    nctg = max(runs, nruns)
    truth_off, every_off, truth_pos, every_pos, labels, counts = E(nctg + 1), E(nctg + 1), E(n), E(n), E((n, 16), torch.float32), E(2)
    _lib.check(lib.cv_truth_tables_workspace(n, ctypes.byref(need)))
    ws, wsn = E(need.value, torch.uint8), need.value
    rc = torch.arange(max(nruns, 1), dtype=torch.int32, device=dev)
    ms = event_ms(lambda: _lib.check(lib.cv_truth_tables_dev(n, P(pos), P(label), P(run), P(rc), nruns, nctg, 1 if runs == nctg else 0, P(bed_off),
                                                               P(bed_begin), P(bed_emax), P(truth_off), P(truth_pos), P(labels), P(every_off),
                                                               P(every_pos), P(counts), P(ws), wsn, st)))
    print("kernels  cv_truth_tables_dev: %d rows -> %s (truth rows, distinct positions): %s ms"
          % (n, counts.cpu().tolist(), " ".join("%.3f" % m for m in ms)), flush=True)


def end_to_end(tmp, rows, var, bed, runs):
    """GetTrainingSetDevice over a BGZF tensor file of `rows` rows on the truth contigs, both routes"""
    import torch
    from clairvoyante_amd import synth, utils_v2
    from clairvoyante_amd.pileup import format_rows
    x = synth.make_candidates(rows, seed=9, device="cuda").cpu().numpy()
    x[..., 1:] += x[..., 0:1]
    x = np.maximum(x, 0)
    ref = b"N" * 83 + b"ACGT" * ((rows + 200) // 4 + 8)
    fn = os.path.join(tmp, "tensor_%d.bgzf.gz" % rows)
    with utils_v2.BgzfWriter(fn, level=1) as fh:
        fh.write(b"\n".join(format_rows("chr1", np.arange(10000, 10000 + rows), ref, 0, x)) + b"\n")
    for route in ("host", "device"):
        os.environ["CV_TRUTH_TABLES"] = route
        out = []
        for r in range(runs + 1):
            random.seed(1); torch.cuda.synchronize(); t0 = time.perf_counter()
            ts = utils_v2.GetTrainingSetDevice(fn, var, bed)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            assert ts.route == "device", ts.reason
            if r:
                out.append((dt, ts.times["tables"]))
        print("e2e      GetTrainingSetDevice %d tensor rows, tables %s: total s %s | tables s %s"
              % (rows, route, " ".join("%.3f" % a for a, _b in out), " ".join("%.3f" % b for _a, b in out)), flush=True)
    os.unlink(fn)


def main():
    opt = dict(a.split("=", 1) for a in sys.argv[1:])
    rungs = [int(v) for v in opt.get("rungs", "20000,200000,1000000,4000000").split(",")]
    runs, parent, e2e = int(opt.get("runs", 5)), opt.get("parent"), int(opt.get("e2e", 0))
    tmp = tempfile.mkdtemp(prefix="cv_truth_")
    print("rows form bed | host route s per run | device route s per run | verdict", flush=True)
    last = None
    for n in rungs:
        t0 = time.time()
        forms, bed_fn, nbed = write_files(tmp, n)
        print("# wrote %d truth rows, %d intervals in %.1f s: %s" % (n, nbed, time.time() - t0, ", ".join(
            "%s %d bytes" % (k, os.path.getsize(v)) for k, v in list(forms.items()) + [("bed", bed_fn)])), flush=True)
        for bed in (None, bed_fn):
            for form, var in forms.items():
                vcf = var if form == "vcf" else None         # (four sources on three contigs, two of them bounded and overlapping)
                host, hgot = timed("host", None if vcf else var, bed, runs, vcf)
                devt, dgot = timed("device", None if vcf else var, bed, runs, vcf)
                assert same(dgot, hgot), "the routes disagree"
                wins = max(devt) < min(host)
                print("%8d %-5s %-3s | %s | %s | %s" % (n, form, "bed" if bed else "-", " ".join("%.3f" % v for v in host),
                                                       " ".join("%.3f" % v for v in devt),
                                                       "device ahead in every run" if wins else "device NOT ahead in every run"), flush=True)
            if parent:
                got = subprocess.check_output([sys.executable, "-c", PARENT_CHILD, parent, forms["gz"], bed or "", str(runs)])
                print("%8d gz    %-3s | parent commit, host loop, s per run: %s" % (n, "bed" if bed else "-", " ".join(got.decode().split())), flush=True)
        if e2e and n == rungs[-1]:
            end_to_end(tmp, e2e, forms["gz"], bed_fn, runs)
        if last:
            for fn in list(last[0].values()) + [last[1]]:
                os.unlink(fn)
        last = (forms, bed_fn)
    kernels(last[0]["plain"], last[1])
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
