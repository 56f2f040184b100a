"""Development probe: the VCF merge, the host route against the opt-in device route of the same tree (the parent commit has
no merge to compare with).
    python tools/gpu_vcf_merge_probe.py [rungs=65536,1000000,5000000] [runs=5] [threads=16]
Per rung (records of callVar's shape spread over chr1 .. chr22, X, Y in chunk files of 10 Mbp, given in glob order, which
is not genome order) and per input form (plain text, BGZF): vcf_merge.merge under CV_VCF_MERGE=host and =device into a
.vcf.gz + .tbi -- seconds of every run (run 0 of each warms up and is not reported), whether the device route was ahead
in EVERY run, and the split of the last run: read (inputs to memory / to HBM), order + index (host: the per-line loop, the
sort, the tables; device: line pass, cv_vcf_merge_dev, cv_vcf_windows_dev and the tables crossing), BGZF write (host
threads on both routes; on the device route it includes the sorted text crossing in pinned slabs), .tbi write; and the
device calls by HIP events in milliseconds (lines = cv_item_lines_dev; order_gather_chunks = cv_vcf_merge_dev: fields,
sort, gather, chunk table; windows = cv_vcf_windows_dev).  The files of the two routes are compared once per line."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONTIGS = [("chr%s" % c, n) for c, n in zip(list(range(1, 23)) + ["X", "Y"],
                                             [248, 242, 198, 190, 181, 170, 159, 145, 138, 133, 135, 133, 114, 107, 101, 90, 83, 80, 58, 64,
                                              46, 50, 156, 57])]


def fmt(v, form="%.3f"):
    return " ".join(form % x for x in v)


def make_inputs(tmp, n, utils_v2, vc):
    """-> (plain files, BGZF files) in glob order, .fai"""
    rs = np.random.RandomState(n % 1000003)
    total = float(sum(m for _c, m in CONTIGS))
    fai = os.path.join(tmp, "ref_%d.fa.fai" % n)
    with open(fai, "w") as fh:
        for c, m in CONTIGS:
            fh.write("%s\t%d\t0\t60\t61\n" % (c, m * 1000000))
    header = vc.HEADER.split(b"##contig")[0] + b"".join(b"##contig=<ID=%s,length=%d>\n" % (c.encode(), m * 1000000) for c, m in CONTIGS) + \
        b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n"
    plain, bgzf = [], []
    for c, m in CONTIGS:
        k = int(round(n * m / total))
        pos = np.sort(rs.randint(1, m * 1000000, k))
        cut = np.searchsorted(pos, np.arange(0, m * 1000000 + 10000000, 10000000))
        for j in range(len(cut) - 1):
            ps = pos[cut[j]:cut[j + 1]].tolist()
            if not ps:
                continue
            body = b"".join(vc.rec(c, p, "ACGT"[p % 4] + "ACGTT"[:p % 11 == 0 and p % 5], "ACGT"[(p + 1) % 4], p % 100, ("PASS", "LowQual", ".")[p % 3],
                                   "LENGUESS=%d" % (p % 5) if p % 11 == 0 else ".", ("0/1", "1/1")[p % 2], 4 + p % 97, (1 + p % 99) / 100.0)
                            for p in ps)
            name = os.path.join(tmp, "p%d.%s_%d_%d.vcf" % (n, c, j * 10000000, (j + 1) * 10000000))
            with open(name, "wb") as fh:
                fh.write(header + body)
            with utils_v2.BgzfWriter(name + ".gz", level=1) as w:
                w.write(header + body)
            plain.append(name); bgzf.append(name + ".gz")
    return sorted(plain), sorted(bgzf), fai


def timed(route, files, fai, out, runs, threads):
    import torch
    from clairvoyante_amd import vcf_merge
    os.environ["CV_VCF_MERGE"] = route
    secs, split, got = [], {}, None
    for r in range(runs + 1):
        vcf_merge.TIMES = {}
        vcf_merge.counts(reset=True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        got = vcf_merge.merge(files, out, fai_fn=fai, threads=threads)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        c = vcf_merge.counts()
        assert (c["device_calls"], c["host_calls"], c["handed_over_calls"]) == ((1, 0, 0) if route == "device" else (0, 1, 0)), c
        if r:
            secs.append(dt)
        split = dict(vcf_merge.TIMES)
    vcf_merge.TIMES = None
    return secs, split, got["records"]


def main():
    opt = dict(a.split("=", 1) for a in sys.argv[1:])
    rungs = [int(v) for v in opt.get("rungs", "65536,1000000,5000000").split(",") if v]
    runs, threads = int(opt.get("runs", 5)), int(opt.get("threads", 16))
    import vcf_merge_cases as vc
    from clairvoyante_amd import utils_v2
    tmp = tempfile.mkdtemp(prefix="cv_vcfmerge_")
    say = lambda s: (sys.stdout.write(s + "\n"), sys.stdout.flush())
    say("records form files | host route s per run | device route s per run | verdict | last run's split, host then device")
    keys = ("read_s", "order_index_s", "bgzf_write_s", "tbi_write_s", "lines_ms", "order_gather_chunks_ms", "windows_ms")
    for n in rungs:
        plain, bgzf, fai = make_inputs(tmp, n, utils_v2, vc)
        for form, files in (("plain", plain), ("bgzf", bgzf)):
            outs = {r: os.path.join(tmp, "%s_%d.vcf.gz" % (r, n)) for r in ("host", "device")}
            host, hs, hn = timed("host", files, fai, outs["host"], runs, threads)
            dev, ds, dn = timed("device", files, fai, outs["device"], runs, threads)
            assert hn == dn, "the routes disagree on the records"
            for sfx in ("", ".tbi"):
                assert open(outs["host"] + sfx, "rb").read() == open(outs["device"] + sfx, "rb").read(), "the routes disagree"
            verdict = "device ahead in every run" if max(dev) < min(host) else "device NOT ahead in every run"
            show = lambda s: " ".join("%s %.3f" % (k, s[k]) for k in keys if k in s)
            say("%8d %-5s %4d | %s | %s | %s | host: %s | device: %s" % (hn, form, len(files), fmt(host), fmt(dev), verdict, show(hs), show(ds)))
        for f in plain + bgzf:
            os.remove(f)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
