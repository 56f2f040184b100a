"""Development probe: utils_v2.BgzfWriter with its members compressed on the device (CV_BGZF_DEFLATE=device, opt-in)
against the host writer of the same tree at 16 threads, at zlib's level 6 (the default) and level 1.
    python tools/gpu_bgzf_deflate_probe.py [merge=65536,1000000,5000000] [rows=65536,262144,1000000] [runs=5] [threads=16]
MergeVcf: vcf_merge.merge under CV_VCF_MERGE=device over the plain chunk files of tools/gpu_vcf_merge_probe.py, end to end
into a .vcf.gz + .tbi.  CreateTensor --bgzf: its write loop (pileup.format_row_blocks under CV_ROW_FORMAT=device into the
writer) over synthetic tensors already in HBM.  Per rung the three writers alternate, run 0 of each warms up and is not
listed; seconds of every run, min..max, whether the device writer was ahead of BOTH host writers in EVERY run, the file
sizes, and the bytes that cross the link per run (host writers: the text comes down; device writer: what
bgzf_deflate_counts() counted up and down).  The inflated files are compared through their members' ISIZE and CRC-32.
Then the three kernels of cv_bgzf_deflate_dev by HIP events over one slab of 256 members of each text
(cv_bgzf_deflate_phase_dev), five times each, and the members per block type.
The host writer is the parent commit's code, unchanged by the switch; the parent itself is not run here."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

WRITERS = (("host6", "host", 6), ("host1", "host", 1), ("device", "device", 6))
say = lambda s: (sys.stdout.write(s + "\n"), sys.stdout.flush())


def span(v):
    return "%.3f..%.3f" % (min(v), max(v))


def members_of(fn):
    from clairvoyante_amd import utils_v2
    table, total = utils_v2.bgzf_scan(np.fromfile(fn, dtype=np.uint8))
    return table[:, 3].tolist(), total


def report(name, n, secs, sizes, crossed, text_bytes):
    ahead = max(secs["device"]) < min(min(secs["host6"]), min(secs["host1"]))
    say("%-12s %8d | text %d B | host6 %s s | host1 %s s | device %s s | %s | file B host6 %d host1 %d device %d (%.3f x level 1, %.3f x level 6)"
        " | crossing B host: %d down; device: %d up %d down"
        % (name, n, text_bytes, span(secs["host6"]), span(secs["host1"]), span(secs["device"]),
           "device ahead in every run" if ahead else "device NOT ahead in every run", sizes["host6"], sizes["host1"], sizes["device"],
           sizes["device"] / float(sizes["host1"]), sizes["device"] / float(sizes["host6"]), text_bytes, crossed["uploaded"], crossed["downloaded"]))
    for k in secs:
        say("    %-6s per run: %s" % (k, " ".join("%.3f" % s for s in secs[k])))


def leveled(base, level):
    class Writer(base):
        def __init__(self, fn, **kw):
            kw.setdefault("level", level)
            base.__init__(self, fn, **kw)
    return Writer


def merge_rung(tmp, n, runs, threads):
    import torch
    import gpu_vcf_merge_probe as mp
    import vcf_merge_cases as vc
    from clairvoyante_amd import utils_v2, vcf_merge
    plain, bgzf, fai = mp.make_inputs(tmp, n, utils_v2, vc)
    os.environ["CV_VCF_MERGE"] = "device"
    secs, sizes, crossed, outs = {k: [] for k, _r, _l in WRITERS}, {}, {}, {}
    plainwriter = utils_v2.BgzfWriter
    for r in range(runs + 1):
        for key, route, level in WRITERS:                    # the routes alternate
            os.environ["CV_BGZF_DEFLATE"] = route
            vcf_merge.utils_v2.BgzfWriter = leveled(plainwriter, level)
            outs[key] = os.path.join(tmp, "%s_%d.vcf.gz" % (key, n))
            utils_v2.bgzf_deflate_counts(reset=True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            got = vcf_merge.merge(plain, outs[key], fai_fn=fai, threads=threads)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            assert got["route"] == "device"
            if r:
                secs[key].append(dt)
            sizes[key], crossed[key] = os.path.getsize(outs[key]), utils_v2.bgzf_deflate_counts()
    vcf_merge.utils_v2.BgzfWriter = plainwriter
    want, text_bytes = members_of(outs["host6"])
    for key in ("host1", "device"):
        assert members_of(outs[key]) == (want, text_bytes), "the writers disagree on the inflated file"
    assert crossed["device"]["device"] > 0 and crossed["host6"]["device"] == 0        # (the device run's "host" members are the .tbi's)
    report("MergeVcf", got["records"], secs, sizes, crossed["device"], text_bytes)
    parts, have = [], 0                                       # a slab's worth of the inputs for the kernel timings
    for f in plain:
        parts.append(np.fromfile(f, dtype=np.uint8))
        have += len(parts[-1])
        if have >= 256 * 65280:
            break
    text = np.concatenate(parts)
    for f in plain + bgzf:
        os.remove(f)
    return text


def rows_rung(tmp, rows, runs, threads):
    import torch
    from clairvoyante_amd import pileup, utils_v2
    os.environ["CV_ROW_FORMAT"] = "device"
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev); g.manual_seed(rows)
    depth = torch.randint(8, 60, (rows, 33, 1), generator=g, device=dev).float()
    t = torch.zeros((rows, 33, 4, 4), dtype=torch.float32, device=dev)
    t[:, :, :, 0] = torch.where(torch.rand((rows, 33, 4), generator=g, device=dev) < 0.3, depth.expand(rows, 33, 4), torch.zeros((), device=dev))
    t[:, :, :, 1:] = torch.where(torch.rand((rows, 33, 4, 3), generator=g, device=dev) < 0.04,
                                 torch.randint(1, 9, (rows, 33, 4, 3), generator=g, device=dev).float(), torch.zeros((), device=dev))
    ref = torch.randint(0, 4, (2 * rows + 200,), generator=g, device=dev)
    ref = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[ref]
    centers = 100 + 2 * np.arange(rows, dtype=np.int64)
    secs, sizes, crossed, outs = {k: [] for k, _r, _l in WRITERS}, {}, {}, {}
    first = None
    for r in range(runs + 1):
        for key, route, level in WRITERS:
            outs[key] = os.path.join(tmp, "%s_%d.tensor.gz" % (key, rows))
            utils_v2.bgzf_deflate_counts(reset=True)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            w = utils_v2.BgzfWriter(outs[key], level=level, threads=threads, deflate=route)
            for block in pileup.format_row_blocks("chr20", centers, ref, 0, t, in_hbm=w.deflate == "device"):
                if first is None and hasattr(block, "is_cuda"):
                    first = block[:256 * 65280].clone()
                w.write_device(block) if hasattr(block, "is_cuda") else w.write(block)
            w.close()
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if r:
                secs[key].append(dt)
            sizes[key], crossed[key] = os.path.getsize(outs[key]), utils_v2.bgzf_deflate_counts()
    want, text_bytes = members_of(outs["host6"])
    for key in ("host1", "device"):
        assert members_of(outs[key]) == (want, text_bytes), "the writers disagree on the inflated file"
        os.remove(outs[key])
    os.remove(outs["host6"])
    assert crossed["device"]["host"] == 0 and crossed["device"]["uploaded"] == 0
    report("CreateTensor", rows, secs, sizes, crossed["device"], text_bytes)
    return first.cpu().numpy()


def kernels(name, text, runs):
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    block = 65280
    n = min(len(text), 256 * block)
    members = -(-n // block)
    src = torch.from_numpy(np.ascontiguousarray(text[:n])).to(dev)
    cap = members * (block + 31)
    out, sizes, info = (torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(members, dtype=torch.int32, device=dev),
                        torch.empty(8, dtype=torch.int64, device=dev))
    need = _lib.workspace(lib.cv_bgzf_deflate_workspace, members, block)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P, st = _lib.ptr, _lib.stream_arg(dev)
    args = (P(src), n, block, P(out), cap, P(sizes), P(info), P(ws), need, st)
    _lib.check(lib.cv_bgzf_deflate_dev(*args))
    torch.cuda.synchronize()
    i = info.cpu().numpy()
    ms = [[], [], []]
    for _ in range(runs):
        for phase in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _lib.check(lib.cv_bgzf_deflate_phase_dev(phase, *args))
            b.record()
            b.synchronize()
            ms[phase].append(a.elapsed_time(b))
    say("kernels %-12s %d members of %d B (%d B -> %d B; stored %d fixed %d dynamic %d) | bd_compress %s ms (%.2f GB/s of text at best) | "
        "bd_offsets %s ms | bd_assemble %s ms"
        % (name, members, block, n, i[0], i[2], i[3], i[4], span(ms[0]), n / min(ms[0]) / 1e6, span(ms[1]), span(ms[2])))


def main():
    opt = dict(a.split("=", 1) for a in sys.argv[1:])
    ints = lambda key, default: [int(v) for v in opt.get(key, default).split(",") if v]
    runs, threads = int(opt.get("runs", 5)), int(opt.get("threads", 16))
    tmp = tempfile.mkdtemp(prefix="cv_bgzfdeflate_")
    say("what rung | text | seconds per run min..max of the three writers | verdict | file sizes | bytes crossing per run")
    texts = {}
    for n in ints("merge", "65536,1000000,5000000"):
        texts["vcf"] = merge_rung(tmp, n, runs, threads)
    for rows in ints("rows", "65536,262144,1000000"):
        texts["tensor rows"] = rows_rung(tmp, rows, runs, threads)
    for name, text in texts.items():
        kernels(name, text, runs)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
