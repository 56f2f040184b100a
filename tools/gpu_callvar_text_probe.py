"""Development probe: callVar.py end to end on text tensors (BASELINE.json configs[0] path at a larger size):
rows/s for a plain and a gzip-compressed tensor file, with the share of each stage.
    python tools/gpu_callvar_text_probe.py [rows] [parse=device|host]
parse=... forces one text reader (CV_TEXT_PARSE) for the whole run.  With a ladder,
    python tools/gpu_callvar_text_probe.py ladder=1000,16384,65536,200000,1000000 [runs=5] [gzmax=1000000] [forms=plain,gz,bgzf] [gzlevel=6]
one process alternates parse=host and parse=device at every size, plain, .gz (`gzip -6`: the device side finds its
block starts and inflates it, the gzip-device route; its column also counts the chunks it inflated and the hand-overs to
the host) and BGZF (the same text re-blocked by clairvoyante_amd.bgzf; the device side inflates it too): a warm-up run
of each, then `runs` timed runs of each in turn (wall time of callVar.Test behind a loaded model, ending in a device
synchronise), rows/s as median and range, and which side wins by more than the host side's own range.  kernels=ROWS
times the parse kernels of one slab, the inflate of the same slab as BGZF members and as one `gzip -6` stream (find,
counting pass, writing pass, resolve, CRC), beside the forward pass of the same rows."""
import cProfile
import gzip
import os
import pstats
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def _write_rows(path, n, x, ngz):
    from clairvoyante_amd.pileup import format_rows
    with open(path, "wb") as fh:
        for s in range(0, n, ngz):
            k = min(ngz, n - s)
            rows = format_rows("chr1", np.arange(100 + s, 100 + s + k), b"N" * 83 + b"ACGT" * ((n + 200) // 4 + 8), 0, x[:k])
            fh.write(b"\n".join(rows) + b"\n")


def ladder(sizes, runs, gzmax, want_forms=("plain", "gz", "bgzf"), gzlevel=6):
    import torch
    import common
    from oracle import cv_oracle as O
    from clairvoyante_amd import bgzf, callVar, clairvoyante_v3, synth, utils_v2
    tmp = tempfile.mkdtemp(prefix="cv_cvtext_")
    ngz = min(max(sizes), 200000)
    x = synth.make_candidates(ngz, seed=9, device="cuda").cpu().numpy()
    x[..., 1:] += x[..., 0:1]
    x = np.maximum(x, 0)
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.setParameters(common.bench_params(O, "full", seed=11))
    print("rows form bytes | host rows/s median (min..max) | device rows/s median (min..max) | verdict")
    for n in sizes:
        txt = os.path.join(tmp, "t%d.txt" % n)
        _write_rows(txt, n, x, ngz)
        forms = [("plain", txt)] if "plain" in want_forms else []
        if n <= gzmax and "gz" in want_forms:
            subprocess.check_call("gzip -%d -c %s > %s.gz" % (gzlevel, txt, txt), shell=True)
            forms.append(("gz", txt + ".gz"))
        if n <= gzmax and "bgzf" in want_forms:
            bgzf.reblock(txt, txt + ".bgzf.gz", level=1)
            forms.append(("bgzf", txt + ".bgzf.gz"))
        for form, fn in forms:
            a = types.SimpleNamespace(tensor_fn=fn, chkpnt_fn=None, call_fn=os.path.join(tmp, "out.vcf"), qual=None, sampleName="S",
                                      ref_fn=None, threads=None, showRef=False, v3=True, v2=False, slim=False)
            rate = {"host": [], "device": []}
            vcf = {}
            chunks = dict(utils_v2.gzip_chunk_counts)
            for r in range(runs + 1):                       # run 0 of each side warms up
                for side in ("host", "device"):
                    os.environ["CV_TEXT_PARSE"] = side
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    callVar.Test(a, m, utils_v2)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if r:
                        rate[side].append(n / dt)
                    else:
                        vcf[side] = open(a.call_fn, "rb").read()
            assert vcf["host"] == vcf["device"], "the two readers disagree"
            h, d = np.array(rate["host"]), np.array(rate["device"])
            wins = np.median(d) > np.median(h) + (h.max() - h.min())
            grew = {k: utils_v2.gzip_chunk_counts[k] - chunks[k] for k in chunks}
            print("%8d %-5s %11d | %.3g (%.3g..%.3g) | %.3g (%.3g..%.3g) | %s%s" % (
                n, form, os.path.getsize(fn), np.median(h), h.min(), h.max(), np.median(d), d.min(), d.max(),
                "device wins" if wins else "device does not win",
                " | gzip-device: %d chunks, %d hand-overs in %d runs" % (grew["device"], grew["host"], runs + 1) if form == "gz" else ""), flush=True)
            if form != "plain":
                os.unlink(fn)
        os.unlink(txt)
    os.environ.pop("CV_TEXT_PARSE", None)
    m.close()
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


def kernels(n):
    """HIP-event time of the parse kernels (and the gather) for one slab of n rows beside the forward pass of the rows"""
    import ctypes
    import torch
    import common
    from oracle import cv_oracle as O
    from clairvoyante_amd import _lib, clairvoyante_v3, synth
    lib = _lib.load()
    tmp = tempfile.mkdtemp(prefix="cv_cvtext_")
    x = synth.make_candidates(n, seed=9, device="cuda").cpu().numpy()
    x[..., 1:] += x[..., 0:1]
    x = np.maximum(x, 0)
    txt = os.path.join(tmp, "k.txt")
    _write_rows(txt, n, x, n)
    text = open(txt, "rb").read()
    os.unlink(txt); os.rmdir(tmp)
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.setParameters(common.bench_params(O, "full", seed=11))
    need = ctypes.c_int64()
    _lib.check(lib.cv_parse_tensor_text_dev_workspace(len(text), n, ctypes.byref(need)))
    buf = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    buf = torch.cat([buf, torch.zeros(64, dtype=torch.uint8, device="cuda")])
    xd = torch.empty((n, 528), device="cuda"); meta = torch.empty((n, 6), dtype=torch.int64, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda"); info = torch.empty(4, dtype=torch.int64, device="cuda")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    idx = torch.arange(0, n, 2, dtype=torch.int64, device="cuda"); out = torch.empty((len(idx), 528), device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def parse():
        _lib.check(lib.cv_parse_tensor_text_dev(ctypes.c_void_p(buf.data_ptr()), len(text), n, ctypes.c_void_p(xd.data_ptr()),
                                                ctypes.c_void_p(meta.data_ptr()), ctypes.c_void_p(status.data_ptr()),
                                                ctypes.c_void_p(info.data_ptr()), ctypes.c_void_p(ws.data_ptr()), need.value, st))

    def gather():
        _lib.check(lib.cv_text_gather_rows(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(idx.data_ptr()), len(idx),
                                           ctypes.c_void_p(out.data_ptr()), st))

    def forward():
        m.predict_device(xd.reshape(n, 33, 4, 4))

    # the same slab as BGZF members (65 280 input bytes each, zlib level 1 and 6), inflated into a second buffer
    from clairvoyante_amd import utils_v2
    inflates = []
    for level in (1, 6):
        blob = b"".join(utils_v2.BgzfWriter.member(text[at:at + 65280], level) for at in range(0, len(text), 65280))
        table, total = utils_v2.bgzf_scan(np.frombuffer(blob, dtype=np.uint8))
        assert total == len(text)
        table[:, 0] -= table[0, 0]
        comp = torch.frombuffer(bytearray(blob[18:]), dtype=torch.uint8).cuda()
        tab = torch.from_numpy(table).cuda()
        mstat = torch.zeros(len(table), dtype=torch.uint8, device="cuda")
        dst = torch.zeros(len(text) + 64, dtype=torch.uint8, device="cuda")

        def inflate(comp=comp, tab=tab, mstat=mstat, dst=dst):
            _lib.check(lib.cv_inflate_bgzf_dev(ctypes.c_void_p(comp.data_ptr()), ctypes.c_void_p(tab.data_ptr()), len(tab),
                                               ctypes.c_void_p(dst.data_ptr()), len(text), ctypes.c_void_p(mstat.data_ptr()), st))
        inflate(); torch.cuda.synchronize()
        assert int((mstat != 1).sum()) == 0 and torch.equal(dst[:len(text)], buf[:len(text)])
        inflates.append(("inflate + CRC, %d members, level %d, %.1f MB" % (len(table), level, len(blob) / 1e6), inflate))

    # the same slab as ONE gzip -6 stream: the kernels of the gzip-device route one by one, tables as the reader builds them
    import zlib
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(text) + c.flush()
    spacing = int(os.environ.get("CV_GZIP_GUESS_BYTES") or utils_v2.GZIP_GUESS_BYTES)
    gcomp = torch.frombuffer(bytearray(raw + b"\0" * 8), dtype=torch.uint8).cuda()
    guesses = -(-len(raw) // spacing)
    found = torch.empty(guesses, dtype=torch.int64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def find():
        _lib.check(lib.cv_gzip_find_dev(P(gcomp), len(raw), 0, spacing, guesses, P(found), st))
    find()
    f = found.cpu().numpy()
    starts = np.concatenate(([0], f[f >= 0]))
    rows = np.zeros((len(starts), 6), dtype=np.int64)
    rows[:, 0], rows[:, 1], rows[:, 4] = starts, np.append(starts[1:], -1), 32768
    rows[0, 4] = 0
    gtab = torch.from_numpy(rows).cuda()
    gres = torch.zeros((len(starts), 4), dtype=torch.int64, device="cuda")

    def count():
        _lib.check(lib.cv_gzip_decode_dev(P(gcomp), len(raw), P(gtab), len(starts), None, 0, P(gres), st))
    count()
    r = gres.cpu().numpy()
    assert np.all(r[:-1, 2] == 1) and r[-1, 2] == 2 and int(r[:, 0].sum()) == len(text)
    off = np.concatenate(([0], np.cumsum(r[:, 0])))
    rows[:, 2], rows[:, 3] = off[:-1], r[:, 0]
    gtab2, goff = torch.from_numpy(rows).cuda(), torch.from_numpy(off).cuda()
    gsym = torch.empty(len(text) + 8, dtype=torch.int16, device="cuda")
    gtext = torch.zeros(65536 + len(text) + 64, dtype=torch.uint8, device="cuda")
    gbad = torch.zeros(2 + (len(text) + 1023) // 1024, dtype=torch.int32, device="cuda")

    def write():
        _lib.check(lib.cv_gzip_decode_dev(P(gcomp), len(raw), P(gtab2), len(starts), P(gsym), len(text), P(gres), st))

    def resolve():
        _lib.check(lib.cv_gzip_resolve_dev(P(gsym), P(goff), len(starts), len(text), 0, ctypes.c_void_p(gtext.data_ptr() + 65536), P(gbad), st))

    def crc():
        _lib.check(lib.cv_gzip_crc_dev(ctypes.c_void_p(gtext.data_ptr() + 65536), len(text), ctypes.c_void_p(gbad.data_ptr() + 8), st))
    write(); resolve(); crc(); torch.cuda.synchronize()
    assert torch.equal(gtext[65536:65536 + len(text)], buf[:len(text)]) and int(gbad[0]) == 0
    assert (utils_v2._crc_shift(0xffffffff, len(text)) ^ utils_v2._crc_fold(gbad.cpu().numpy()[2:].view(np.uint32))) ^ 0xffffffff == zlib.crc32(text)
    tag = "gzip -6, %.1f MB, %d chunks at %d KiB guesses: " % (len(raw) / 1e6, len(starts), spacing >> 10)
    inflates += [(tag + "find", find), (tag + "counting pass", count), (tag + "writing pass", write), (tag + "resolve", resolve), (tag + "CRC", crc)]

    for name, fn in [("index + parse", parse), ("gather of every second row", gather), ("forward pass", forward)] + inflates:
        ms = []
        for r in range(8):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            if r >= 3:
                ms.append(e0.elapsed_time(e1))
        print("%d rows, %.1f MB of text: %-64s %.3f ms median (%.3f..%.3f)" % (n, len(text) / 1e6, name, np.median(ms), min(ms), max(ms)))
    assert tuple(info.cpu().numpy()) == (len(text), n, n, 0)
    m.close()


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    sys.argv = [a for a in sys.argv if "=" not in a]
    if "parse" in opts:
        os.environ["CV_TEXT_PARSE"] = opts["parse"]
    if "kernels" in opts:
        kernels(int(opts["kernels"]))
    if "ladder" in opts:
        ladder([int(v) for v in opts["ladder"].split(",")], int(opts.get("runs", 5)), int(opts.get("gzmax", 1000000)),
               tuple(opts.get("forms", "plain,gz,bgzf").split(",")), int(opts.get("gzlevel", 6)))
    if "kernels" in opts or "ladder" in opts:
        return
    import common
    from oracle import cv_oracle as O
    from clairvoyante_amd import callVar, clairvoyante_v3, synth
    from clairvoyante_amd.pileup import format_rows
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000         # plain text; the .gz leg takes the first ngz rows
    ngz = min(n, 200000)
    tmp = tempfile.mkdtemp(prefix="cv_cvtext_")
    x = synth.make_candidates(ngz, seed=9, device="cuda").cpu().numpy()
    x[..., 1:] += x[..., 0:1]                       # back to raw counts (the file holds them; the reader subtracts)
    x = np.maximum(x, 0)
    t0 = time.time()
    txt = os.path.join(tmp, "t.txt")
    small = os.path.join(tmp, "s.txt")
    with open(txt, "wb") as fh:                     # the same ngz tensors at advancing coordinates until n rows are written
        for s in range(0, n, ngz):
            k = min(ngz, n - s)
            rows = format_rows("chr1", np.arange(100 + s, 100 + s + k), b"N" * 83 + b"ACGT" * ((n + 200) // 4 + 8), 0, x[:k])
            blob = b"\n".join(rows) + b"\n"
            fh.write(blob)
            if s == 0:
                open(small, "wb").write(blob)
    print("wrote %d rows, %.0f MB in %.1f s" % (n, os.path.getsize(txt) / 1e6, time.time() - t0))
    subprocess.check_call("gzip -1 -c %s > %s.gz" % (small, small), shell=True)
    m = clairvoyante_v3.Clairvoyante(); m.init(); m.setParameters(common.bench_params(O, "full", seed=11))
    chk = os.path.join(tmp, "model-000001"); m.saveParameters(chk); m.close()
    # a list of compressed files (one per chunk of the genome, the form that scales): 8 copies of the small .gz, read ahead
    # several at a time by one process (utils_v2.GetTensorFiles)
    copies = []
    for i in range(8):
        c = os.path.join(tmp, "c%d.txt.gz" % i)
        os.link(small + ".gz", c)
        copies.append(c)
    gzlist = ",".join(copies)
    want = {txt: n, small: ngz, small + ".gz": ngz, gzlist: 8 * ngz}
    for fn in (txt, txt, small, small + ".gz", gzlist, gzlist):          # the large file twice: the second pass finds it in the page cache
        n = want[fn]
        a = types.SimpleNamespace(tensor_fn=fn, chkpnt_fn=chk, call_fn=os.path.join(tmp, "out.vcf"), qual=None,
                                  sampleName="S", ref_fn=None, threads=None, showRef=False, v3=True, v2=False, slim=False)
        pr = cProfile.Profile()
        t0 = time.time(); pr.enable(); callVar.Run(a); pr.disable(); dt = time.time() - t0
        nrec = sum(1 for l in open(a.call_fn) if not l.startswith("#"))
        print("%s: %.2f s -> %.0f rows/s, %d VCF records" % (os.path.basename(fn) if "," not in fn else "8 x s.txt.gz as a list", dt, n / dt, nrec))
        pstats.Stats(pr).sort_stats("tottime").print_stats(6)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
