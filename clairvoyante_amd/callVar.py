"""Variant-calling driver: same command line, VCF output and function surface as
/root/reference/clairvoyante/callVar.py (Run :21-47, Output :50-153, PrintVCFHeader
:156-178, Test :180-216, main :219-262).

    python -m clairvoyante_amd.callVar --chkpnt_fn MODEL --tensor_fn TENSORS.gz --call_fn OUT.vcf

Pipeline (one process per GPU): a reader thread parses text tensors into pinned batches
(native parser), the GPU runs the network and the per-candidate arg-max / quality / depth
reductions (cv_call_postproc), and the host formats VCF lines only for the candidates
that produce one.  `Output()` keeps the reference's signature (host arrays in, text out)
and is the formatter both paths share.  CV_VCF_FORMAT=device (opt-in) writes the lines on the GPU instead
(cv_vcf_records_dev, csrc/cv_vcf_dev.hip): the same bytes, and what returns per batch is the text alone.
"""
import argparse
import ctypes
import logging
import os
import sys
import time
from math import log

import numpy as np

if __package__ in (None, ""):      # run as `python <dir>/callVar.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import param

logging.basicConfig(format='%(message)s', level=logging.INFO)
num2base = dict(zip((0, 1, 2, 3), "ACGT"))
base2num = dict(zip("ACGT", (0, 1, 2, 3)))
v2Zygosity2Name = dict(zip((0, 1), ('HET', 'HOM')))
v2Type2Name = dict(zip((0, 1, 2, 3), ('REF', 'SNP', 'INS', 'DEL')))
v2Length2Name = dict(zip((0, 1, 2, 3, 4, 5), ('0', '1', '2', '3', '4', '4+')))
maxVarLength = 5
inferIndelLengthMinimumAF = 0.125
_F = param.flankingBaseNum


def _top2_products(t, z, l):
    """fp32 products of the best and second-best probabilities of the three softmax heads
    (np.sort(x)[::-1][0/1], callVar.py:69-72); evaluated left to right in fp32 like NumPy.  The order is NumPy's
    ascending sort reversed: NaN first, equal values (+0 beside -0, NaN beside NaN) the higher index first -- a
    stable argsort, so that it does not depend on which sort NumPy picks for a row ("Decisions")."""
    def desc(h):
        return np.take_along_axis(h, np.argsort(h, axis=1, kind="stable")[:, ::-1], axis=1)
    st = desc(t); sz = desc(z); sl = desc(l)
    p1 = (st[:, 0] * sz[:, 0]) * sl[:, 0]
    p2 = (st[:, 1] * sz[:, 1]) * sl[:, 1]
    return p1.astype(np.float32), p2.astype(np.float32)


def _base_order(base):
    """base.argsort()[::-1] per row (callVar.py:81): descending, NaN first, the higher index first among equal values"""
    return np.argsort(base, axis=1, kind="stable")[:, ::-1]


def _qual(p1, p2):
    """callVar.py:72 with reference-era promotion: fp32 products, then float64."""
    return int(-4.343 * log((float(p2) + 1e-300) / (float(p1) + 1e-300)))


def _depth(X):
    """dp of callVar.py:86-87 for every candidate (values are integers: exact in fp32)"""
    return ((X[:, _F, :, 0].sum(1, dtype=np.float32) + X[:, _F + 1, :, 1].sum(1, dtype=np.float32))
            + X[:, _F + 1, :, 2].sum(1, dtype=np.float32)) + X[:, _F, :, 3].sum(1, dtype=np.float32)


def _format_record(args, x, pos, varType, varZygosity, varLength, base1, base2, qual, dp):
    """One VCF line (or None when dp == 0) from per-candidate decisions; x is the candidate's
    [33,4,4] tensor.  Allele / length inference of callVar.py:88-153."""
    if dp == 0:
        return None
    chromosome, coordination, refSeq = pos.split(":")
    coordination = int(coordination)
    info = []
    inferred = 0
    refBase = refSeq[_F]
    if varType == 1 or varType == 0:
        b1 = num2base[base1]; b2 = num2base[base2]
        altBase = refBase if varType == 0 else (b1 if b1 != refBase else b2)
        af = x[_F, base2num[altBase], 3] / dp
    elif varType == 2:
        if varLength == 0:
            varLength = 1
        af = x[_F + 1, :, 1].sum(dtype=np.float32) / dp
        ins = ""
        if varLength != maxVarLength:
            for k in range(_F + 1, _F + varLength + 1):
                ins += num2base[int(np.argmax(x[k, :, 1]))]
        else:
            for k in range(_F + 1, 2 * _F + 1):
                if k < (_F + maxVarLength) or x[k, :, 1].sum(dtype=np.float32) >= inferIndelLengthMinimumAF * x[k, :, 0].sum(dtype=np.float32):
                    inferred += 1
                    ins += num2base[int(np.argmax(x[k, :, 1]))]
                else:
                    break
        if inferred >= _F:
            altBase = "<INS>"
            info.append("SVTYPE=INS")
        else:
            altBase = refBase + ins
    else:
        if varLength == 0:
            varLength = 1
        af = x[_F + 1, :, 2].sum(dtype=np.float32) / dp
        if varLength == maxVarLength:
            for k in range(_F + 1, 2 * _F + 1):
                if k < (_F + maxVarLength) or x[k, :, 2].sum(dtype=np.float32) >= inferIndelLengthMinimumAF * x[k, :, 0].sum(dtype=np.float32):
                    inferred += 1
                else:
                    break
        if inferred >= _F:
            altBase = "<DEL>"
            info.append("SVTYPE=DEL")
        elif varLength != maxVarLength:
            refBase = refSeq[_F:_F + varLength + 1]
            altBase = refSeq[_F]
        else:
            refBase = refSeq[_F:_F + inferred + 1]
            altBase = refSeq[_F]
    if 0 < inferred < _F:
        info.append("LENGUESS=%d" % inferred)
    infoStr = ";".join(info) if info else "."
    if varType == 0:
        gt = "0/0"
    else:
        gt = "0/1" if varZygosity == 0 else "1/1"
    filt = "."
    if args.qual is not None:
        filt = "PASS" if qual >= args.qual else "LowQual"
    return "%s\t%d\t.\t%s\t%s\t%d\t%s\t%s\tGT:GQ:DP:AF\t%s:%d:%d:%.4f" % (
        chromosome, coordination, refBase, altBase, qual, filt, infoStr, gt, qual, dp, af)


def Output(args, call_fh, num, XBatch, posBatch, base, z, t, l):
    """callVar.py:50-153: writes the VCF records of one batch given host arrays."""
    if num != len(base):
        sys.exit("Inconsistent shape between input tensor and output predictions %d/%d" % (num, len(base)))
    if num == 0:
        return
    X = np.asarray(XBatch, dtype=np.float32)
    base = np.asarray(base); z = np.asarray(z); t = np.asarray(t); l = np.asarray(l)
    varType = np.argmax(t, axis=1)
    keep = np.arange(num) if args.showRef else np.nonzero(varType != 0)[0]
    if keep.size == 0:
        return
    varZyg = np.argmax(z, axis=1)
    varLen = np.argmax(l, axis=1)
    p1, p2 = _top2_products(t[keep], z[keep], l[keep])
    order = _base_order(base[keep])
    dp = _depth(X[keep])
    lines = []
    for i, j in enumerate(keep):
        rec = _format_record(args, X[j], posBatch[j], int(varType[j]), int(varZyg[j]), int(varLen[j]),
                             int(order[i, 0]), int(order[i, 1]), _qual(p1[i], p2[i]), dp[i])
        if rec is not None:
            lines.append(rec)
    if lines:
        call_fh.write("\n".join(lines) + "\n")


def PrintVCFHeader(args, call_fh):
    """callVar.py:156-178"""
    hdr = ['##fileformat=VCFv4.1',
           '##FILTER=<ID=PASS,Description="All filters passed">',
           '##FILTER=<ID=LowQual,Description="Confidence in this variant being real is below calling threshold.">',
           '##ALT=<ID=DEL,Description="Deletion">',
           '##ALT=<ID=INS,Description="Insertion of novel sequence">',
           '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
           '##INFO=<ID=LENGUESS,Number=.,Type=Integer,Description="Best guess of the indel length">',
           '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
           '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype Quality">',
           '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read Depth">',
           '##FORMAT=<ID=AF,Number=1,Type=Float,Description="Estimated allele frequency in the range (0,1)">']
    if args.ref_fn is not None:
        with open(args.ref_fn + ".fai") as fai_fp:
            for line in fai_fp:
                fields = line.strip().split("\t")
                hdr.append("##contig=<ID=%s,length=%d>" % (fields[0], int(fields[1])))
    hdr.append('#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s' % (args.sampleName))
    call_fh.write("\n".join(hdr) + "\n")


_tls = __import__("threading").local()


def _out_buffer(cap):
    """a grow-only output buffer per calling thread (a fresh ctypes buffer is zero-filled on every call)"""
    buf = getattr(_tls, "buf", None)
    if buf is None or len(buf) < cap:
        buf = _tls.buf = (ctypes.c_char * max(cap, 1 << 20))()
    return buf


def format_records(args, num, X, pos, call, qual, xrow=None):
    """The VCF text (bytes) of one batch through the native formatter (cv_format_vcf, csrc/cv_hostio.cpp):
    `call` [num,8] int32 / `qual` [num,4] fp32 host arrays from cv_call_postproc, X the tensors ([rows,33,4,4]
    fp32, C-contiguous; candidate i = row xrow[i], or row i), pos a utils_v2.PosBatch or a sequence of
    "chrom:coord:seq" strings.  Same records as `_format_record` line for line (tests/test_host_golden.py)."""
    from . import _lib
    from .utils_v2 import PosBatch
    if num == 0:
        return b""
    lib = _lib.load()
    if not isinstance(pos, PosBatch):
        pos = PosBatch.from_strings([pos[i] for i in range(num)])
    call = np.ascontiguousarray(call, dtype=np.int32); qual = np.ascontiguousarray(qual, dtype=np.float32)
    X = np.ascontiguousarray(X, dtype=np.float32)
    if xrow is not None:
        xrow = np.ascontiguousarray(xrow, dtype=np.int64)
    out = []
    nlen = ctypes.c_int64(); nrec = ctypes.c_int64()
    row_bytes = X.strides[0] if X.ndim > 1 else 0
    for start, rows, buf, meta in pos.pieces():
        if rows == 0:
            continue
        stop = min(start + rows, num)
        if stop <= start:
            break
        n = stop - start
        kept = n if args.showRef else int(np.count_nonzero(call[start:stop, 0]))
        if kept == 0:
            continue
        meta = np.ascontiguousarray(meta, dtype=np.int64)
        cap = kept * (int(meta[:n, 1].max()) + 160)
        if isinstance(buf, np.ndarray):              # a view of the memory-mapped input: its address, no copy
            hold = buf if buf.flags.c_contiguous else np.ascontiguousarray(buf)
            cbuf = ctypes.c_void_p(hold.ctypes.data)
        else:
            cbuf = buf if isinstance(buf, bytes) else bytes(buf)
        xptr = X.ctypes.data + (0 if xrow is not None else start * row_bytes)
        xr = ctypes.c_void_p(xrow.ctypes.data + start * 8) if xrow is not None else None
        for _try in range(2):
            dst = _out_buffer(cap)
            rc = lib.cv_format_vcf(ctypes.c_void_p(call.ctypes.data + start * 32), ctypes.c_void_p(qual.ctypes.data + start * 16),
                                   n, ctypes.c_void_p(xptr), xr, cbuf, ctypes.c_void_p(meta.ctypes.data), None,
                                   1 if args.showRef else 0, 0 if args.qual is None else 1,
                                   0 if args.qual is None else int(args.qual), dst, cap, ctypes.byref(nlen), ctypes.byref(nrec))
            if rc != 2:
                break
            cap = nlen.value
        _lib.check(rc)
        out.append(ctypes.string_at(dst, nlen.value))
    return b"".join(out)


def OutputFromDevice(args, call_fh, num, XBatch, posBatch, call, qual, xrow=None):
    """Formatter of the GPU path: `call` [n,8] int32 and `qual` [n,4] fp32 come from cv_call_postproc (arg-maxes,
    two best bases, the fp32 top-2 products, dp); the records are written by the native formatter."""
    text = format_records(args, num, XBatch, posBatch, call, qual, xrow)
    if text:
        call_fh.write(text.decode("ascii"))


# ---- the same records written on the device (csrc/cv_vcf_dev.hip) ----------------------------------------------------
# CV_VCF_FORMAT=host|device chooses who writes the records of called_batches; unset means the host (cv_format_vcf), as
# before: measured, the device route wins with --showRef and ties without it, and no default was chosen from that.
_vcf_counts = {"host": 0, "device": 0, "handed_over": 0}
_vcf_counts_lock = __import__("threading").Lock()      # called_batches may run on one thread per GPU


def _count_batch(*sides):
    with _vcf_counts_lock:
        for side in sides:
            _vcf_counts[side] += 1


def vcf_format_route():
    """"host" or "device": CV_VCF_FORMAT, "host" when it is not set"""
    forced = os.environ.get("CV_VCF_FORMAT")
    if forced in ("host", "device"):
        return forced
    if forced:
        raise ValueError("CV_VCF_FORMAT must be 'host' or 'device', got %r" % forced)
    return "host"


def vcf_format_counts():
    """batches of called_batches whose records the host / the device wrote, and how many of the host's the device
    handed over (a batch with a candidate cv_vcf_records_dev does not vouch for goes to cv_format_vcf whole)"""
    with _vcf_counts_lock:
        return dict(_vcf_counts)


def _packed_tokens(buf, meta):
    """-> (bytes, meta): the tokens `meta` names inside `buf`, packed end to end when `buf` holds much more than them (a
    host-parsed batch's pieces are views of the input text, ~2.3 KB per row for ~40 bytes of tokens)"""
    b = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, dtype=np.uint8)
    lens = meta[:, 1::2].reshape(-1)
    total = int(lens.sum())
    if len(b) <= 2 * total + 4096:
        return b, meta
    new = np.cumsum(lens) - lens
    idx = np.repeat(meta[:, 0::2].reshape(-1) - new, lens) + np.arange(total, dtype=np.int64)
    packed = meta.copy()
    packed[:, 0::2] = new.reshape(-1, 3)
    return b[idx], packed


def device_tokens(text, meta, first=0):
    """what a PosBatch carries as `.device` when its tokens lie in HBM: the address of the bytes, of the [rows,6] meta
    from row `first` on, no row index, nothing parsed on the host"""
    return {"text_ptr": text.data_ptr(), "meta_ptr": meta.data_ptr() + first * 48, "keep": None, "merged": False,
            "hold": (text, meta)}


def predict_and_reduce(m, xd):
    """network + per-candidate reductions on the device: x [n,33,4,4] -> (call [n,8] int32, qual [n,4] fp32)"""
    import torch
    from . import _lib
    num = xd.shape[0]
    out = m.predict_device(xd)
    call = torch.empty((num, 8), dtype=torch.int32, device=m.device)
    qual = torch.empty((num, 4), dtype=torch.float32, device=m.device)
    _lib.check(m._lib.cv_call_postproc(m._h, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(out.data_ptr()), num,
                                       ctypes.c_void_p(call.data_ptr()), ctypes.c_void_p(qual.data_ptr()), m._stream()))
    return call, qual


class ResultFetcher(object):
    """Brings the per-candidate decisions of a batch to the host WITHOUT queueing behind the next batch's kernels:
    the copies run on a side stream that waits for the event recorded after the batch's own kernels, into page-locked
    buffers, so the host formats batch k while the GPU computes batch k+1 (callVar.py:197-204 overlaps Output(k) with
    predict(k+1) the same way)."""

    def __init__(self, m):
        import torch
        self.m = m
        self.side = torch.cuda.Stream(device=m.device)

    def mark(self):
        """call right after enqueueing a batch's kernels on the current stream"""
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.m.device))
        return ev

    def fetch(self, ev, call_d, qual_d, x_dev=None, show_ref=False):
        """-> (call, qual) host arrays; with x_dev also (rows [k,33,4,4] of the candidates that give a record, xrow [n]
        = row of candidate i in `rows`) -- only those rows cross PCIe"""
        import torch
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            call_h = torch.empty(call_d.shape, dtype=call_d.dtype, pin_memory=True)
            qual_h = torch.empty(qual_d.shape, dtype=qual_d.dtype, pin_memory=True)
            call_h.copy_(call_d, non_blocking=True); qual_h.copy_(qual_d, non_blocking=True)
            self.side.synchronize()
            call = call_h.numpy(); qual = qual_h.numpy()
            if x_dev is None:
                return call, qual
            n = call.shape[0]
            keep = np.arange(n) if show_ref else np.flatnonzero(call[:, 0] != 0)
            xrow = np.zeros(n, dtype=np.int64)
            xrow[keep] = np.arange(len(keep))
            if len(keep) == 0:
                return call, qual, np.zeros((0, 33, 4, 4), np.float32), xrow
            idx = torch.from_numpy(keep).to(self.m.device, non_blocking=True)
            rows_h = torch.empty((len(keep),) + tuple(x_dev.shape[1:]), dtype=torch.float32, pin_memory=True)
            rows_h.copy_(x_dev.index_select(0, idx), non_blocking=True)
            self.side.synchronize()
            return call, qual, rows_h.numpy(), xrow

    def upload(self, arrays):
        """host arrays (8-byte aligned sizes first) as ONE block of HBM, copied on the side stream from a page-locked
        buffer so that it does not queue behind the kernels of the batch before; the current stream waits for it.
        -> (uint8 tensor, byte offset of each array in it, the page-locked buffer: to be held until the copy has run)"""
        import torch
        offs = np.cumsum([0] + [(a.nbytes + 7) & ~7 for a in arrays])
        stage = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
        h = stage.numpy()
        for a, o in zip(arrays, offs):
            h[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        with torch.cuda.stream(self.side):
            block = stage.to(self.m.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.side)
        torch.cuda.current_stream(self.m.device).wait_event(ev)
        return block, [int(o) for o in offs[:-1]], stage

    def fetch_text(self, ev, parts):
        """the records cv_vcf_records_dev wrote for a batch (enqueue_records): the 32 bytes of info per call, then exactly
        info[0] bytes of text -> bytes, or None when a candidate was left to the host (info[2] > 0)"""
        import torch
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            info_h = torch.empty((len(parts), 4), dtype=torch.int64, pin_memory=True)
            for k, p in enumerate(parts):
                info_h[k].copy_(p["info"], non_blocking=True)
            self.side.synchronize()
            info = info_h.numpy()
            if int(info[:, 2].sum()) > 0:
                return None
            total = int(info[:, 0].sum())
            if total == 0:
                return b""
            text_h = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            at = 0
            for k, p in enumerate(parts):
                nb = int(info[k, 0])
                if nb:
                    text_h[at:at + nb].copy_(p["text"][:nb], non_blocking=True)
                at += nb
            self.side.synchronize()
            return text_h.numpy().tobytes()


def enqueue_records(args, m, fetcher, num, xd, pos, call, qual):
    """cv_vcf_records_dev for one batch on the current stream, right behind its cv_call_postproc: one call per piece of
    `pos`.  The tokens are read where they lie in HBM when the batch says so (pos.device: GetTensorDevice with
    keep_device, CallFromDevice); otherwise the piece's tokens and meta are uploaded, ~90 bytes per row.  text_cap is
    the host's own bound, n (longest contig token + 160).  -> [{"info": [4] int64, "text": uint8, ...}] in HBM, for
    ResultFetcher.fetch_text; `call`, `qual` and the rows of xd stay where they are."""
    import torch
    from . import _lib
    from .utils_v2 import PosBatch
    lib, dev = _lib.load(), m.device
    if not isinstance(pos, PosBatch):
        pos = PosBatch.from_strings([pos[i] for i in range(num)])
    d = getattr(pos, "device", None)
    calls = []                               # (first candidate, n, text address, meta address, row index tensor or None, longest contig, held)
    if d is not None and not d["merged"] and d.get("text_ptr") and d.get("meta_ptr"):
        longest = d.get("longest")           # (a batch made on the device knows it without its host copy: DevicePosBatch)
        if longest is None:
            longest = max([int(meta[:, 1].max()) for _s, rows, _b, meta in pos.pieces() if rows] or [0])
        keep = None if d["keep"] is None else fetcher.upload([np.ascontiguousarray(d["keep"], dtype=np.int64)])
        calls.append((0, num, d["text_ptr"], d["meta_ptr"], keep[0] if keep else None, longest, (d, keep)))
    else:
        for start, rows, buf, meta in pos.pieces():
            n = min(start + rows, num) - start
            if n <= 0:
                continue
            tok, tmeta = _packed_tokens(buf, np.ascontiguousarray(meta[:n], dtype=np.int64))
            block, offs, stage = fetcher.upload([tmeta, tok])
            calls.append((start, n, block.data_ptr() + offs[1], block.data_ptr() + offs[0], None, int(tmeta[:, 1].max()), (block, stage)))
    parts = []
    for start, n, text_ptr, meta_ptr, keep, longest, held in calls:
        need = _lib.workspace(lib.cv_vcf_records_workspace, n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        small = torch.empty(4 + n + 1, dtype=torch.int64, device=dev)            # info | off
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        cap = n * (longest + 160)
        text = torch.empty(cap, dtype=torch.uint8, device=dev)
        _lib.check(lib.cv_vcf_records_dev(
            ctypes.c_void_p(call.data_ptr() + start * 32), ctypes.c_void_p(qual.data_ptr() + start * 16), n,
            ctypes.c_void_p(xd.data_ptr() + start * 2112), None, ctypes.c_void_p(text_ptr), ctypes.c_void_p(meta_ptr),
            ctypes.c_void_p(keep.data_ptr()) if keep is not None else None, 1 if args.showRef else 0, 0 if args.qual is None else 1,
            0 if args.qual is None else int(args.qual), ctypes.c_void_p(small.data_ptr() + 32), ctypes.c_void_p(status.data_ptr()),
            ctypes.c_void_p(small.data_ptr()), ctypes.c_void_p(text.data_ptr()), cap, ctypes.c_void_p(ws.data_ptr()), need,
            m._stream()))
        parts.append({"info": small[:4], "text": text, "held": (ws, small, status, held)})
    return parts


def called_batches(args, m, items):
    """The call loop: `items` are (key, num, X, pos) batches -- X a host array ([num,33,4,4] fp32, copied to the
    device here) or rows that are in HBM already (a torch tensor) -- and (key, None, None, None) end markers.  Yields
    (key, VCF text of the batch as bytes) ONE BATCH BEHIND what it has enqueued: per batch the H2D copy (or the device
    rows), predict_device, cv_call_postproc and an event go to the GPU, then the decisions of the batch before come to
    the host on the fetcher's side stream and are formatted while the GPU works.  End markers pass through in order,
    as (key, None), behind the text of the batches in front of them.  Closes `items` when it ends, however it ends."""
    import torch
    try:
        with torch.cuda.device(m.device):
            fetcher = ResultFetcher(m)
            pending = None                   # (key, num, X, pos, call_dev, qual_dev, records, event) of the batch the GPU works on
            on_device = vcf_format_route() == "device"

            def finish(key, num, X, pos, call, qual, records, ev):
                if records is not None:      # the records were written in HBM: 32 bytes of info, then the text itself
                    text = fetcher.fetch_text(ev, records)
                    if text is not None:
                        _count_batch("device")
                        return key, text
                    _count_batch("handed_over")            # a candidate the device does not vouch for: the batch goes the host's way
                _count_batch("host")
                if torch.is_tensor(X):       # rows on the device: only those that give a record come to the host
                    hcall, hqual, rows, xrow = fetcher.fetch(ev, call, qual, X, bool(args.showRef))
                    return key, format_records(args, num, rows, pos, hcall, hqual, xrow)
                hcall, hqual = fetcher.fetch(ev, call, qual)
                return key, format_records(args, num, X, pos, hcall, hqual)

            for key, num, X, pos in items:
                nxt = None
                if num:
                    xd = X if torch.is_tensor(X) else torch.from_numpy(X).to(m.device, non_blocking=True)
                    call, qual = predict_and_reduce(m, xd)
                    records = enqueue_records(args, m, fetcher, num, xd, pos, call, qual) if on_device else None
                    nxt = (key, num, X, pos, call, qual, records, fetcher.mark())
                if pending is not None:      # format batch k while the GPU works on batch k + 1
                    yield finish(*pending)
                pending = nxt
                if num is None:              # end of `key` (its last batch was formatted just above)
                    yield key, None
            if pending is not None:
                yield finish(*pending)
    finally:
        items.close()


def CallFromDevice(args, m, call_fh, X_dev, pos, batch=65536):
    """VCF records for tensors that are already in HBM (callVarBam's fused path): X_dev [n,33,4,4] with matrices 1..3
    minus matrix 0; pos: utils_v2.PosBatch (or a function i -> "chrom:coord:seq") for the n rows.  Batch k's decisions
    and the rows that produce a record (non-REF calls, or all with --showRef) come to the host on a side stream and
    are formatted by the host threads while the GPU runs batch k+1 (called_batches).  A utils_v2.DevicePosBatch (its
    tokens lie in HBM already) is cut into parts that point there: nothing is uploaded for it, and its host copy is
    fetched only if a batch is formatted by the host."""
    from .utils_v2 import DevicePosBatch, PosBatch
    n = X_dev.shape[0]
    if isinstance(pos, DevicePosBatch):
        if len(pos) != n:
            raise ValueError("CallFromDevice: %d positions for %d tensors" % (len(pos), n))
        slices = ((0, min(batch, n - s), X_dev[s:s + batch].contiguous(), pos.part(s, batch)) for s in range(0, n, batch))
        for _key, text in called_batches(args, m, slices):
            call_fh.write(text.decode("ascii"))
        return
    if callable(pos):
        pos = PosBatch.from_strings([pos(i) for i in range(n)])
    pieces = pos.pieces()
    if len(pieces) != 1:
        pos = PosBatch.from_strings(list(pos))
        pieces = pos.pieces()
    _start, _rows, buf, meta = pieces[0]
    tokens = None
    if n and vcf_format_route() == "device":         # the records are written in HBM: the tokens go there once, not per slice
        import torch
        b = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, dtype=np.uint8)
        tokens = (torch.from_numpy(np.ascontiguousarray(b).copy()).to(X_dev.device),
                  torch.from_numpy(np.ascontiguousarray(meta[:n], dtype=np.int64).copy()).to(X_dev.device))

    def piece(s):
        p = PosBatch(buf, meta[s:s + batch])
        if tokens is not None:
            p.device = device_tokens(tokens[0], tokens[1], s)
        return p

    slices = ((0, min(batch, n - s), X_dev[s:s + batch].contiguous(), piece(s)) for s in range(0, n, batch))
    for _key, text in called_batches(args, m, slices):
        call_fh.write(text.decode("ascii"))


def Run(args):
    """callVar.py:21-47"""
    logging.info("Loading model ...")
    from . import utils_v2 as utils
    utils.SetupEnv()
    if args.v2:
        sys.exit("Clairvoyante v2 topologies are not part of this build (v3 / v3 slim only)")
    if args.slim:
        from . import clairvoyante_v3_slim as cv
    else:
        from . import clairvoyante_v3 as cv
    if args.threads is None:
        if args.tensor_fn == "PIPE":
            param.NUM_THREADS = 4
    else:
        param.NUM_THREADS = args.threads
    from . import parallel
    rank, ws, _local = parallel.init_from_env(os.environ.get("CV_DIST_BACKEND"))   # torchrun: one process per GPU
    m = cv.Clairvoyante()
    m.init()
    m.restoreParameters(os.path.abspath(args.chkpnt_fn))
    if ws > 1:
        TestSharded(args, m, utils, rank, ws)
    else:
        Test(args, m, utils)


def tensor_files(tensor_fn):
    """--tensor_fn as a list: "a.gz,b.gz,c.gz" names one tensor file per chunk of the genome, called in list order (one
    process) or file k by rank k % N (torchrun).  A name that exists as given is ONE file even if it holds a comma; PIPE
    stays PIPE.  (A list whose every item holds a comma of its own cannot be expressed: rename the files.)"""
    if tensor_fn == "PIPE" or "," not in tensor_fn or os.path.exists(tensor_fn):
        return [tensor_fn]
    return [f for f in tensor_fn.split(",") if f]


# input lines per block of the multi-rank split (block k -> rank k % N); CV_SHARD_BLOCK_LINES overrides (tests)
SHARD_BLOCK_LINES = int(os.environ.get("CV_SHARD_BLOCK_LINES", "16384"))


# The `range` route of a single file under several ranks (utils_v2.shard_span): rank r reads only the byte range -- of a
# BGZF file: the members -- that holds its lines.  Whether it is the default of a form ("text": plain text, "bgzf") follows
# from profiles/r18/sharded_reader.txt by the rule of CV_CALL_COLUMNS: ahead of the `lines` route in every run of every
# rung at 2 and at 4 ranks, or opt-in (CV_SHARD=range).  When it is the default it applies from a SHARE (file size // ranks)
# of the floor of the form upwards (TEXT_DEVICE_MIN_BYTES[0], BGZF_DEVICE_MIN_BYTES): the floors stand for fixed costs of
# the device reader, which every process pays for itself.  That reasoning has NOT been measured under ranks.
# Measured (1, 2, 4 processes on ONE GPU, the whole command per run): BGZF is ahead in every run at 1 M rows (2.7-3.0 s
# against 5.1-5.9 s with 2 ranks, 3.0-4.0 s against 5.9-6.5 s with 4) and in the medians at 65 536 and 262 144 rows, where
# its slowest run misses the fastest `lines` run by 0.3-21 %; plain text is within noise at every rung.  Both stay opt-in.
SHARD_RANGE_DEFAULT = {"text": False, "bgzf": False}
_shard_counts = {"lines": 0, "range": 0}


def shard_counts():
    """how often TestSharded took each route in this process: {"lines": .., "range": ..}"""
    return dict(_shard_counts)


def _shard_form(files):
    """"text" / "bgzf" when --tensor_fn is ONE regular file the ownership rule covers, None otherwise (a list of files,
    PIPE, a FIFO, ordinary gzip and the other formats `gzip -fdc` decodes, CV_TEXT=stream)"""
    from . import utils_v2
    if len(files) != 1 or files[0] == "PIPE" or not os.path.isfile(files[0]) or os.environ.get("CV_TEXT") == "stream":
        return None
    if utils_v2.is_compressed(files[0]):
        return "bgzf" if utils_v2.is_bgzf(files[0]) else None
    return "text"


def shard_route(tensor_fn, ws):
    """How `ws` ranks split --tensor_fn: "lines" (every rank reads the whole input and parses its blocks of lines; a list
    of files: file k by rank k % ws) or "range" (ONE plain-text or BGZF file, every rank reads only its byte range).
    CV_SHARD=lines|range forces a side -- `range` over an input the rule does not cover is an error --; unset, the input
    decides (SHARD_RANGE_DEFAULT and the floors, above)."""
    forced = os.environ.get("CV_SHARD")
    if forced and forced not in ("lines", "range"):
        raise ValueError("CV_SHARD must be 'lines' or 'range', got %r" % forced)
    files = tensor_files(tensor_fn)
    form = _shard_form(files)
    if forced == "range":
        if form is None:
            raise ValueError("CV_SHARD=range needs ONE regular tensor file that is plain text or BGZF, got %r" % tensor_fn)
        return "range"
    if forced == "lines" or form is None or not SHARD_RANGE_DEFAULT[form]:
        return "lines"
    floor = TEXT_DEVICE_MIN_BYTES[0] if form == "text" else BGZF_DEVICE_MIN_BYTES
    return "range" if floor is not None and os.path.getsize(files[0]) // ws >= max(floor, 1) else "lines"


def range_batches(utils, tensor_fn, rank, ws, device, keep_device=False, batch=65536):
    """the (endFlag, c, X, pos) batches of the lines rank `rank` of `ws` owns of ONE file: the ranged device reader, or the
    ranged host reader under CV_TEXT_PARSE=host and without a GPU"""
    forced = os.environ.get("CV_TEXT_PARSE")
    if forced and forced not in ("host", "device"):
        raise ValueError("CV_TEXT_PARSE must be 'host' or 'device', got %r" % forced)
    on_device = forced != "host" and utils._gpu_present()
    side = "device" if on_device else "host"
    utils.text_parse_counts[side] += 1
    logging.info("Text tensors are parsed on the %s (rank %d reads its range of %s)" % (side, rank, tensor_fn))
    if on_device:
        return utils.GetTensorDevice(tensor_fn, batch, device, log=False, keep_device=keep_device, part=(rank, ws))
    return utils.GetTensor(tensor_fn, batch, log=False, part=(rank, ws))


def merge_fragments(call_fn, ws, out_fh):
    """Rank 0: append the per-rank record fragments to the VCF in input order.  Rank r wrote CALL.rank<r> (its
    records, block after block) and CALL.rank<r>.idx (one line per block it owns: "<block> <bytes>"); block k
    belongs to rank k % ws, so walking k = 0, 1, 2, ... and taking the next <bytes> of that rank's fragment
    reproduces the single-process file -- the reference's own multi-process recipe is per-chunk VCFs joined by
    `vcfcat` (README.md:184-202)."""
    frags = [open("%s.rank%d" % (call_fn, r), "rb") for r in range(ws)]
    idx = []
    for r in range(ws):
        with open("%s.rank%d.idx" % (call_fn, r)) as f:
            idx.append([tuple(int(v) for v in line.split()) for line in f if line.strip()])
    nblocks = sum(len(i) for i in idx)
    for k in range(nblocks):
        r = k % ws
        if k // ws >= len(idx[r]) or idx[r][k // ws][0] != k:
            raise RuntimeError("fragment index of rank %d does not hold block %d" % (r, k))
        nbytes = idx[r][k // ws][1]
        if nbytes:
            data = frags[r].read(nbytes)
            if len(data) != nbytes:
                raise RuntimeError("fragment of rank %d is short at block %d" % (r, k))
            out_fh.write(data.decode("ascii"))
    for f in frags:
        f.close()
    for r in range(ws):
        os.remove("%s.rank%d" % (call_fn, r)); os.remove("%s.rank%d.idx" % (call_fn, r))


def TestSharded(args, m, utils, rank, ws):
    """Test() under torchrun (BASELINE configs[2]: candidates sharded over the GPUs of a node): candidates are
    independent (v3.py:54-138 has no cross-candidate state), so the ranks split the INPUT LINES block-cyclically,
    every rank calls its blocks with its own replica of the weights -- no collective on the data path -- and
    rank 0 joins the per-rank record fragments in input order: the VCF is byte-identical to the single-process
    one.  On the `range` route (shard_route) a rank does not even read the lines of the others: one plain-text or BGZF
    file is split by byte ranges and rank r's share is block r."""
    import torch
    import torch.distributed as dist
    # the fragments are files next to --call_fn that rank 0 reads back: one node, or a file system all ranks share
    if int(os.environ.get("LOCAL_WORLD_SIZE", str(ws))) != ws and rank == 0:
        logging.warning("callVar under %d ranks on several nodes: --call_fn must lie on a file system every rank shares" % ws)
    logging.info("Calling variants (rank %d of %d) ..." % (rank, ws))
    predictStart = time.time()
    files = tensor_files(args.tensor_fn)
    route = shard_route(args.tensor_fn, ws)         # (a mistyped CV_SHARD ends the run here, before any file exists)
    _shard_counts[route] += 1
    frag_fn = "%s.rank%d" % (args.call_fn, rank)
    frag = open(frag_fn, "wb")
    index = []

    # "--tensor_fn a.gz,b.gz,...": one file per chunk, file k -> rank k % ws (each rank inflates only its own files);
    # a single file: its LINES are split block-cyclically (every rank inflates the whole stream -- the job is then
    # capped by one core's gzip rate whatever the number of GPUs)
    # ... unless the file is plain text or BGZF and takes the `range` route (shard_route): rank r then reads only the
    # bytes (the BGZF members) that hold its share of the lines, and its whole share is block r
    if route == "lines" and len(files) == 1 and ws > 1 and rank == 0 and utils.is_compressed(files[0]):
        logging.warning("callVar: ONE compressed tensor file under %d ranks -- every rank inflates the whole stream to find its "
                        "line blocks, so the job runs at one core's inflate rate (~0.35 M rows/s) whatever the number of GPUs. "
                        "Rewrite the file as BGZF (python -m clairvoyante_amd.bgzf IN OUT), whose members the ranks can share "
                        "(CV_SHARD=range), give --tensor_fn a comma-separated list (one file per chunk of the genome; file k "
                        "goes to rank k mod N) or uncompressed text to scale." % ws)

    def batches():
        if route == "range":         # this rank's byte range of the one file: its batches are block `rank`
            for _end, c, X, pos in range_batches(utils, files[0], rank, ws, m.device, keep_device=vcf_format_route() == "device"):
                yield rank, c, X, pos
            yield rank, None, None, None
        elif len(files) > 1:         # this rank's files, compressed ones several at a time, batches as they complete
            for item in utils.GetTensorFiles(files, max(param.predictBatchSize, 16384), rank, ws, ordered=False):
                yield item
        else:                        # one batch per owned block of lines
            for block, num, X, pos in utils.GetTensorBlocks(files[0], SHARD_BLOCK_LINES, rank, ws):
                yield block, num, X, pos
                yield block, None, None, None

    # the fragment holds this rank's blocks / files in ascending order (merge_fragments walks k = 0, 1, 2, ...): text that
    # is ready before its turn waits in memory (_OrderedWriter); one index entry per block that was seen
    seen = set()

    def write(k, text):
        frag.write(text)
        if index and index[-1][0] == k:
            index[-1] = (k, index[-1][1] + len(text))
        else:
            index.append((k, len(text)))

    out = _OrderedWriter(write, first=rank, step=ws)

    failure = None
    try:
        for k, text in called_batches(args, m, utils._read_ahead(batches(), 4)):
            if text is None:             # block / file complete
                seen.add(k)
            out.put(k, text)
        # every block this rank owns gets an index entry, also one without records (merge_fragments counts them)
        have = dict(index)
        index = [(k, have.get(k, 0)) for k in sorted(seen)]
        frag.close()
        with open(frag_fn + ".idx", "w") as f:
            f.write("".join("%d %d\n" % e for e in index))
    except BaseException as e:          # the other ranks must not wait at the barrier for a rank that died
        failure = e
    # every rank learns whether all fragments are complete (MAX of a flag) before anyone merges or leaves
    flag = torch.tensor([1 if failure is not None else 0], dtype=torch.int32,
                        device=m.device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    if int(flag.item()) != 0:
        for fn in (frag_fn, frag_fn + ".idx"):
            try:
                os.remove(fn)
            except OSError:
                pass
        if failure is not None:
            raise failure
        sys.exit("callVar: another rank failed; no VCF written")
    if rank == 0:
        try:
            with open(args.call_fn, "w") as call_fh:
                PrintVCFHeader(args, call_fh)
                merge_fragments(args.call_fn, ws, call_fh)
        finally:                                    # also when the merge fails: no fragment is left behind
            for r in range(ws):
                for fn in ("%s.rank%d" % (args.call_fn, r), "%s.rank%d.idx" % (args.call_fn, r)):
                    try:
                        os.remove(fn)
                    except OSError:
                        pass
        logging.info("Total time elapsed: %.2f s" % (time.time() - predictStart))
    dist.barrier()


class _OrderedWriter(object):
    """VCF text of several input files, produced in any order, written in LIST order: the text of the file whose turn
    it is goes straight to the output, that of files further down the list waits in memory (records only -- a few per
    cent of the input rows) until the files in front of them are complete."""

    def __init__(self, write, first=0, step=1):
        self.write, self.next, self.step = write, first, step
        self.held, self.done = {}, set()

    def put(self, k, text):
        """what called_batches yields: the text of a batch of file k, or None behind its last batch"""
        if text is None:
            self.end(k)
        else:
            self.add(k, text)

    def add(self, k, text):
        if not text:
            return
        if k == self.next:
            self.write(k, text)
        else:
            self.held.setdefault(k, []).append(text)

    def end(self, k):
        self.done.add(k)
        while self.next in self.done:
            self.done.discard(self.next)
            self.next += self.step
            for text in self.held.pop(self.next, []):
                self.write(self.next, text)


# Smallest input (bytes on disk) whose text rows are parsed on the device: (plain text, compressed); None = never.
# Measured (profiles/r07/text_parse_device.txt): plain text wins from the 65 536-row rung (150 MB) upwards -- below it
# the fixed cost of the device path (streams, buffers, a round trip per slab) outweighs the host parser's time; a
# compressed file arrives at one core's inflate rate and the device path wins at no size.
TEXT_DEVICE_MIN_BYTES = (150000000, None)
# The same for a .gz that is BGZF through and through (utils_v2.is_bgzf), whose members the device inflates itself:
# bytes on disk, None = never.  Measured (profiles/r07/bgzf_device.txt): the device wins from the 16 384-row rung
# (3.8 MB on disk) upwards, 1.2 M rows/s against the host reader's 0.2-0.25 M there and 4.1 M against 0.37 M at 1 M rows;
# at 1 000 rows (0.23 MB) the fixed cost of the device path loses.
BGZF_DEVICE_MIN_BYTES = 3800000
# The same for an ordinary gzip file (one DEFLATE stream: `gzip`, Python's gzip module), whose block starts the device
# finds and whose chunks it inflates itself (utils_v2._gzip_slabs): bytes on disk, None = never.
# Measured (profiles/r09/gzip_device.txt, `gzip -6` files): the device wins from the 200 000-row rung (24.5 MB on disk)
# upwards, 0.79 M rows/s against the host reader's 0.55 M there and 1.41 M against 0.56 M at 1 M rows; at 65 536 rows
# (8 MB) and below it loses: one block is ~32 768 symbols decoded by one lane, twice (count, write), which is ~90 ms
# whatever the size of the file.
GZIP_DEVICE_MIN_BYTES = 24500000


def parses_on_device(tensor_fn):
    """Which text reader a one-file run uses is decided from the input, not by the user: the device parser
    (utils_v2.GetTensorDevice) for a regular file of at least TEXT_DEVICE_MIN_BYTES (BGZF_DEVICE_MIN_BYTES for a BGZF
    file, GZIP_DEVICE_MIN_BYTES for an ordinary gzip file, both of which that reader also inflates on the device), the host parser below that and for PIPE.  CV_TEXT_PARSE=host|device forces one side for a regular file -- it exists so that tests and
    tools/gpu_callvar_text_probe.py can run both readers over the same input, like CV_TEXT=stream."""
    from . import utils_v2
    if tensor_fn == "PIPE" or not os.path.isfile(tensor_fn):
        return False
    forced = os.environ.get("CV_TEXT_PARSE")
    if forced in ("host", "device"):
        return forced == "device"
    if forced:
        raise ValueError("CV_TEXT_PARSE must be 'host' or 'device', got %r" % forced)
    if utils_v2.is_compressed(tensor_fn):
        if utils_v2.is_bgzf(tensor_fn):
            floor = BGZF_DEVICE_MIN_BYTES
        else:                                    # (the floor of every compressed file, or the lower one of a gzip file's own)
            floor = TEXT_DEVICE_MIN_BYTES[1]
            if GZIP_DEVICE_MIN_BYTES is not None and utils_v2._map_gzip(tensor_fn) is not None:
                floor = GZIP_DEVICE_MIN_BYTES if floor is None else min(floor, GZIP_DEVICE_MIN_BYTES)
    else:
        floor = TEXT_DEVICE_MIN_BYTES[0]
    return floor is not None and os.path.getsize(tensor_fn) >= max(floor, 1)


def Test(args, m, utils):
    """callVar.py:180-216 re-cut for the GPU: reader thread(s) (inflate, parse) || GPU (predict + per-candidate
    reductions) || writer (format); the records of a file stay in the order of its rows, files in list order, so the VCF
    is the reference's record for record."""
    call_fh = open(args.call_fn, "w")
    PrintVCFHeader(args, call_fh)
    logging.info("Calling variants ...")
    predictStart = time.time()
    files = tensor_files(args.tensor_fn)
    # plain text is parsed where the page cache holds it at millions of rows/s: batches of 65 536 (the pass size of
    # the network); a compressed stream arrives at one core's inflate rate: smaller batches keep the stages overlapped
    on_device = len(files) == 1 and parses_on_device(files[0])
    mapped = on_device or utils._map_plain_text(files[0]) is not None      # (either way the rows arrive at millions per second)
    batch = getattr(args, "batch_size", None) or (65536 if mapped else max(param.predictBatchSize, 16384))

    def batches():
        if len(files) > 1:                       # a list of files: compressed ones are inflated several at a time and their
            for item in utils.GetTensorFiles(files, batch, 0, 1, ordered=False):         # batches taken as they complete
                yield item
        else:
            side = "device" if on_device else "host"
            utils.text_parse_counts[side] += 1
            logging.info("Text tensors are parsed on the %s" % side)
            # (records written on the device read the tokens where the parser left them: keep_device)
            for _end, c, X, pos in (utils.GetTensorDevice(files[0], batch, m.device, keep_device=vcf_format_route() == "device")
                                    if on_device else utils.GetTensor(files[0], batch)):
                yield 0, c, X, pos
            yield 0, None, None, None

    # the reader(s) run in a thread of their own; an exception there surfaces here (the reference loses it)
    out = _OrderedWriter(lambda _k, text: call_fh.write(text.decode("ascii")))
    for k, text in called_batches(args, m, utils._read_ahead(batches(), 2 if mapped else 4)):
        out.put(k, text)
    call_fh.close()
    logging.info("Total time elapsed: %.2f s" % (time.time() - predictStart))


_CLI = (   # flag, type, default, help  -- the reference's options and defaults (callVar.py:219-254)
    ("--tensor_fn", str, "PIPE", "Tensor input, use PIPE for standard input"),
    ("--chkpnt_fn", str, None, "Input a checkpoint for testing or continue training"),
    ("--call_fn", str, None, "Output variant predictions"),
    ("--qual", int, None, "If set, variant with equal or higher quality will be marked PASS, or LowQual otherwise, optional"),
    ("--sampleName", str, "SAMPLE", "Define the sample name to be shown in the VCF file"),
    ("--ref_fn", str, None, "Reference fasta file input, optional, print contig tags in the VCF header if set"),
    ("--threads", int, None, "Number of threads, optional"),
)
_SWITCHES = (("--showRef", False, "Show reference calls, optional"), ("--v3", True, "Use Clairvoyante version 3"),
             ("--v2", False, "Use Clairvoyante version 2"),
             ("--slim", False, "Train using the slim version of Clairvoyante, optional"))


def main():
    parser = argparse.ArgumentParser(
        description="Call variants using a trained Clairvoyante model and tensors of candididate variants")
    for flag, typ, default, text in _CLI:
        parser.add_argument(flag, type=typ, default=default, help=text)
    for flag, default, text in _SWITCHES:
        parser.add_argument(flag, type=param.str2bool, nargs='?', const=True, default=default, help=text)
    args = parser.parse_args()
    if not sys.argv[1:]:
        parser.print_help()
        sys.exit(1)
    Run(args)


if __name__ == "__main__":
    main()
