"""Host handle of the on-GPU pileup (include/clairvoyante_amd.h, "pileup front end"): SAM text in,
[n,33,4,4] count tensors in HBM out.  Behaviour of /root/reference/dataPrepScripts/CreateTensor.py
(OutputAlnTensor :93-246, GenerateTensor :23-54); see csrc/cv_pileup.hip for the decomposition.
"""
import ctypes
import os

import numpy as np

from . import _lib

FLANK = 16
WIDTH = 2 * FLANK + 1
CALL_COLUMNS_ROW_TEXT = 10 + WIDTH      # bytes of a row's coordinate and window at most (CV_CALL_COLUMNS_ROW_TEXT)
CALL_COLUMNS_MAX_CTG = 1024             # bytes of a contig name call_columns takes (CV_CALL_COLUMNS_MAX_CTG)
CALL_COLUMNS_MAX_ROWS = 1 << 27
FLUSH_COLUMNS = 1 << 26         # queue at most this many alignment columns on the host before a scatter launch

# BAM records on the device (csrc/cv_bam_dev.hip): `route` of Pileup.add_bam, else CV_BAM_DECODE=host|device, else the
# device from BAM_DEVICE_MIN_BYTES of file size on.  None: no measured size from which the device route wins in every
# run, so the route is opt-in and the default is the host.
BAM_DEVICE_MIN_BYTES = None
BAM_SLAB_BYTES = 64 << 20       # compressed bytes per slab; CV_BAM_SLAB_BYTES overrides (tests set it small)
_BAM_KEYS = ("host_views", "device_views", "device_slabs", "device_records", "device_members", "host_members",
             "handed_over_slabs", "handed_over_records", "walkers", "members")
_bam_counts = dict.fromkeys(_BAM_KEYS, 0)


def bam_decode_counts(reset=False):
    """what Pileup.add_bam did since the start (or the last reset), per side: views by route, slabs / records / BGZF
    members the device took, members the host had to inflate for it, slabs (and their records) handed over to the host
    because the device did not vouch for them, walkers that ran"""
    out = dict(_bam_counts)
    if reset:
        for k in _BAM_KEYS:
            _bam_counts[k] = 0
    return out


def _bam_route(route, bam_path):
    r = route if route is not None else os.environ.get("CV_BAM_DECODE")
    if r is None or r == "":
        if BAM_DEVICE_MIN_BYTES is None:
            return "host"
        try:
            return "device" if os.path.getsize(bam_path) >= BAM_DEVICE_MIN_BYTES else "host"
        except OSError:
            return "host"
    if r not in ("host", "device"):
        raise ValueError("BAM decode route %r: host or device" % (r,))
    return r


class Pileup(object):
    def __init__(self, device=None, minMQ=0, dcov=250, considerleftedge=True, evc=False, retain=False, evc_minMQ=0,
                 contig=None, threads=None):
        import torch
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.CvError("the pileup kernels need an MI355X (no GPU visible); there is no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.cv_pileup_create(self.device.index, int(minMQ), int(dcov), int(bool(considerleftedge)),
                                             ctypes.byref(self.h)))
        if evc:
            _lib.check(self.lib.cv_pileup_set_option(self.h, b"evc", 1))
            _lib.check(self.lib.cv_pileup_set_option(self.h, b"evc_min_mq", int(evc_minMQ)))
            if contig is not None:
                _lib.check(self.lib.cv_pileup_set_contig(self.h, contig.encode()))
        if retain:
            _lib.check(self.lib.cv_pileup_set_option(self.h, b"retain", 1))
        # SAM text is parsed by several host threads (chunks of >= 1 MiB); the result does not depend on the count
        self.threads = min(_lib.usable_cores(), 16) if threads is None else int(threads)
        _lib.check(self.lib.cv_pileup_set_option(self.h, b"threads", self.threads))
        self.n = 0
        self.centers = np.zeros(0, dtype=np.int64)
        self._tail = b""
        self.reads_kept = 0
        self._nsel = 0                  # entries of the last sample_candidates()

    def close(self):
        if getattr(self, "_bam_dev", None):
            self.lib.cv_bam_dev_destroy(self._bam_dev)
            self._bam_dev = None
        if getattr(self, "h", None):
            self.lib.cv_pileup_destroy(self.h)
            self.h = None

    __del__ = close

    def _stream(self):
        return _lib.stream_arg(self.device)

    def set_reference(self, seq, first_pos0=0):
        """seq: the bases `samtools faidx` printed (str/bytes); seq[0] is 0-based position first_pos0"""
        b = seq.encode() if isinstance(seq, str) else bytes(seq)
        _lib.check(self.lib.cv_pileup_set_reference(self.h, b, len(b), int(first_pos0)))

    def set_candidates(self, centers):
        """1-based candidate positions; sorted and de-duplicated here"""
        c = np.unique(np.asarray(centers, dtype=np.int64))
        self.centers = np.ascontiguousarray(c)
        self.n = len(c)
        _lib.check(self.lib.cv_pileup_set_candidates(self.h, self.centers.ctypes.data_as(ctypes.c_void_p), self.n))

    def _feed(self, data, off, final):
        """parse data[off:] in place (no copy); returns the bytes consumed"""
        n = len(data) - off
        if n <= 0:
            return 0
        consumed = ctypes.c_int64(0)
        kept = ctypes.c_int64(0)
        base = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value        # data stays referenced by the caller
        _lib.check(self.lib.cv_pileup_add_sam(self.h, ctypes.c_void_p(base + off), n, int(final), ctypes.byref(consumed),
                                              ctypes.byref(kept)))
        self.reads_kept += kept.value
        self._kept_now += kept.value
        return consumed.value

    def add_sam(self, chunk, final=False):
        """feed SAM text (bytes) in arbitrary chunks; an incomplete last line is kept for the next call"""
        self._kept_now = 0
        off = 0
        if self._tail:
            nl = chunk.find(b"\n")
            if nl < 0 and not final:
                self._tail += chunk
                return 0
            head = self._tail + (chunk if nl < 0 else chunk[:nl + 1])           # one line: the only bytes copied
            self._tail = b""
            self._feed(head, 0, final and nl < 0)
            off = len(chunk) if nl < 0 else nl + 1
        off += self._feed(chunk, off, final)
        if off < len(chunk):
            self._tail = chunk[off:]
        if self.lib.cv_pileup_pending(self.h) >= FLUSH_COLUMNS:
            _lib.check(self.lib.cv_pileup_flush(self.h, self._stream()))
        return self._kept_now

    def add_bam(self, bam, ref, start=None, end=None, exclude_flags=2308, contig_ok=True, window=64 << 20, route=None):
        """feed the records `samtools view -F exclude_flags BAM ref[:start-end]` would print, straight from the
        BAM (bam: clairvoyante_amd.bam.BamFile) -- no SAM text in between; same result as add_sam on that text.
        route: "host" (records walked and cut into segments by host threads), "device" (the compressed blocks go to
        the GPU, csrc/cv_bam_dev.hip; needs the .bai, a view without one takes the host route), None: CV_BAM_DECODE,
        else BAM_DEVICE_MIN_BYTES.  Same result either way; bam_decode_counts() tells which one ran."""
        self._kept_now = 0
        if self._tail:
            self.add_sam(b"", final=True)
        if _bam_route(route, bam.path) == "device":
            usable = ctypes.c_int(0)
            _lib.check(self.lib.cv_bam_view_plan_begin(bam.h, ref.encode(), int(start or 0), int(end or 0), int(exclude_flags),
                                                       ctypes.byref(usable)))
            if usable.value:
                return self._add_bam_device(bam, contig_ok)
        _bam_counts["host_views"] += 1
        _lib.check(self.lib.cv_bam_view_begin(bam.h, ref.encode(), int(start or 0), int(end or 0), int(exclude_flags), 0))
        base = ctypes.c_void_p(); offs = ctypes.c_void_p(); done = ctypes.c_int(0); kept = ctypes.c_int64(0)
        total = 0
        while not done.value:
            n = self.lib.cv_bam_view_records(bam.h, int(window), ctypes.byref(base), ctypes.byref(offs), ctypes.byref(done))
            if n < 0:
                _lib.check(1)
            if n:
                _lib.check(self.lib.cv_pileup_add_bam(self.h, base, offs, n, int(bool(contig_ok)), ctypes.byref(kept)))
                self.reads_kept += kept.value
                total += kept.value
                if self.lib.cv_pileup_pending(self.h) >= FLUSH_COLUMNS:
                    _lib.check(self.lib.cv_pileup_flush(self.h, self._stream()))
        return total

    def _add_bam_device(self, bam, contig_ok):
        if getattr(self, "_bam_dev", None) is None:
            self._bam_dev = ctypes.c_void_p()
            _lib.check(self.lib.cv_bam_dev_create(self.device.index, ctypes.byref(self._bam_dev)))
        slab = int(os.environ.get("CV_BAM_SLAB_BYTES") or BAM_SLAB_BYTES)
        kept = ctypes.c_int64(0)
        cnt = (ctypes.c_int64 * 8)()
        rc = self.lib.cv_bam_dev_view(self._bam_dev, bam.h, self.h, slab, int(bool(contig_ok)), self._stream(), ctypes.byref(kept), cnt)
        _bam_counts["device_views"] += 1
        for k, i in (("device_slabs", 0), ("device_records", 1), ("device_members", 2), ("host_members", 3),
                     ("handed_over_slabs", 4), ("walkers", 5), ("handed_over_records", 6), ("members", 7)):
            _bam_counts[k] += cnt[i]
        self.reads_kept += kept.value
        _lib.check(rc)
        return kept.value

    def bam_device_ms(self):
        """time (ms) of the device BAM route on this handle: host wall time between its synchronisations by phase (copies,
        launches and, in emit_handover, the pileup's own kernels included), and the HIP-event time of the inflate and the
        walk kernel alone"""
        ms = (ctypes.c_double * 7)()
        if getattr(self, "_bam_dev", None):
            _lib.check(self.lib.cv_bam_dev_times(self._bam_dev, ms))
        return dict(zip(("inflate", "walk", "count_scan", "emit_handover", "host_slabs", "inflate_kernel", "walk_kernel"), ms))

    def finish(self, subtract=False, want_tensors=True):
        """-> (tensors [n,33,4,4] fp32 on the device, depth [n] int32, touched [n] bool)"""
        import torch
        if self._tail:
            self.add_sam(b"", final=True)
        t = torch.empty((self.n, WIDTH, 4, 4), dtype=torch.float32, device=self.device) if want_tensors else None
        d = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        u = torch.empty((self.n,), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.cv_pileup_finish(self.h, ctypes.c_void_p(t.data_ptr()) if want_tensors and self.n else None,
                                             ctypes.c_void_p(d.data_ptr()) if self.n else None,
                                             ctypes.c_void_p(u.data_ptr()) if self.n else None, int(bool(subtract)),
                                             self._stream()))
        return t, d, u.bool()

    def extract_candidates(self, threshold=0.125, minCoverage=4, region=None, bed=None):
        """ExtractVariantCandidates.py's selection over the reads added so far (needs evc=True).
        region: (ctgStart, ctgEnd) as the reference compares them with the 0-based position (:181-183);
        bed: list of half-open (begin, end), or None.  -> dict(pos0, late, counts [n,7] in A,C,G,T,I,D,N
        order, reads)"""
        if self._tail:
            self.add_sam(b"", final=True)
        n = ctypes.c_int64(0)
        if bed is not None:
            bb = np.ascontiguousarray([b for b, _ in bed], dtype=np.int64)
            be = np.ascontiguousarray([e for _, e in bed], dtype=np.int64)
            nbed = len(bed)
        else:
            bb = be = np.zeros(1, dtype=np.int64)
            nbed = -1
        _lib.check(self.lib.cv_pileup_extract_candidates(
            self.h, float(threshold), float(minCoverage), int(region is not None), int(region[0]) if region else 0,
            int(region[1]) if region else 0, bb.ctypes.data_as(ctypes.c_void_p), be.ctypes.data_as(ctypes.c_void_p),
            nbed, self._stream(), ctypes.byref(n)))
        self._nsel = n.value
        return self.extracted()

    def adopt_candidates(self, lo1=None, hi1=None):
        """make the extracted positions (+1, optionally inside [lo1, hi1]) the candidate centres and scatter
        the retained alignments for them (needs retain=True)"""
        n = ctypes.c_int64(0)
        _lib.check(self.lib.cv_pileup_adopt_candidates(self.h, int(lo1 is not None), int(lo1 or 0), int(hi1 or 0),
                                                       self._stream(), ctypes.byref(n)))
        self.n = n.value
        self.centers = np.zeros(self.n, dtype=np.int64)
        _lib.check(self.lib.cv_pileup_get_candidates(self.h, self.centers.ctypes.data_as(ctypes.c_void_p), self.n,
                                                     ctypes.byref(n)))
        return self.centers

    def _bed_arrays(self, bed):
        if bed is None:
            z = np.zeros(1, dtype=np.int64)
            return z, z, -1
        return (np.ascontiguousarray([b for b, _ in bed], dtype=np.int64),
                np.ascontiguousarray([e for _, e in bed], dtype=np.int64), len(bed))

    def sample_candidates(self, seed, outputProb, region=None, bed=None):
        """ExtractVariantCandidates --gen4Training --seed on the device (needs evc=True and a contig): every position the
        candidate pass booked, inside region / bed as extract_candidates tests them, kept unless its stream-0 draw exceeds
        outputProb.  The entries stay in HBM -> their number; extracted() fetches them."""
        if self._tail:
            self.add_sam(b"", final=True)
        n = ctypes.c_int64(0)
        bb, be, nbed = self._bed_arrays(bed)
        _lib.check(self.lib.cv_pileup_sample_candidates(
            self.h, int(seed), float(outputProb), int(region is not None), int(region[0]) if region else 0,
            int(region[1]) if region else 0, bb.ctypes.data_as(ctypes.c_void_p), be.ctypes.data_as(ctypes.c_void_p), nbed,
            self._stream(), ctypes.byref(n)))
        self._nsel = n.value
        return n.value

    def select_candidates(self, threshold=0.125, minCoverage=4, region=None, bed=None):
        """extract_candidates' selection with the entries left in HBM (as sample_candidates leaves them) -> their number;
        selected_device() gathers them there, extracted() fetches them"""
        if self._tail:
            self.add_sam(b"", final=True)
        n = ctypes.c_int64(0)
        bb, be, nbed = self._bed_arrays(bed)
        _lib.check(self.lib.cv_pileup_select_candidates(
            self.h, float(threshold), float(minCoverage), int(region is not None), int(region[0]) if region else 0,
            int(region[1]) if region else 0, bb.ctypes.data_as(ctypes.c_void_p), be.ctypes.data_as(ctypes.c_void_p), nbed,
            self._stream(), ctypes.byref(n)))
        self._nsel = n.value
        return n.value

    def selected_device(self):
        """the entries of the last select_candidates() / sample_candidates() as device tensors, nothing fetched:
        dict(pos0 int64 [n], late int32 [n], counts int32 [n,7], reads, last_pos)"""
        import torch
        k = self._nsel
        with torch.cuda.device(self.device):
            pos0 = torch.empty(k, dtype=torch.int64, device=self.device)
            late = torch.empty(k, dtype=torch.int32, device=self.device)
            c7 = torch.empty((k, 7), dtype=torch.int32, device=self.device)
            info = (ctypes.c_int64 * 2)()
            _lib.check(self.lib.cv_pileup_selected_dev(self.h, _lib.ptr(pos0), _lib.ptr(late), _lib.ptr(c7), info, self._stream()))
        return {"pos0": pos0, "late": late, "counts": c7, "reads": info[0], "last_pos": info[1]}

    def extracted(self):
        """the entries of the last extract_candidates() / sample_candidates(): dict(pos0, late, counts [n,7] in
        A,C,G,T,I,D,N order, reads, last_pos)"""
        k = self._nsel
        pos0 = np.zeros(k, dtype=np.int64); late = np.zeros(k, dtype=np.int32); c7 = np.zeros((k, 7), dtype=np.int32)
        info = (ctypes.c_int64 * 2)()
        _lib.check(self.lib.cv_pileup_get_extracted(self.h, pos0.ctypes.data_as(ctypes.c_void_p),
                                                    late.ctypes.data_as(ctypes.c_void_p),
                                                    c7.ctypes.data_as(ctypes.c_void_p), info))
        return {"pos0": pos0, "late": late, "counts": c7, "reads": info[0], "last_pos": info[1]}

    def adopt_union(self, truth, lo1=None, hi1=None):
        """centres = sampled positions (+1, inside [lo1, hi1]) united with the ascending 1-based `truth` positions, made
        and flagged on the device; the retained alignments are scattered for them (needs retain=True) -> their number"""
        t = np.ascontiguousarray(truth, dtype=np.int64)
        n = ctypes.c_int64(0)
        _lib.check(self.lib.cv_pileup_adopt_union(self.h, int(lo1 is not None), int(lo1 or 0), int(hi1 or 0),
                                                  t.ctypes.data_as(ctypes.c_void_p), len(t), self._stream(), ctypes.byref(n)))
        self.n = n.value
        self.centers = None                 # (they stay in HBM; cv_pileup_get_candidates fetches them)
        return self.n

    def columns(self, depth, touched, minCoverage=0):
        """behind finish(): per centre the columns cv_trainset_finish sorts and labels by -> dict of device tensors
        pos int64, digits / centre / acgt / cflag / row uint8 (csrc/cv_bamtrain.hip)"""
        import torch
        n = self.n
        col = {"pos": torch.empty(n, dtype=torch.int64, device=self.device)}
        for k in ("digits", "centre", "acgt", "cflag", "row"):
            col[k] = torch.empty(n, dtype=torch.uint8, device=self.device)
        u8 = touched.to(torch.uint8)
        p = _lib.ptr
        _lib.check(self.lib.cv_bamtrain_columns(self.h, p(depth), p(u8), int(minCoverage), p(col["pos"]), p(col["digits"]),
                                                p(col["centre"]), p(col["acgt"]), p(col["cflag"]), p(col["row"]),
                                                self._stream()))
        return col

    def call_columns(self, touched, contig):
        """behind finish(): what callVarBam needs between the tensors and the call loop, made in HBM
        (csrc/cv_callcols_dev.hip) -> (index int64 [k] on the device: the centres that give a row -- touched, window
        starting inside the loaded reference, centre base one of ACGT -- ascending; utils_v2.DevicePosBatch of those k
        rows: the bytes and meta of PosBatch.from_columns(contig, centres[index], windows)).  Two integers come to the
        host here; the batch fetches its host copy only if someone reads it."""
        import torch
        from .utils_v2 import DevicePosBatch
        cb = contig if isinstance(contig, bytes) else str(contig).encode("ascii")
        n = self.n
        if touched.numel() != n:
            raise _lib.CvError("call_columns: %d flags for %d centres" % (touched.numel(), n))
        with torch.cuda.device(self.device):
            u8 = touched.contiguous().view(torch.uint8) if touched.dtype == torch.bool else touched.to(torch.uint8).contiguous()
            need = _lib.workspace(self.lib.cv_call_columns_workspace, n)
            cap = len(cb) + CALL_COLUMNS_ROW_TEXT * n
            # info [4] | index [n] | meta [n,6] | text: the meta and the text are neighbours, so one copy fetches both
            block = torch.empty(32 + 8 * n + 48 * n + cap + 8, dtype=torch.uint8, device=self.device)
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            base = block.data_ptr()
            _lib.check(self.lib.cv_pileup_call_columns(self.h, cb, len(cb), ctypes.c_void_p(u8.data_ptr()) if n else None,
                                                       ctypes.c_void_p(base + 32), ctypes.c_void_p(base + 32 + 8 * n),
                                                       ctypes.c_void_p(base + 32 + 56 * n), cap, ctypes.c_void_p(base),
                                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), self._stream()))
            k, nbytes = block[:16].view(torch.int64).tolist()         # (the synchronisation: ws and u8 are no longer in use)
            index = block[32:32 + 8 * k].view(torch.int64)
            return index, DevicePosBatch.over(block[32 + 8 * n:], k, 48 * n, nbytes, len(cb))

    def stats(self):
        ms = (ctypes.c_float * 3)()
        cnt = (ctypes.c_int64 * 3)()
        _lib.check(self.lib.cv_pileup_stats(self.h, ms, cnt))
        return {"scatter_ms": ms[0], "finalize_ms": ms[1], "candidate_ms": ms[2], "columns": cnt[0], "segments": cnt[1],
                "launches": cnt[2]}


def format_rows(ctg, centers, ref_seq, ref_shift, counts):
    """CreateTensor.py:50-52 text rows for host arrays: centers [k] (1-based), counts [k,33,4,4] raw.
    ref_shift = refStart-1 (0 when the whole contig was loaded)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64 + len(ctg) + WIDTH + WIDTH * 16 * 16)
    cb = ctg.encode()
    rb = ref_seq.encode() if isinstance(ref_seq, str) else ref_seq
    counts = np.ascontiguousarray(counts, dtype=np.float32)
    rows = []
    for k, c in enumerate(centers):
        new_pos = int(c) - ref_shift
        seq = rb[new_pos - (FLANK + 1):new_pos + FLANK]
        n = lib.cv_format_tensor_row(cb, int(c), seq, len(seq), counts[k].ctypes.data_as(ctypes.c_void_p), buf, len(buf))
        if n < 0:
            raise _lib.CvError("cv_format_tensor_row: buffer too small")
        rows.append(buf.raw[:n])
    return rows


# ---- the same rows written on the device (csrc/cv_rowtext_dev.hip) ---------------------------------------------------
# CV_ROW_FORMAT=host|device forces a side; without it the device formats a call of at least ROWTEXT_DEVICE_MIN_ROWS rows
# whose tensors lie on a GPU (None would make the route opt-in).  0: the device route won every run of every rung from
# 16 384 rows on, 9-12 times faster than the host loop (profiles/r15/rowtext_device.txt).
ROWTEXT_DEVICE_MIN_ROWS = 0
ROWTEXT_BATCH = 32768           # rows per block of text
_row_counts = {"host": 0, "device": 0}
_pinned = None                  # the host end of the text's copy, grown on demand and kept


def row_format_counts(reset=False):
    """rows formatted since the start (or the last reset) per side: {"host": n, "device": n}"""
    out = dict(_row_counts)
    if reset:
        _row_counts["host"] = _row_counts["device"] = 0
    return out


def _row_route(rows, on_gpu):
    r = os.environ.get("CV_ROW_FORMAT")
    if r is None or r == "":
        return "device" if on_gpu and ROWTEXT_DEVICE_MIN_ROWS is not None and rows >= ROWTEXT_DEVICE_MIN_ROWS else "host"
    if r not in ("host", "device"):
        raise ValueError("row format route %r: host or device" % (r,))
    return r


def _host_block(ctg, centers, ref_seq, ref_shift, counts):
    """one batch through format_rows -> its rows, each with its newline, as one block"""
    rows = format_rows(ctg, centers, ref_seq, ref_shift, counts.cpu().numpy() if hasattr(counts, "cpu") else counts)
    _row_counts["host"] += len(rows)
    rows.append(b"")
    return b"\n".join(rows)


def _pinned_bytes(n):
    import torch
    global _pinned
    if _pinned is None or _pinned.numel() < n:
        _pinned = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
    return _pinned


def format_rows_device(ctg, centers, ref_seq, ref_shift, tensors_dev, batch=ROWTEXT_BATCH, in_hbm=False):
    """format_rows on the device: yields, per batch of at most 32 768 rows, ONE block of bytes -- the rows format_rows
    gives for it, each followed by "\\n".  in_hbm: a batch the kernel printed is yielded where it lies, as a uint8
    tensor on the GPU (for utils_v2.BgzfWriter.write_device: the text never crosses); a batch the host takes stays bytes.
    tensors_dev [k,33,4,4] fp32 on a GPU; ref_seq bytes / str (uploaded once here)
    or a uint8 tensor already on that GPU.  A batch with a row the device does not vouch for (cv_tensor_rows_text_dev:
    status CV_ROWTEXT_HOST) is formatted whole by format_rows, so is one with a centre less than 17 bytes into the
    reference; row_format_counts() tells which side took what."""
    import torch
    if not tensors_dev.is_cuda:
        raise _lib.CvError("format_rows_device: the tensors are not on a GPU; there is no CPU form of the kernel")
    lib = _lib.load()
    dev = tensors_dev.device
    centers = np.ascontiguousarray(centers, dtype=np.int64)
    k = len(centers)
    if tensors_dev.dtype != torch.float32 or tuple(tensors_dev.shape) != (k, WIDTH, 4, 4):
        raise _lib.CvError("format_rows_device: tensors of shape %r for %d centres" % (tuple(tensors_dev.shape), k))
    cb = ctg.encode()
    host_ref = None if isinstance(ref_seq, torch.Tensor) else (ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq))
    with torch.cuda.device(dev):
        if host_ref is None:
            ref_dev = ref_seq
        else:
            ref_dev = torch.frombuffer(bytearray(host_ref) or bytearray(1), dtype=torch.uint8).to(dev)[:len(host_ref)]
        ref_len = int(ref_dev.numel())
        need = _lib.workspace(lib.cv_tensor_rows_text_workspace, min(batch, max(k, 1)))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        stream = _lib.stream_arg(dev)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        for s in range(0, k, batch):
            n = min(batch, k - s)
            cen = torch.from_numpy(centers[s:s + n]).to(dev)
            cnt = tensors_dev[s:s + n].contiguous()
            off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            status = torch.empty(n, dtype=torch.uint8, device=dev)

            def call(text, cap):
                _lib.check(lib.cv_tensor_rows_text_dev(cb, len(cb), ptr(cen), n, ptr(ref_dev) if ref_len else None, int(ref_shift),
                                                       ref_len, ptr(cnt), ptr(off), ptr(status), text, cap, ptr(ws), need,
                                                       stream))
            call(None, 0)                                   # lengths and status: the text is sized exactly
            total, host_rows = (int(v) for v in torch.stack((off[n], status.sum(dtype=torch.int64))).tolist())
            # (a window that starts in front of the reference: the kernel takes what lies inside, format_rows what Python's
            # negative slice index selects -- CreateTensor drops such a candidate, anyone else gets format_rows' bytes)
            if host_rows or int(centers[s:s + n].min()) - int(ref_shift) - (FLANK + 1) < 0:
                if host_ref is None:
                    host_ref = ref_dev.cpu().numpy().tobytes()
                yield _host_block(ctg, centers[s:s + n], host_ref, ref_shift, cnt)
                continue
            text = torch.empty(total, dtype=torch.uint8, device=dev)
            call(ptr(text), total)
            if in_hbm:
                _row_counts["device"] += n
                yield text
                continue
            pin = _pinned_bytes(total)
            pin[:total].copy_(text, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            _row_counts["device"] += n
            yield pin.numpy()[:total].tobytes()


def format_row_blocks(ctg, centers, ref_seq, ref_shift, tensors, batch=ROWTEXT_BATCH, in_hbm=False):
    """the text of the rows as pieces to write one after the other, by the route CV_ROW_FORMAT / ROWTEXT_DEVICE_MIN_ROWS
    choose: one block per `batch` rows from the device, row by row from the host (joining them first costs more than the
    writes it saves); the same bytes either way.  tensors: [k,33,4,4] fp32, a torch tensor (on a GPU for the device route).
    in_hbm: format_rows_device's -- the device route's blocks as tensors on the GPU."""
    if _row_route(len(centers), bool(getattr(tensors, "is_cuda", False))) == "device":
        for block in format_rows_device(ctg, centers, ref_seq, ref_shift, tensors, batch, in_hbm):
            yield block
        return
    for s in range(0, len(centers), batch):                 # the host's loop as it always ran: a row, its newline, nothing joined
        part = tensors[s:s + batch]
        rows = format_rows(ctg, centers[s:s + batch], ref_seq, ref_shift, part.cpu().numpy() if hasattr(part, "cpu") else part)
        _row_counts["host"] += len(rows)
        for row in rows:
            yield row
            yield b"\n"


# ---- ExtractVariantCandidates' rows written on the device (csrc/cv_candrows_dev.hip) ------------------------------------
# CV_CANDIDATE_ROWS=device selects the route; unset or "host" is the host loop (ExtractVariantCandidates.candidate_rows,
# the definition).  The route is opt-in: profiles/r21/candidate_list_device.txt holds what was measured, no floor follows
# from it yet.
CANDROWS_BATCH = 32768          # rows per block of text
CANDROWS_TIMES = None           # the probe: a dict that receives the milliseconds of the device calls by name (HIP events)
_cand_row_counts = {"host": 0, "device": 0}


def candidate_row_counts(reset=False):
    """candidate rows formatted since the start (or the last reset) per side: {"host": n, "device": n}"""
    out = dict(_cand_row_counts)
    if reset:
        _cand_row_counts["host"] = _cand_row_counts["device"] = 0
    return out


def candidate_rows_route():
    """"host" or "device": CV_CANDIDATE_ROWS when it is set (any other value raises), else the host; always "host"
    without a GPU"""
    forced = os.environ.get("CV_CANDIDATE_ROWS")
    if forced not in (None, "", "host", "device"):
        raise ValueError("CV_CANDIDATE_ROWS must be 'host' or 'device', got %r" % forced)
    if forced != "device":
        return "host"
    import torch
    return "device" if torch.cuda.is_available() else "host"


class _CandTimer(object):
    """HIP events around device calls when CANDROWS_TIMES is a dict; read() behind the caller's next synchronisation"""

    def __init__(self, torch, name):
        self.name, self.on = name, CANDROWS_TIMES is not None
        if self.on:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()

    def stop(self):
        if self.on:
            self.b.record()

    def read(self):
        if self.on:
            self.b.synchronize()
            CANDROWS_TIMES[self.name] = CANDROWS_TIMES.get(self.name, 0.0) + self.a.elapsed_time(self.b)


def candidate_order_device(sel):
    """candidate_order on the device: sel = Pileup.selected_device() -> int64 tensor of the entry indices in the
    reference's output order"""
    import torch
    lib = _lib.load()
    pos0, late = sel["pos0"], sel["late"]
    n, dev = int(pos0.numel()), pos0.device
    with torch.cuda.device(dev):
        order = torch.empty(n, dtype=torch.int64, device=dev)
        need = _lib.workspace(lib.cv_candidate_order_workspace, n)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        tm = _CandTimer(torch, "order")
        _lib.check(lib.cv_candidate_order_dev(_lib.ptr(pos0), _lib.ptr(late), n, int(sel["last_pos"]), _lib.ptr(order),
                                              ctypes.c_void_p(ws.data_ptr()), need, _lib.stream_arg(dev)))
        tm.stop()
        torch.cuda.current_stream(dev).synchronize()        # (the workspace may go)
        tm.read()
    return order


def candidate_row_blocks(ctg, sel, ref_seq, ref_shift, host_rows, batch=None):
    """the rows of ExtractVariantCandidates for the entries sel = Pileup.selected_device(), in the reference's order:
    yields, per batch of at most CANDROWS_BATCH rows, ONE block of bytes -- the rows, each followed by "\\n" -- through one
    pinned copy.  ref_seq bytes / str: the loaded reference, ref_seq[0] at 0-based position ref_shift.  A batch with a row
    the device does not vouch for (cv_candidate_rows_dev: status CV_CANDROWS_HOST) is formatted whole by
    host_rows(ctg, res, ref_seq, ref_shift) -> list of str (ExtractVariantCandidates.candidate_rows) from a fetch of just
    that batch's entries; candidate_row_counts() tells which side took what."""
    import torch
    lib = _lib.load()
    batch = int(batch if batch is not None else CANDROWS_BATCH)
    pos0, late, c7 = sel["pos0"], sel["late"], sel["counts"]
    k, dev = int(pos0.numel()), pos0.device
    if k == 0:
        return
    cb = ctg.encode()
    host_ref = ref_seq.encode() if isinstance(ref_seq, str) else bytes(ref_seq)
    with torch.cuda.device(dev):
        order = candidate_order_device(sel)
        ref_dev = torch.frombuffer(bytearray(host_ref) or bytearray(1), dtype=torch.uint8).to(dev)[:len(host_ref)]
        ref_len = int(ref_dev.numel())
        need = _lib.workspace(lib.cv_candidate_rows_workspace, min(batch, k))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        stream = _lib.stream_arg(dev)
        P = _lib.ptr
        for s in range(0, k, batch):
            n = min(batch, k - s)
            off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            status = torch.empty(n, dtype=torch.uint8, device=dev)

            def call(text, cap):
                _lib.check(lib.cv_candidate_rows_dev(cb, len(cb), ctypes.c_void_p(order.data_ptr() + 8 * s), n, k, P(pos0), P(late),
                                                     P(c7), P(ref_dev), int(ref_shift), ref_len, P(off), P(status), text, cap,
                                                     ctypes.c_void_p(ws.data_ptr()), need, stream))
            tm = _CandTimer(torch, "lengths")
            call(None, 0)                                   # lengths and status: the text is sized exactly
            tm.stop()
            total, host_n = (int(v) for v in torch.stack((off[n], status.sum(dtype=torch.int64))).tolist())
            tm.read()
            if host_n:
                idx = order[s:s + n]
                res = {"pos0": pos0[idx].cpu().numpy(), "late": late[idx].cpu().numpy(), "counts": c7[idx].cpu().numpy(),
                       "last_pos": sel["last_pos"]}     # (already in output order: candidate_order leaves it as it is)
                rows = host_rows(ctg, res, host_ref, ref_shift)
                _cand_row_counts["host"] += n
                rows.append("")
                yield "\n".join(rows).encode()
                continue
            text = torch.empty(total, dtype=torch.uint8, device=dev)
            tm = _CandTimer(torch, "rows")
            call(P(text), total)
            tm.stop()
            pin = _pinned_bytes(total)
            pin[:total].copy_(text, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            tm.read()
            _cand_row_counts["device"] += n
            yield pin.numpy()[:total].tobytes()
