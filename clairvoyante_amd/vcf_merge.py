"""The last line of the whole-genome recipe, `vcfcat PREFIX*.vcf | vcfstreamsort | bgziptabix OUT.vcf.gz`: the chunk VCFs
of callVarBamParallel merged into one VCF sorted by contig and position, BGZF-compressed, with a tabix index beside it --
and the reader of such an index.

  merge(files, out_fn, fai_fn, block, threads)   the header of the first file (any other header must equal it byte for
                      byte: ValueError, where vcfcat keeps the first silently), the records of all files ordered by
                      (contig rank, POS, input order), nothing dropped; out_fn through utils_v2.BgzfWriter plus
                      out_fn + ".tbi", or plain text and no index for a name that ends in ".vcf"
  TabixIndex          read() / query() of a .tbi, write_tbi() its writer
  fetch(vcf_fn, ctg, beg, end)   the lines of a 0-based half-open region: only the members the index names are inflated

The host route is the definition: a per-line Python loop for the fields, numpy for the order and the tables.  The device
route (csrc/cv_vcfmerge_dev.hip; CV_VCF_MERGE=device) lays the record bytes of all inputs end to end in HBM, runs the item
line pass, computes the fields, sorts, gathers the sorted text and builds the chunk and window tables there; the text and
the tables cross once and go through the same writer.  A line the device does not vouch for gives the whole call to the
host route, with the same file or the same exception.  Byte parity with htslib's own writer is unpinned (htslib also folds
small bins into their parents, which this writer does not); the reader takes either."""
import glob as _glob
import os
import struct
import zlib

import numpy as np

from . import _lib, utils_v2

MAX_END = 1 << 29                   # the .tbi binning scheme ends here (CSI is not built)
PSEUDO_BIN = 37450
WINDOW_SHIFT = 14
_COUNT_KEYS = ("device_calls", "host_calls", "handed_over_calls", "device_records", "host_records", "fetch_calls",
               "members_inflated")
_counts = dict.fromkeys(_COUNT_KEYS, 0)
TIMES = None                        # the probe: a dict that receives seconds by stage (and HIP-event milliseconds by kernel group)


def counts(reset=False):
    """what ran where so far: calls per route, calls the device route began and gave to the host, records per side; and
    for the reader: fetch() calls and the BGZF members they inflated"""
    out = dict(_counts)
    if reset:
        _counts.update(dict.fromkeys(_COUNT_KEYS, 0))
    return out


def route():
    """"host" or "device": CV_VCF_MERGE (unset: host; anything else raises); always "host" without a GPU"""
    forced = os.environ.get("CV_VCF_MERGE")
    if forced not in (None, "", "host", "device"):
        raise ValueError("CV_VCF_MERGE must be 'host' or 'device', got %r" % forced)
    if forced != "device" or not utils_v2._gpu_present():
        return "host"
    return "device"


# ---- bins -----------------------------------------------------------------------------------------------------------------
def reg2bin(beg, end):
    """the UCSC bin of the 0-based half-open interval [beg, end)"""
    e = end - 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == e >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    """every bin that may hold a record overlapping [beg, end)"""
    e = min(end, MAX_END) - 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (e >> shift) + 1))
    return out


def _reg2bin_np(beg, end):
    e = end - 1
    out = np.zeros(len(beg), dtype=np.int64)
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):      # the finest level that holds wins
        out = np.where(beg >> shift == e >> shift, first + (beg >> shift), out)
    return out


def record_interval(line):
    """-> (contig bytes, POS, beg, end) of one record line (bytes, with or without its newline): beg = POS - 1, end = beg +
    len(REF), or END=n of INFO when n > beg.  ValueError for fewer than 8 columns, POS < 1 and end > 2^29"""
    cols = line.rstrip(b"\n").split(b"\t")
    if len(cols) < 8:
        raise ValueError("a VCF record needs 8 columns, got %d: %r" % (len(cols), line[:80]))
    pos = int(cols[1])
    beg = pos - 1
    end = beg + len(cols[3])
    for kv in cols[7].split(b";"):
        if kv.startswith(b"END="):
            n = int(kv[4:])
            if n > beg:
                end = n
    if beg < 0 or end > MAX_END:
        raise ValueError("%s:%d covers [%d, %d): outside what a .tbi index addresses (1 .. 2^29)"
                         % (cols[0].decode("ascii", "replace"), pos, beg, end))
    return cols[0], pos, beg, end


# ---- reading the inputs ---------------------------------------------------------------------------------------------------
def _read_all(fn):
    """the whole text of a plain, .gz or BGZF file through the project's stream reader"""
    proc, fo = utils_v2._open_tensor_stream(fn)
    parts, done = [], False
    try:
        while True:
            b = fo.read(1 << 24)
            if not b:
                break
            parts.append(b)
        done = True
    finally:
        utils_v2._close_quietly_unless(done, proc, fo, fn)
    return b"".join(parts)


def _header_len(data):
    """bytes of the leading lines that start with '#'"""
    at = 0
    while data[at:at + 1] == b"#":
        k = data.find(b"\n", at)
        at = len(data) if k < 0 else k + 1
    return at


def _contig_names(header, fai_fn):
    """the names that carry a rank, in rank order: the lines of the .fai, else the ##contig=<ID=...> lines of the header"""
    names = []
    if fai_fn is not None:
        with open(fai_fn, "rb") as fh:
            names = [ln.split(b"\t")[0].strip() for ln in fh if ln.strip()]
    else:
        for ln in header.split(b"\n"):
            if ln.startswith(b"##contig=<ID="):
                rest = ln[len(b"##contig=<ID="):]
                cut = min((k for k in (rest.find(b","), rest.find(b">")) if k >= 0), default=len(rest))
                names.append(rest[:cut])
    seen, out = set(), []
    for n in names:
        if n not in seen:
            seen.add(n)
            out.append(n)
    return out


def _inputs(files):
    """-> (header, [record bytes per file]); ValueError for a header that differs from the first file's"""
    header, bodies = None, []
    for fn in files:
        data = _read_all(fn)
        h = _header_len(data)
        if header is None:
            header = data[:h]
        elif data[:h] != header:
            raise ValueError("the header of %s differs from the header of %s" % (fn, files[0]))
        bodies.append(data[h:])
    return header or b"", bodies


# ---- the tables of an index -----------------------------------------------------------------------------------------------
class _Tables(object):
    """what either route hands the writer.  Offsets are UNCOMPRESSED, counted from the first record byte.
      names[r]                          contig of rank r (every rank, with or without records)
      crank, cbin, cubeg, cuend [c]     the chunks, sorted by (rank, bin), in file order within a bin
      win_off[nrank + 1], win[..]       the linear index of rank r = win[win_off[r]:win_off[r + 1]], back-filled
      first, last, count [nrank]        offset of the contig's first record, behind its last, its records"""

    def same(self, o):
        keys = ("crank", "cbin", "cubeg", "cuend", "win_off", "win", "first", "last", "count")
        return self.names == o.names and all(np.array_equal(np.asarray(getattr(self, k), dtype=np.int64),
                                                            np.asarray(getattr(o, k), dtype=np.int64)) for k in keys)


def _host_order(header, bodies, fai_fn):
    """the definition -> (lines in output order, _Tables)"""
    names = _contig_names(header, fai_fn)
    ranks = {n: i for i, n in enumerate(names)}
    lines, rank, pos, beg, end = [], [], [], [], []
    for body in bodies:
        if body and not body.endswith(b"\n"):
            body += b"\n"                                    # a last line without newline gets one
        for ln in _split_nl(body):
            ctg, p, b, e = record_interval(ln)
            r = ranks.get(ctg)
            if r is None:
                r = ranks[ctg] = len(names)                  # a contig nobody named: behind all named ones, as they come
                names.append(ctg)
            lines.append(ln); rank.append(r); pos.append(p); beg.append(b); end.append(e)
    n = len(lines)
    rank, pos = np.array(rank, dtype=np.int64), np.array(pos, dtype=np.int64)
    beg, end = np.array(beg, dtype=np.int64), np.array(end, dtype=np.int64)
    order = np.lexsort((pos, rank)) if n else np.zeros(0, dtype=np.int64)      # stable: ties keep input order
    lines = [lines[i] for i in order.tolist()]
    rank, beg, end = rank[order], beg[order], end[order]
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.fromiter((len(x) for x in lines), dtype=np.int64, count=n), out=off[1:])
    return lines, _tables_of(names, rank, beg, end, off)


def _split_nl(body):
    """the lines of `body`, cut at b"\\n" alone (bytes.splitlines would cut at a '\\r' too)"""
    return [x + b"\n" for x in body[:-1].split(b"\n")] if body else []


def _tables_of(names, rank, beg, end, off):
    """the chunk and window tables of records in output order (rank, beg, end per record; off[n + 1] their offsets)"""
    n, nrank = len(rank), len(names)
    t = _Tables()
    t.names = list(names)
    bins = _reg2bin_np(beg, end)
    head = np.ones(n, dtype=bool)
    if n:
        head[1:] = (rank[1:] != rank[:-1]) | (bins[1:] != bins[:-1])
    first = np.flatnonzero(head)
    last = np.concatenate((first[1:], [n])).astype(np.int64) if n else first
    crank, cbin, cubeg, cuend = rank[first], bins[first], off[first], off[last]
    by_bin = np.lexsort((cbin, crank))                       # stable: the chunks of a bin stay in file order
    t.crank, t.cbin, t.cubeg, t.cuend = crank[by_bin], cbin[by_bin], cubeg[by_bin], cuend[by_bin]
    t.first, t.last, t.count = (np.zeros(nrank, dtype=np.int64) for _ in range(3))
    n_intv = np.zeros(nrank, dtype=np.int64)
    for r in range(nrank):
        lo, hi = np.searchsorted(rank, r, side="left"), np.searchsorted(rank, r, side="right")
        if hi > lo:
            t.first[r], t.last[r], t.count[r] = off[lo], off[hi], hi - lo
            n_intv[r] = ((int(end[lo:hi].max()) - 1) >> WINDOW_SHIFT) + 1
    t.win_off = np.concatenate(([0], np.cumsum(n_intv))).astype(np.int64)
    unset = np.iinfo(np.int64).max
    t.win = np.full(int(t.win_off[-1]), unset, dtype=np.int64)
    for i in range(n):                                       # the smallest offset of a record that overlaps the window
        base = int(t.win_off[rank[i]])
        for w in range(int(beg[i]) >> WINDOW_SHIFT, ((int(end[i]) - 1) >> WINDOW_SHIFT) + 1):
            if off[i] < t.win[base + w]:
                t.win[base + w] = off[i]
    for r in range(nrank):                                   # a window nobody touches takes the next one's value
        for w in range(int(t.win_off[r + 1]) - 2, int(t.win_off[r]) - 1, -1):
            if t.win[w] == unset:
                t.win[w] = t.win[w + 1]
    return t


# ---- writing ----------------------------------------------------------------------------------------------------------------
def _virtual(u, block, member_sizes):
    """uncompressed file offsets -> virtual offsets of a file whose members were cut every `block` bytes"""
    cum = np.concatenate(([0], np.cumsum(np.asarray(member_sizes, dtype=np.int64)))).astype(np.int64)
    u = np.asarray(u, dtype=np.int64)
    return ((cum[u // block] << 16) | (u % block)).astype(np.uint64)


def _bins_bytes(bins):
    """the bins of one contig as the index holds them.  bins: [(bin, [(beg, end), ...])] ascending, or the same as arrays
    (bin numbers [nb], chunks per bin [nb], virtual offsets [nc, 2]) -> (number of bins, bytes)"""
    if not isinstance(bins, tuple):
        ids = np.array([b for b, _c in bins], dtype=np.uint64)
        per = np.array([len(c) for _b, c in bins], dtype=np.uint64)
        pairs = np.array([p for _b, c in bins for p in c], dtype=np.uint64).reshape(-1, 2)
    else:
        ids, per, pairs = (np.asarray(x, dtype=np.uint64) for x in bins)
    nb, nc = len(ids), len(pairs)
    first = np.concatenate(([0], np.cumsum(per)[:-1])).astype(np.int64) if nb else np.zeros(0, dtype=np.int64)
    words = np.zeros(nb + 2 * nc, dtype="<u8")               # per bin: (uint32 bin, int32 n_chunk), then its (beg, end) pairs
    words[np.arange(nb) + 2 * first] = ids | (per << np.uint64(32))
    at = np.repeat(np.arange(nb), per.astype(np.int64)) + 1 + 2 * np.arange(nc)
    words[at] = pairs[:, 0]
    words[at + 1] = pairs[:, 1]
    return nb, words.tobytes()


def write_tbi(fn, names, contigs, threads=None):
    """contigs[i] = (bins, (first, last, count), ioff) of names[i]; bins as _bins_bytes takes them"""
    nm = b"".join(n + b"\0" for n in names)
    out = [b"TBI\1", struct.pack("<8i", len(names), 2, 1, 2, 0, 35, 0, len(nm)), nm]
    for bins, (first, last, count), ioff in contigs:
        nb, raw = _bins_bytes(bins)
        out.append(struct.pack("<i", nb + 1))
        out.append(raw)
        out.append(struct.pack("<Ii4Q", PSEUDO_BIN, 2, first, last, count, 0))
        out.append(struct.pack("<i", len(ioff)))
        out.append(np.asarray(ioff, dtype="<u8").tobytes())
    # (the index is BGZF too; its bytes do not depend on the threads -- nor on CV_BGZF_DEFLATE: zlib writes it)
    with utils_v2.BgzfWriter(fn, threads=threads, deflate="host") as w:
        w.write(b"".join(out))


def _write(out_fn, header, blocks, t, block, threads):
    """header + blocks (the records in order) to out_fn; the index from the tables and the writer's member sizes"""
    import time
    t0 = time.time()
    if out_fn.endswith(".vcf"):
        with open(out_fn, "wb") as fh:
            fh.write(header)
            for b in blocks:
                fh.write(b)
        return
    w = utils_v2.BgzfWriter(out_fn, block=block, threads=threads)
    with w:
        w.write(header)
        for b in blocks:                                    # (a block that is still in HBM: the device writer's)
            w.write_device(b) if hasattr(b, "is_cuda") else w.write(b)
    t1 = time.time()
    H = len(header)
    V = lambda u: _virtual(np.asarray(u, dtype=np.int64) + H, w.block, w.member_sizes)
    cbeg, cend, win = V(t.cubeg), V(t.cuend), V(t.win)
    first, last = V(t.first), V(t.last)
    names, contigs = [], []
    for r in np.flatnonzero(np.asarray(t.count) > 0).tolist():
        lo, hi = np.searchsorted(t.crank, r, side="left"), np.searchsorted(t.crank, r, side="right")
        cb = np.asarray(t.cbin[lo:hi])
        head = np.flatnonzero(np.concatenate(([True], cb[1:] != cb[:-1]))) if hi > lo else np.zeros(0, dtype=np.int64)
        bins = (cb[head], np.diff(np.concatenate((head, [hi - lo]))), np.stack((cbeg[lo:hi], cend[lo:hi]), axis=1))
        names.append(t.names[r])
        contigs.append((bins, (int(first[r]), int(last[r]), int(t.count[r])), win[int(t.win_off[r]):int(t.win_off[r + 1])]))
    write_tbi(out_fn + ".tbi", names, contigs, threads)
    if TIMES is not None:
        TIMES["bgzf_write_s"] = TIMES.get("bgzf_write_s", 0.0) + t1 - t0
        TIMES["tbi_write_s"] = TIMES.get("tbi_write_s", 0.0) + time.time() - t1


def _merge_host(files, out_fn, fai_fn, block, threads, handed_over=False):
    import time
    t0 = time.time()
    _counts["handed_over_calls"] += int(handed_over)       # (counted before the loop runs: it may raise)
    header, bodies = _inputs(files)
    t1 = time.time()
    lines, t = _host_order(header, bodies, fai_fn)
    if TIMES is not None:
        TIMES["read_s"] = TIMES.get("read_s", 0.0) + t1 - t0
        TIMES["order_index_s"] = TIMES.get("order_index_s", 0.0) + time.time() - t1
    _write(out_fn, header, (b"".join(lines[i:i + 4096]) for i in range(0, len(lines), 4096)), t, block, threads)
    _counts["host_calls"] += 1
    _counts["host_records"] += len(lines)
    return {"route": "host", "records": len(lines), "files": len(files), "contigs": int((np.asarray(t.count) > 0).sum())}


def merge(files, out_fn, fai_fn=None, block=None, threads=None, device=None):
    """the records of `files` (VCFs: plain, .gz or BGZF) in one file sorted by (contig rank, POS, input order) -> a dict of
    what was done.  See the module's text."""
    files = list(files)
    if not files:
        raise ValueError("no VCF files to merge")
    if route() == "device":
        try:
            return _merge_device(files, out_fn, fai_fn, block, threads, device)
        except _HandOver:
            return _merge_host(files, out_fn, fai_fn, block, threads, handed_over=True)
    return _merge_host(files, out_fn, fai_fn, block, threads)


# ---- the device route -------------------------------------------------------------------------------------------------------
class _HandOver(Exception):
    """the device route met something only the definition answers: nothing has been written yet"""


def _device_text(rd, torch, device, fn, first_header):
    """the record bytes of one file on the device (plain text memory-mapped, BGZF inflated there, a .gz on the host) ->
    (header bytes, uint8 tensor)"""
    parts = []
    try:
        for kind, piece in utils_v2._truth_chunks(fn, 1 << 28):
            if kind == "bgzf":
                parts.append(rd._inflate(piece, 0)[:piece.n])
            else:
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    parts.append(torch.from_numpy(np.asarray(piece)).to(device))
    except utils_v2._TruthHandOver as e:
        raise _HandOver(str(e))
    if not parts:
        return b"", torch.empty(0, dtype=torch.uint8, device=device)
    text = torch.cat(parts) if len(parts) != 1 else parts[0]
    # the header: leading '#' lines, found on the host in the file's first bytes (read on while it has not ended)
    want = max(len(first_header) + 1, 1 << 16) if first_header is not None else 1 << 16
    while True:
        head = text[:want].cpu().numpy().tobytes()
        h = _header_len(head)
        if h < len(head) or want >= text.numel():
            break
        want *= 4
    return head[:h], text[h:]


class _JoinedBgzf(object):
    """the members of every BGZF file among `files` as ONE slab for utils_v2._TruthReader._inflate (a file of its own per
    call would wait for a kernel that decodes a handful of members): .comp, .table, .n as utils_v2._BgzfSlab has them;
    where[k] = (first inflated byte, byte behind the last, header bytes) of file k, the header inflated on the host"""

    def __init__(self, files):
        self.where, self.slabs, self.first = {}, [], []
        comps, tables, members, self.n = [], [], 0, 0
        at = 0
        for k, fn in enumerate(files):
            got = utils_v2._map_bgzf(fn)
            if got is None or not len(got[1]) or not got[2]:
                continue
            slab = utils_v2._BgzfSlab(got[0], got[1], fn)
            head, j = b"", 0
            while j < len(slab.table):                       # the header: members inflated here until it has ended
                head += slab.inflate_member(j).tobytes()
                j += 1
                if _header_len(head) < len(head):
                    break
            table = slab.table.copy()
            table[:, 0] += at
            table[:, 2] += self.n
            self.where[k] = (self.n, self.n + slab.n, head[:_header_len(head)])
            self.slabs.append(slab); self.first.append(members)
            comps.append(np.asarray(slab.comp)); tables.append(table)
            at += len(slab.comp); self.n += slab.n; members += len(table)
        self.comp = np.concatenate(comps) if comps else np.zeros(0, dtype=np.uint8)
        self.table = np.concatenate(tables) if tables else np.zeros((0, 4), dtype=np.int64)

    def inflate_member(self, i):
        k = int(np.searchsorted(self.first, i, side="right")) - 1
        return self.slabs[k].inflate_member(i - self.first[k])


def _merge_device(files, out_fn, fai_fn, block, threads, device):
    import time
    import torch
    t0 = time.time()
    device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    total = sum(os.path.getsize(f) for f in files)
    with torch.cuda.device(device):
        free, _all = torch.cuda.mem_get_info(device)
        if total * 8 > free // 2:                            # (compressed inputs grow; the arrays take as much again)
            raise _HandOver("the inputs do not fit half of the free device memory")
        rd = utils_v2._TruthReader(device)
        lib, st, P = rd.lib, _lib.stream_arg(device), _lib.ptr
        E = lambda n, dt=torch.int64: torch.empty(n, dtype=dt, device=device)
        header, texts = None, [None] * len(files)
        try:
            joined = _JoinedBgzf(files)                      # every BGZF input: ONE inflate call over the members of all
            inflated = rd._inflate(joined, 0) if joined.n else None
        except (utils_v2._TruthHandOver, _lib.CvError) as e:
            raise _HandOver(str(e))
        for k, fn in enumerate(files):
            if k in joined.where:
                lo, hi, h = joined.where[k]
                body = inflated[lo + len(h):hi]
            else:
                h, body = _device_text(rd, torch, device, fn, header)
            if header is None:
                header = h
            elif h != header:
                raise ValueError("the header of %s differs from the header of %s" % (fn, files[0]))
            texts[k] = body
        ends = [x[-1:] for x in texts if x.numel()]
        if ends and not bool((torch.cat(ends) == 10).all()):
            raise _HandOver("the last line of a file has no newline")
        n_text = sum(int(x.numel()) for x in texts)
        text = E(n_text + 16, torch.uint8)                  # (the gather reads whole 16-byte granules)
        text[n_text:].zero_()
        at = 0
        for x in texts:
            text[at:at + x.numel()].copy_(x)
            at += int(x.numel())
        del texts
        t_read = time.time()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if TIMES is not None else None
        names = _contig_names(header, fai_fn)
        if n_text == 0:
            t = _tables_of(names, *(np.zeros(0, dtype=np.int64) for _ in range(3)), off=np.zeros(1, dtype=np.int64))
            _write(out_fn, header, (), t, block, threads)
            _counts["device_calls"] += 1
            return {"route": "device", "records": 0, "files": len(files), "contigs": 0}
        # 1. the line pass
        max_lines = n_text // 16 + 16                        # (a record has 8 columns: 16 bytes at the least; shorter lines are the host's)
        need = _lib.workspace(lib.cv_item_lines_workspace, n_text, max_lines)
        ws = E(need, torch.uint8)
        pos, run, off, ln = E(max_lines), E(max_lines, torch.int32), E(max_lines), E(max_lines)
        tok, info = E((max_lines, 2)), E(8)
        if ev:
            ev[0].record()
        _lib.check(lib.cv_item_lines_dev(P(text), n_text, max_lines, P(pos), P(run), P(off), P(ln), P(tok), P(info), P(ws), need, st))
        used, lines, rows, _skip, host, runs = info.cpu().tolist()[:6]
        if host or used != n_text or rows != lines or lines >= max_lines:
            raise _HandOver("%d line(s) only the host loop defines the result for" % host)
        n = rows
        ranks = {nm: i for i, nm in enumerate(names)}
        run_rank = []
        for nm in rd.run_names(text, 0, n_text, tok, runs):
            r = ranks.get(nm)
            if r is None:
                r = ranks[nm] = len(names)
                names.append(nm)
            run_rank.append(r)
        nrank = len(names)
        run_rank = torch.from_numpy(np.array(run_rank, dtype=np.int32)).to(device)
        del ws, tok
        # 2.-5. fields, order, sorted text, chunks and per-contig figures
        need = _lib.workspace(lib.cv_vcf_merge_workspace, n)
        ws = E(need, torch.uint8)
        out_text = E(n_text + 16, torch.uint8)
        srank, sbeg, send, ooff = E(n, torch.int32), E(n), E(n), E(n + 1)
        chunks, stats, minfo = E((4, n)), E((4, nrank)), E(8)
        if ev:
            ev[1].record()
        _lib.check(lib.cv_vcf_merge_dev(P(text), n_text, n, P(pos), P(run), P(off), P(ln), P(run_rank), runs, nrank, P(srank), P(sbeg),
                                        P(send), P(ooff), P(out_text), n_text, P(chunks), P(stats), P(minfo), P(ws), need, st))
        host, nchunks, out_bytes = minfo.cpu().tolist()[:3]
        if host:
            raise _HandOver("%d record(s) only the host loop defines the result for (fewer than 8 columns, END= in INFO, "
                            "an end past 2^29)" % host)
        assert out_bytes == n_text
        stats_h = stats.cpu().numpy()
        t = _Tables()
        t.names = names
        t.first, t.last, t.count = stats_h[0], stats_h[1], stats_h[2]
        n_intv = np.where(t.count > 0, ((stats_h[3] - 1) >> WINDOW_SHIFT) + 1, 0)
        t.win_off = np.concatenate(([0], np.cumsum(n_intv))).astype(np.int64)
        nwin = int(t.win_off[-1])
        # 5. the linear index
        win, win_off = E(nwin), torch.from_numpy(t.win_off).to(device)
        if ev:
            ev[2].record()
        _lib.check(lib.cv_vcf_windows_dev(n, P(srank), P(sbeg), P(send), P(ooff), nrank, P(win_off), P(win), nwin, st))
        if ev:
            ev[3].record()
        ch = chunks[:, :nchunks].cpu().numpy()
        t.crank, t.cbin, t.cubeg, t.cuend = ch[0], ch[1], ch[2], ch[3]
        t.win = win.cpu().numpy()
        t_dev = time.time()
        if ev:
            for k, name in enumerate(("lines_ms", "order_gather_chunks_ms", "windows_ms")):
                TIMES[name] = TIMES.get(name, 0.0) + ev[k].elapsed_time(ev[k + 1])
            TIMES["read_s"] = TIMES.get("read_s", 0.0) + t_read - t0
            TIMES["order_index_s"] = TIMES.get("order_index_s", 0.0) + t_dev - t_read

        # 6. the sorted text crosses in pinned slabs, straight into the writer -- or, with the device writer
        # (CV_BGZF_DEFLATE=device), stays where it is: the writer compresses it in HBM and only the file's bytes cross
        in_hbm = not out_fn.endswith(".vcf") and utils_v2.bgzf_deflate_route() == "device"

        def slabs(step=1 << 24):
            if in_hbm:
                for lo in range(0, n_text, step):
                    yield out_text[lo:min(lo + step, n_text)]
                return
            pinned = torch.empty(min(step, max(n_text, 1)), dtype=torch.uint8).pin_memory()
            for lo in range(0, n_text, step):
                k = min(step, n_text - lo)
                pinned[:k].copy_(out_text[lo:lo + k])
                yield pinned[:k].numpy().tobytes()

        _write(out_fn, header, slabs(), t, block, threads)
    _counts["device_calls"] += 1
    _counts["device_records"] += n
    return {"route": "device", "records": n, "files": len(files), "contigs": int((t.count > 0).sum())}


# ---- reading an index -------------------------------------------------------------------------------------------------------
class TabixIndex(object):
    """a .tbi: names, and per contig {bin: [(beg, end)]} (the pseudo-bin apart, in .meta) and the linear index"""

    @classmethod
    def read(cls, fn):
        raw = _read_all(fn)
        if raw[:4] != b"TBI\1":
            raise ValueError("%s is not a tabix index" % fn)
        self = cls()
        n_ref, self.format, self.col_seq, self.col_beg, self.col_end, self.meta, self.skip, l_nm = struct.unpack_from("<8i", raw, 4)
        at = 36
        self.names = raw[at:at + l_nm].split(b"\0")[:n_ref]
        at += l_nm
        self.bins, self.ioff, self.pseudo = [], [], []
        for _ in range(n_ref):
            n_bin, = struct.unpack_from("<i", raw, at)
            at += 4
            bins, meta = {}, None
            for _b in range(n_bin):
                b, n_chunk = struct.unpack_from("<Ii", raw, at)
                at += 8
                pairs = np.frombuffer(raw, dtype="<u8", count=2 * n_chunk, offset=at).reshape(n_chunk, 2)
                at += 16 * n_chunk
                if b == PSEUDO_BIN:
                    meta = pairs
                else:
                    bins[b] = [(int(x), int(y)) for x, y in pairs]
            n_intv, = struct.unpack_from("<i", raw, at)
            at += 4
            self.ioff.append(np.frombuffer(raw, dtype="<u8", count=n_intv, offset=at))
            at += 8 * n_intv
            self.bins.append(bins)
            self.pseudo.append(meta)
        return self

    def query(self, ctg, beg, end):
        """-> [(voff_beg, voff_end)] ascending, merged: where records of `ctg` that overlap [beg, end) can lie"""
        if isinstance(ctg, str):
            ctg = ctg.encode()
        if ctg not in self.names or end <= beg or beg >= MAX_END:
            return []
        r = self.names.index(ctg)
        beg = max(beg, 0)
        ioff = self.ioff[r]
        floor = int(ioff[min(beg >> WINDOW_SHIFT, len(ioff) - 1)]) if len(ioff) else 0
        got = []
        for b in reg2bins(beg, end):
            got.extend(c for c in self.bins[r].get(b, ()) if c[1] > floor)
        got.sort()
        out = []
        for b, e in got:
            if out and b <= out[-1][1]:
                out[-1][1] = max(out[-1][1], e)
            else:
                out.append([b, e])
        return [(b, e) for b, e in out]


def _member_at(fh, at):
    """the BGZF member at file offset `at` -> (its size, its inflated bytes)"""
    fh.seek(at)
    head = fh.read(12)
    if len(head) < 12 or head[:4] != b"\x1f\x8b\x08\x04":
        raise ValueError("no BGZF member at offset %d" % at)
    xlen, = struct.unpack("<H", head[10:12])
    extra = fh.read(xlen)
    k, bsize = 0, None
    while k + 4 <= xlen:
        slen, = struct.unpack_from("<H", extra, k + 2)
        if extra[k:k + 2] == b"BC" and slen == 2:
            bsize = struct.unpack_from("<H", extra, k + 4)[0] + 1
        k += 4 + slen
    if bsize is None:
        raise ValueError("the member at offset %d states no size" % at)
    body = fh.read(bsize - 12 - xlen)
    data = zlib.decompressobj(-15).decompress(body[:-8])
    crc, isize = struct.unpack("<II", body[-8:])
    if len(data) != isize or zlib.crc32(data) != crc:
        raise ValueError("the member at offset %d fails its check" % at)
    _counts["members_inflated"] += 1
    return bsize, data


def fetch(vcf_fn, ctg, beg, end, index=None):
    """yields the record lines (bytes, with newline) of vcf_fn that overlap the 0-based half-open [beg, end) of `ctg`,
    through vcf_fn + ".tbi" (or a TabixIndex given): only the members its chunks name are inflated"""
    if isinstance(ctg, str):
        ctg = ctg.encode()
    idx = index if index is not None else TabixIndex.read(vcf_fn + ".tbi")
    _counts["fetch_calls"] += 1
    chunks = idx.query(ctg, beg, end)
    if not chunks:
        return
    with open(vcf_fn, "rb") as fh:
        have_at, have = None, None
        for vb, ve in chunks:
            co, uo = vb >> 16, vb & 0xffff
            eco, euo = ve >> 16, ve & 0xffff
            parts = []
            while co < eco or (co == eco and uo < euo):
                if have_at != co:
                    have_at, have = co, _member_at(fh, co)
                bsize, data = have
                if co == eco:
                    parts.append(data[uo:euo])
                    break
                parts.append(data[uo:])
                co, uo = co + bsize, 0
            for ln in _split_nl(b"".join(parts)) if parts else ():
                if ln[:1] == b"#" or not ln.startswith(ctg + b"\t"):
                    continue
                _c, _p, b, e = record_interval(ln)
                if b < end and e > beg:
                    yield ln


# ---- command line -----------------------------------------------------------------------------------------------------------
def chunk_files(pattern):
    """the files a glob names, in the shell's (lexicographic) order"""
    return sorted(_glob.glob(pattern))
