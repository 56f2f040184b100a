"""What the reference's dataPrepScripts helpers compute, shared by ChooseItemInBed, CountNumInBed, RandomSampling and
CombineMultipleDatasetsForTraining.

The host loops restate the reference line by line and are the definitions:
  choose_items_host / count_items_host   ChooseItemInBed.py:11-39 and CountNumInBed.py:13-48: the lines of a file whose first
                                         two columns are contig and position that a BED interval covers
  sample_positions_host                  RandomSampling.py:64-68: the positions of a range that the BED covers and a draw
                                         keeps -- with the keyed draws of draws.py (stream RANDOM) in place of the reference's
                                         unseeded generator, so that a kernel can draw them too
  prefix_lines                           CombineMultipleDatasetsForTraining.py:29-44: one byte in front of every line

The device route (csrc/cv_beditems_dev.hip; CV_BED_ITEMS=device) reads the BED as truth_tables does, walks the item file
slab by slab (plain text memory-mapped, BGZF inflated on the device, an ordinary .gz inflated natively on the host),
gives every line a verdict (cv_item_lines_dev), keeps the rows the BED covers and gathers their bytes
(cv_items_keep_dev).  A line only the definition answers (HOST) hands the REST of the file to the host's per-line function
from that slab's first unconsumed line on: what has been written, the counts and the exception raised are the host loop's.
Sampling walks [start, end) in tiles of SAMPLE_TILE positions (cv_sample_positions_dev).

_PairWalk is the device side of PairWithNonVariants (CV_PAIR=device): the same line pass over both tensor files, the
kernels of the training-set builders for the BED test, the truth look-up and the pairing, and cv_items_copy_dev, the gather
above fed with lengths the caller chose.  There a HOST line hands the WHOLE call to the loop, before anything is written."""
import ctypes
import itertools
import os
import shlex
import subprocess

import numpy as np

from . import _lib, draws
from . import utils_v2
from .utils_v2 import _Intervals, _SlabWalk, _TruthHandOver, _TruthReader, _gpu_present, _read_bed_truth, _truth_chunks, _while_table_full

SAMPLE_TILE = 1 << 24               # positions per call of the sampler: its workspace takes 8 bytes per position
SAMPLE_FIRST_CAP = None             # tests: room for kept positions in the first try of every tile (None: from prob)
# The device route is opt-in (CV_BED_ITEMS=device): the standing rule makes it the default from the smallest rung on which
# it is ahead of the host loop in EVERY run of every larger rung.  profiles/r20/dataprep_device.txt
# (tools/gpu_dataprep_probe.py) has it ahead in every run at 16 384 and 65 536 tensor-shaped rows in all three forms and
# on all three sampling ranges, but the 262 144-row and 1 M-row rungs were not run: no floor until they are.  None = no floor.
DEVICE_MIN_BYTES = None
_COUNT_KEYS = ("device_lines", "host_lines", "device_calls", "host_calls", "handed_over_calls", "device_positions")
_counts = dict.fromkeys(_COUNT_KEYS, 0)
TIMES = None                        # the probe: a dict that receives the milliseconds of the device calls by name (HIP events)


def counts(reset=False):
    """lines, calls and sampled positions per side so far; handed_over_calls: calls the device route began and gave to
    the host (host_lines counts only what the device route handed over: the host loop does not count its lines)"""
    out = dict(_counts)
    if reset:
        _counts.update(dict.fromkeys(_COUNT_KEYS, 0))
    return out


def route(input_fn=None):
    """"host" or "device": CV_BED_ITEMS when it is set, else the device from DEVICE_MIN_BYTES of input_fn upwards (no floor
    is set: the host); always "host" without a GPU"""
    forced = os.environ.get("CV_BED_ITEMS")
    if forced not in (None, "", "host", "device"):
        raise ValueError("CV_BED_ITEMS must be 'host' or 'device', got %r" % forced)
    if forced == "host" or not _gpu_present():
        return "host"
    if forced == "device":
        return "device"
    if DEVICE_MIN_BYTES is None or input_fn is None or not os.path.isfile(input_fn):
        return "host"
    return "device" if os.path.getsize(input_fn) >= max(DEVICE_MIN_BYTES, 1) else "host"


# ---- the host loops ---------------------------------------------------------------------------------------------------------
def _gz_byte_lines(fn):
    """the lines of `gzip -fdc fn` as bytes, each with its own line ending (ChooseItemInBed.py:28-29)"""
    f = subprocess.Popen(shlex.split("gzip -fdc %s" % fn), stdout=subprocess.PIPE, bufsize=8388608)
    try:
        for row in f.stdout:
            yield row
    finally:
        f.stdout.close()
        f.wait()


def _lines_of(blocks):
    """byte blocks -> their lines, cut at b"\\n" only (as iterating a binary pipe does), the last one with or without"""
    tail = b""
    for b in blocks:
        data = tail + b if tail else b
        at = 0
        while True:
            k = data.find(b"\n", at)
            if k < 0:
                break
            yield data[at:k + 1]
            at = k + 1
        tail = data[at:]
    if tail:
        yield tail


def bed_tree(bed_fn):
    """contig -> _Intervals: utils_v2._read_bed_truth's reading of a BED file, half-open [int(begin), int(end) - 1), + 1 on
    the end when that equals the begin (ChooseItemInBed.py:13-23).  Blank BED lines follow the project's reader: they are
    skipped, where the reference's row[0] raises IndexError."""
    return _read_bed_truth(None, bed_fn)[0]


def _host_lines(lines, tree, out, tally):
    """the per-line body of both loops (ChooseItemInBed.py:29-36, CountNumInBed.py:35-44) over `lines` (bytes); tally =
    [lines, kept lines], updated as it goes so that an exception leaves what was counted; out: a binary file or None"""
    for row in lines:
        tally[0] += 1
        tok = row.split()
        ctg, pos = tok[0], tok[1]                           # one token: IndexError
        pos = int(pos)                                       # ValueError
        iv = tree.get(ctg.decode("ascii", "replace"))        # (the BED's names were read as ASCII text)
        if iv is None or not iv.hit(pos):                    # a contig the BED lacks drops the line: no KeyError
            continue
        tally[1] += 1
        if out is not None:
            out.write(row)


def choose_items_host(input_fn, bed_fn, out):
    """ChooseItemInBed.Calc: the lines of input_fn whose (contig, position) a BED interval covers, written unchanged (own
    line ending or none) to the binary file `out`.  A line with fewer than two tokens, or a position int() refuses, raises
    IndexError / ValueError after the lines in front of it have been written.  -> (lines, kept lines)"""
    tally = [0, 0]
    _host_lines(_gz_byte_lines(input_fn), bed_tree(bed_fn), out, tally)
    return tuple(tally)


def count_items_host(input_fn, bed_fn):
    """CountNumInBed.Calc -> (total, overlapped)"""
    tally = [0, 0]
    _host_lines(_gz_byte_lines(input_fn), bed_tree(bed_fn), None, tally)
    return tuple(tally)


def _table_of(intervals):
    iv = _Intervals()
    for b, e in intervals:
        iv.addi(b, e)
    return iv.table()


def sample_positions_host(ctg, start, end, prob, intervals, seed):
    """RandomSampling.py:64-68 -> the positions i of range(start, end) (end exclusive) that lie in one of `intervals`
    (half-open (begin, end) pairs; None: there is no BED) and whose draw u(i) = draws.draws(seed, draws.RANDOM, ctg, i)
    is <= prob, ascending, int64.  Computed over tiles of SAMPLE_TILE positions."""
    out = []
    b, emax = _table_of(intervals) if intervals is not None else (None, None)
    tile = max(int(SAMPLE_TILE), 1)
    for first in range(start, end, tile):
        pos = np.arange(first, min(first + tile, end), dtype=np.int64)
        if intervals is not None:
            if not len(b):
                break
            k = np.searchsorted(b, pos, side="right")        # _Intervals.hit over the tile
            pos = pos[(k > 0) & (emax[np.maximum(k - 1, 0)] > pos)]
        out.append(pos[draws.draws(seed, draws.RANDOM, ctg, pos) <= prob])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def prefix_lines(block, prefix, at_line_start):
    """`block` (bytes, a piece of a file) with the byte `prefix` put in front of every line that starts inside it ->
    (bytes, "the next piece starts a line")"""
    a = np.frombuffer(block, dtype=np.uint8)
    if not len(a):
        return b"", at_line_start
    starts = np.flatnonzero(a[:-1] == 10) + 1
    if at_line_start:
        starts = np.concatenate((np.zeros(1, dtype=starts.dtype), starts))
    return np.insert(a, starts, prefix).tobytes(), bool(a[-1] == 10)


# ---- the device route -------------------------------------------------------------------------------------------------------
class _Timer(object):
    """HIP events around a device call when TIMES is a dict; read after the caller's next synchronisation"""

    def __init__(self, torch, name):
        self.name, self.on = name, TIMES is not None
        if self.on:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.on:
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.b.record()

    def read(self):
        if self.on:
            self.b.synchronize()
            TIMES[self.name] = TIMES.get(self.name, 0.0) + self.a.elapsed_time(self.b)


class _RestToHost(Exception):
    """a slab holds a line only the definition answers: at = offset in the buffer of the first unconsumed line"""

    def __init__(self, at, reason):
        Exception.__init__(self, reason)
        self.at = at


class _ItemWalk(object):
    """the device side of choose / count: the BED tables, then the item file slab by slab"""

    def __init__(self, device, bed_fn, out):
        import torch
        self.torch, self.device, self.out = torch, device, out
        self.rd = _TruthReader(device)
        self.lib, self.st = self.rd.lib, _lib.stream_arg(device)
        self.total = self.kept = 0
        self.bytes_per_line = 16.0                           # sizes the line table: the slab before says what to expect
        self.pinned = None
        self.E = lambda n, dt=torch.int64: torch.empty(n, dtype=dt, device=device)
        self.bed_off, self.bed_begin, self.bed_emax, _nb, self.nctg = self.rd.bed_table(bed_fn)
        torch.cuda.current_stream(device).synchronize()       # (the workspace and the rows may go)

    def slab(self, buf, lo, hi, padded_end):
        """the two passes over buf[lo:hi], again while the line table is full -> bytes consumed.  padded_end: the offset
        behind a newline the walk appended to the file's last line (None: there is none): that byte is not written"""
        torch, lib, P, E = self.torch, self.lib, _lib.ptr, self.E
        want_text = 1 if self.out is not None else 0

        def line_pass(at, n, max_lines):
            text_ptr = ctypes.c_void_p(buf.data_ptr() + at)
            need = _lib.workspace(lib.cv_item_lines_workspace, n, max_lines)
            ws = E(need, torch.uint8)
            pos, run, off, ln = E(max_lines), E(max_lines, torch.int32), E(max_lines), E(max_lines)
            tok, info_dev = E((max_lines, 2)), E(8)
            with _Timer(torch, "lines") as tm:
                _lib.check(lib.cv_item_lines_dev(text_ptr, n, max_lines, P(pos), P(run), P(off), P(ln), P(tok), P(info_dev), P(ws),
                                                 need, self.st))
            used, lines, rows, _skipped, host, runs = info_dev.cpu().tolist()[:6]
            tm.read()
            if host:
                raise _RestToHost(at, "%d line(s) only the host loop defines the result for (a blank line, fewer than two tokens, "
                                      "a position that is not canonical decimal, '\\r', bytes outside printable ASCII, ...)" % host)
            if rows:
                # the BED contig id of each run from its start token, -1 for a contig the BED lacks
                ids = [self.rd.ids.get(name, -1) for name in self.rd.run_names(buf, at, n, tok, runs)]
                run_ctg = torch.from_numpy(np.array(ids, dtype=np.int32)).to(self.device)
                need = _lib.workspace(lib.cv_items_keep_workspace, rows)
                ws = E(need, torch.uint8)
                text_out = E(used, torch.uint8) if want_text else None
                cnt = E(4)
                with _Timer(torch, "keep") as tm:
                    _lib.check(lib.cv_items_keep_dev(text_ptr, n, rows, P(pos), P(run), P(off), P(ln), P(run_ctg), runs, self.nctg,
                                                     P(self.bed_off), P(self.bed_begin), P(self.bed_emax), want_text, P(text_out),
                                                     used if want_text else 0, P(cnt), P(ws), need, self.st))
                    last = None
                    if want_text and padded_end is not None and at + used == padded_end:
                        # is the file's last line kept?  Then the newline the walk gave it stays behind
                        last = E(4)
                        _lib.check(lib.cv_items_keep_dev(text_ptr, n, 1, P(pos[rows - 1:]), P(run[rows - 1:]), P(off[rows - 1:]),
                                                         P(ln[rows - 1:]), P(run_ctg), runs, self.nctg, P(self.bed_off),
                                                         P(self.bed_begin), P(self.bed_emax), 0, None, 0, P(last), P(ws), need,
                                                         self.st))
                _rows, kept, nbytes, _zero = cnt.cpu().tolist()
                tm.read()
                if last is not None and last.cpu().tolist()[1]:
                    nbytes -= 1
                if want_text and nbytes:
                    if self.pinned is None or self.pinned.numel() < nbytes:
                        self.pinned = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8).pin_memory()
                    self.pinned[:nbytes].copy_(text_out[:nbytes])
                    self.out.write(self.pinned[:nbytes].numpy().tobytes())
                self.kept += kept
            self.total += lines
            _counts["device_lines"] += lines
            if lines:
                self.bytes_per_line = max(used / float(lines), 2.0)
            return used, lines

        return _while_table_full(lo, hi, lambda n: min(int(n / self.bytes_per_line * 1.25) + 1024, n), line_pass)

    def walk(self, input_fn):
        """every slab of the file; _RestToHost / _TruthHandOver with .blocks = the bytes the host continues over"""
        slab_bytes = max(int(utils_v2.TRUTH_SLAB_BYTES), 1)
        walk = _SlabWalk(self.torch, self.device, _truth_chunks(input_fn, slab_bytes), slab_bytes, self.rd._inflate,
                         pad_always=False, join_unbroken=True, whole_lines=True, keep_open=(_RestToHost, _TruthHandOver))
        try:
            walk.run(self.slab)
        except _RestToHost as e:
            rest, chunks = walk.rest(e.at)
            e.blocks = itertools.chain([rest], _host_blocks(chunks))
            raise


# ---- PairWithNonVariants on the device: existing kernels composed (PairWithNonVariants.Pair chooses the route) -------------
PAIR_RESIDENT_BYTES = None          # tests: text of one file that may stay in HBM between the two passes (None: half of what is free)
_KEY_BITS = 40                      # a position of at most 12 digits is below 2^40: (contig id << 40 | position) is one int64


class _PairFile(object):
    """what the counting pass keeps of one tensor file: per row the contig id and the position (and, for candidates, the
    usable flag); per line pass a unit (rows, bytes, buffer, offsets, lengths) -- buffer, offsets and lengths only while
    the file's text stays resident"""

    def __init__(self, fn, room):
        self.fn, self.room = fn, room
        self.ctg, self.pos, self.usable, self.units = [], [], [], []
        self.rows = self.held = 0
        self.resident, self.cur = True, None

    def saw(self, buf):
        """a new buffer of the walk: does the file's text still fit?"""
        if buf is not self.cur:
            self.cur = buf
            self.held += int(buf.numel())
            if self.resident and self.held > self.room:
                self.resident = False
                self.units = [(rows, used, None, None, None) for rows, used, _b, _o, _l in self.units]

    def column(self, torch, parts, dtype, device):
        return torch.cat(parts) if parts else torch.empty(0, dtype=dtype, device=device)


class _PairWalk(object):
    """The device side of PairWithNonVariants.Pair.  Nothing here is a kernel of its own: the BED through
    _TruthReader.bed_table, both tensor files slab by slab through cv_item_lines_dev, the BED test and the truth look-up
    of the candidates through cv_trainset_join, ONE cv_bamtrain_pair over the rows of both files, the written lines
    through cv_items_copy_dev; torch for the glue (the truth keys sorted and made unique, the edge bytes of every line).
    _TruthHandOver wherever only the loop answers: every verdict is known before the first byte is written, so the WHOLE
    call is Pair_host's then."""

    def __init__(self, device, bed_fn):
        import torch
        self.torch, self.device = torch, device
        self.rd = _TruthReader(device)
        self.lib, self.st = self.rd.lib, _lib.stream_arg(device)
        self.E = lambda n, dt=torch.int64: torch.empty(n, dtype=dt, device=device)
        self.has_bed = bed_fn is not None
        self.bed_lines = 0
        if self.has_bed:
            self.bed_off, self.bed_begin, self.bed_emax, self.bed_lines, _nctg = self.rd.bed_table(bed_fn)     # (its intervals)
            torch.cuda.current_stream(device).synchronize()   # (the workspace and the rows may go)
        self.var = self.can = None

    # -- one line pass, for both passes over a file
    def _lines(self, buf, at, n, max_lines):
        """cv_item_lines_dev over buf[at:at + n] -> (used, lines, rows, runs, pos, run, offsets into buf, lengths, tok)"""
        torch, lib, P, E = self.torch, self.lib, _lib.ptr, self.E
        need = _lib.workspace(lib.cv_item_lines_workspace, n, max_lines)
        ws = E(need, torch.uint8)
        pos, run, off, ln = E(max_lines), E(max_lines, torch.int32), E(max_lines), E(max_lines)
        tok, info_dev = E((max_lines, 2)), E(8)
        with _Timer(torch, "pair_lines") as tm:
            _lib.check(lib.cv_item_lines_dev(ctypes.c_void_p(buf.data_ptr() + at), n, max_lines, P(pos), P(run), P(off), P(ln), P(tok),
                                             P(info_dev), P(ws), need, self.st))
        used, lines, rows, _skipped, host, runs = info_dev.cpu().tolist()[:6]
        tm.read()
        if host:
            raise _TruthHandOver("%d line(s) only the host loop defines the result for (a blank line, fewer than two tokens, a "
                                 "position that is not canonical decimal, '\\r', bytes outside printable ASCII, ...)" % host)
        return used, lines, rows, runs, pos[:rows], run[:rows], off[:rows] + at, ln[:rows].clone(), tok

    def _walk(self, f, line_pass):
        slab_bytes = max(int(utils_v2.TRUTH_SLAB_BYTES), 1)
        state = {"bytes_per_line": 16.0}                     # (both passes over a file start alike: they cut the same units)

        def slab(buf, lo, hi, _padded_end):                  # (the newline the walk gives the last line is written, as strip() + "\n" is)
            def one(at, n, max_lines):
                used, lines = line_pass(buf, at, n, max_lines)
                if lines:
                    state["bytes_per_line"] = max(used / float(lines), 2.0)
                return used, lines
            return _while_table_full(lo, hi, lambda n: min(int(n / state["bytes_per_line"] * 1.25) + 1024, n), one)

        _SlabWalk(self.torch, self.device, _truth_chunks(f.fn, slab_bytes), slab_bytes, self.rd._inflate, pad_always=False,
                  join_unbroken=True, whole_lines=True).run(slab)

    def _count(self, fn, on_rows):
        """the counting pass over one file: on_rows(f, rows, pos, run, run_ctg, runs) per line pass with rows"""
        torch = self.torch
        room = PAIR_RESIDENT_BYTES
        if room is None:
            room = torch.cuda.mem_get_info(self.device)[0] // 2
        f = _PairFile(fn, room)

        def line_pass(buf, at, n, max_lines):
            used, lines, rows, runs, pos, run, off, ln, tok = self._lines(buf, at, n, max_lines)
            f.saw(buf)
            if rows:
                # the device writes a line's raw bytes: they are strip() + "\n" only without a blank at either edge
                edge = buf[torch.cat((off, off + ln - 2))]
                if bool(((edge == 32) | (edge == 9)).any()):
                    raise _TruthHandOver("a line with white space at either edge: the host loop strips it")
                ids = [self.rd.contigs.id_of(name) for name in self.rd.run_names(buf, at, n, tok, runs)]
                run_ctg = torch.from_numpy(np.array(ids, dtype=np.int32)).to(self.device)
                on_rows(f, rows, pos, run, run_ctg, runs)
                f.pos.append(pos.clone())
                f.units.append((rows, used, buf, off, ln) if f.resident else (rows, used, None, None, None))
                f.rows += rows
            return used, lines

        self._walk(f, line_pass)
        torch.cuda.current_stream(self.device).synchronize()
        f.ctg = f.column(torch, f.ctg, torch.int32, self.device)
        f.pos = f.column(torch, f.pos, torch.int64, self.device)
        return f

    def count_variants(self, fn):
        """v, and the truth keys of all contigs as the tables cv_trainset_join reads (a duplicate row counts in v, once here)"""
        torch = self.torch
        self.var = f = self._count(fn, lambda f, rows, pos, run, run_ctg, runs: f.ctg.append(run_ctg[run.long()]))
        self.ntab = ntab = len(self.rd.names)
        keys = torch.unique((f.ctg.to(torch.int64) << _KEY_BITS) | f.pos)
        self.truth_pos = keys & ((1 << _KEY_BITS) - 1)
        self.truth_off = torch.searchsorted(keys, torch.arange(ntab + 1, dtype=torch.int64, device=self.device) << _KEY_BITS)
        # a contig the truth file brought has no BED interval: an empty table, so the BED test drops it as the loop does
        off = self.bed_off if self.has_bed else torch.zeros(1, dtype=torch.int64, device=self.device)
        self.tab_off = torch.cat((off, off[-1:].expand(ntab + 1 - int(off.numel())))) if off.numel() < ntab + 1 else off
        one = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.tab_begin = self.bed_begin if self.has_bed and self.bed_begin.numel() else one
        self.tab_emax = self.bed_emax if self.has_bed and self.bed_emax.numel() else one
        return f.rows

    def count_candidates(self, fn):
        """per candidate row the contig id and usable = the BED keeps it (when there is one) and no truth row has its key"""
        torch, lib, P, E = self.torch, self.lib, _lib.ptr, self.E

        def on_rows(f, rows, pos, run, run_ctg, runs):
            ctg, keep, truth = E(rows, torch.int32), E(rows, torch.uint8), E(rows, torch.int32)
            with _Timer(torch, "pair_join") as tm:
                _lib.check(lib.cv_trainset_join(rows, P(run), P(run_ctg), runs, P(pos), self.ntab, 1 if self.has_bed else 0,
                                                P(self.tab_off), P(self.tab_begin), P(self.tab_emax),
                                                P(self.truth_off) if self.truth_pos.numel() else None, P(self.truth_pos),
                                                P(ctg), P(keep), P(truth), self.st))
            f.ctg.append(ctg)
            f.usable.append(keep & (truth < 0).to(torch.uint8))
            tm.read()

        self.can = f = self._count(fn, on_rows)
        f.usable = f.column(torch, f.usable, torch.uint8, self.device)
        return f.rows

    def pair(self, seed, amp):
        """one cv_bamtrain_pair over the variant rows (truth centres, kept) and the candidate rows (keep = usable)
        -> (v, c, r, picked); the candidates' verdicts stay in self.keep"""
        torch, P = self.torch, _lib.ptr
        v, n = self.var.rows, self.var.rows + self.can.rows
        self.keep = torch.cat((torch.ones(v, dtype=torch.uint8, device=self.device), self.can.usable))
        if n == 0:
            return 0, 0, 1.0, 0
        flags = torch.zeros(n, dtype=torch.uint8, device=self.device)
        flags[:v] = 1                                        # CV_CENTRE_TRUTH
        acgt = torch.ones(n, dtype=torch.uint8, device=self.device)
        ctg, pos = torch.cat((self.var.ctg, self.can.ctg)), torch.cat((self.var.pos, self.can.pos))
        h = np.array([draws.fnv1a32(nm) for nm in self.rd.names], dtype=np.uint32).view(np.int32)
        h_dev = torch.from_numpy(h).to(self.device)
        counts, r = torch.zeros(4, dtype=torch.int64, device=self.device), torch.zeros(1, dtype=torch.float64, device=self.device)
        with _Timer(torch, "pair_draw") as tm:
            _lib.check(self.lib.cv_bamtrain_pair(n, P(ctg), P(pos), P(flags), P(acgt), P(h_dev), len(self.rd.names), int(seed), float(amp),
                                                 P(self.keep), P(counts), P(r), self.st))
        got_v, c, picked, kept = counts.cpu().tolist()
        tm.read()
        if got_v != v or kept != v + picked:
            raise _lib.CvError("cv_bamtrain_pair: %d truth rows and %d kept rows where %d and %d were expected" % (got_v, kept, v, v + picked))
        return v, c, float(r.item()), picked

    def gather(self, f, keep, write):
        """the kept lines of one file in file order through cv_items_copy_dev, unit by unit -> lines written.  keep: the
        file's rows' verdicts (uint8); write(tensor of bytes in HBM).  A file whose text did not stay resident is walked again."""
        torch, lib, P, E = self.torch, self.lib, _lib.ptr, self.E
        done = {"unit": 0, "row": 0, "lines": 0}

        def unit(buf, off, ln, rows, used):
            k = keep[done["row"]:done["row"] + rows]
            kept_len = ln * k
            need = _lib.workspace(lib.cv_items_copy_workspace, rows)
            ws, out, cnt = E(need, torch.uint8), E(used, torch.uint8), E(4)
            with _Timer(torch, "pair_copy") as tm:
                _lib.check(lib.cv_items_copy_dev(P(buf), int(buf.numel()), rows, P(off), P(kept_len), P(out), used, P(cnt), P(ws), need,
                                                 self.st))
            nbytes, lines = cnt.cpu().tolist()[2], int(k.sum())
            tm.read()
            if nbytes > used:
                raise _lib.CvError("cv_items_copy_dev: %d bytes kept of a unit of %d" % (nbytes, used))
            if nbytes:
                write(out[:nbytes])
            done["unit"] += 1; done["row"] += rows; done["lines"] += lines

        if f.resident:
            for rows, used, buf, off, ln in f.units:
                unit(buf, off, ln, rows, used)
        else:
            def line_pass(buf, at, n, max_lines):
                used, lines, rows, _runs, _pos, _run, off, ln, _tok = self._lines(buf, at, n, max_lines)
                if rows:
                    if done["unit"] >= len(f.units) or f.units[done["unit"]][:2] != (rows, used):
                        raise _lib.CvError("%s changed between the two passes of PairWithNonVariants" % f.fn)
                    unit(buf, off, ln, rows, used)
                return used, lines
            self._walk(f, line_pass)
        if done["row"] != f.rows:
            raise _lib.CvError("%s changed between the two passes of PairWithNonVariants" % f.fn)
        return done["lines"]


def _host_blocks(chunks):
    """what is left of _truth_chunks as bytes on the host (a stream that breaks off ends there, as the pipe of `gzip -fdc` does)"""
    try:
        for kind, piece in chunks:
            if kind is None:
                return
            if kind == "host":
                yield np.asarray(piece).tobytes()
            else:
                for i in range(len(piece.table)):
                    yield piece.inflate_member(i).tobytes()
    except (_TruthHandOver, _lib.CvError):
        return


def _items_host(input_fn, bed_fn, out, handed_over=False):
    _counts["handed_over_calls"] += int(handed_over)
    _counts["host_calls"] += 1
    return choose_items_host(input_fn, bed_fn, out) if out is not None else count_items_host(input_fn, bed_fn)


def _items(input_fn, bed_fn, out, device=None):
    """choose (out: a binary file) or count (out: None) by route() -> (lines, kept lines).  (The device route reads the BED
    through utils_v2._TruthReader, whose lines count in utils_v2.truth_table_counts() as well.)"""
    if route(input_fn) != "device":
        return _items_host(input_fn, bed_fn, out)
    import torch
    device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    with torch.cuda.device(device):
        try:
            walk = _ItemWalk(device, bed_fn, out)
        except _TruthHandOver:                               # the BED: nothing has been written, the whole call is the host's
            return _items_host(input_fn, bed_fn, out, handed_over=True)
        try:
            walk.walk(input_fn)
        except _TruthHandOver:
            # the item file is nothing the native readers take: the host's pipe reads it.  (A stream that breaks off
            # LATER ends the device's walk where the pipe of `gzip -fdc` ends too: what was consumed stays.)
            if walk.total == 0:
                return _items_host(input_fn, bed_fn, out, handed_over=True)
        except _RestToHost as e:
            _counts["handed_over_calls"] += 1
            tally = [0, 0]
            try:
                _host_lines(_lines_of(e.blocks), bed_tree(bed_fn), out, tally)
            finally:
                _counts["host_lines"] += tally[0]
            return walk.total + tally[0], walk.kept + tally[1]
    _counts["device_calls"] += 1
    return walk.total, walk.kept


def choose_items(input_fn, bed_fn, out, device=None):
    """ChooseItemInBed by route(): choose_items_host, or the device route with the same bytes, counts and exceptions"""
    return _items(input_fn, bed_fn, out, device)


def count_items(input_fn, bed_fn, device=None):
    """CountNumInBed by route() -> (total, overlapped)"""
    return _items(input_fn, bed_fn, None, device)


def sample_positions_device(ctg, start, end, prob, intervals, seed, device=None):
    """sample_positions_host on the device: the contig's table uploaded once, [start, end) walked in tiles of SAMPLE_TILE"""
    import torch
    if end <= start or (intervals is not None and not len(intervals)):
        return np.zeros(0, dtype=np.int64)
    device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    lib = _lib.load()
    P = _lib.ptr
    out = []
    with torch.cuda.device(device):
        st = _lib.stream_arg(device)
        nbed, b_dev, e_dev = 0, None, None
        if intervals is not None:
            b, emax = _table_of(intervals)
            nbed, b_dev, e_dev = len(b), torch.from_numpy(b).to(device), torch.from_numpy(emax).to(device)
        tile = max(int(SAMPLE_TILE), 1)
        need = _lib.workspace(lib.cv_sample_positions_workspace, min(tile, end - start))
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        cnt = torch.empty(2, dtype=torch.int64, device=device)
        h = draws.fnv1a32(ctg)
        for first in range(start, end, tile):
            count = min(tile, end - first)
            cap = SAMPLE_FIRST_CAP if SAMPLE_FIRST_CAP is not None else int(count * min(max(prob, 0.0), 1.0) * 1.05) + 4096
            while True:
                cap = max(min(cap, count), 1)
                pos = torch.empty(cap, dtype=torch.int64, device=device)
                with _Timer(torch, "sample") as tm:
                    _lib.check(lib.cv_sample_positions_dev(int(seed), h, first, count, float(prob), nbed, P(b_dev), P(e_dev), P(pos), cap,
                                                           P(cnt), P(ws), need, st))
                wrote, would = cnt.cpu().tolist()
                tm.read()
                if wrote == would:
                    break
                cap = would                                  # the room was too small: the tile again
            _counts["device_positions"] += count
            out.append(pos[:wrote].cpu().numpy())
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def sample_positions(ctg, start, end, prob, intervals, seed, device=None):
    """the sampled positions by route() (RandomSampling obeys CV_BED_ITEMS too)"""
    if route() == "device":
        got = sample_positions_device(ctg, start, end, prob, intervals, seed, device)
        _counts["device_calls"] += 1
        return got
    _counts["host_calls"] += 1
    return sample_positions_host(ctg, start, end, prob, intervals, seed)
