"""Shared by tests/test_pileup_tiles_host.py (CPU) and tests/test_gpu_pileup_tiles.py (GPU): which of the two code paths
of the column kernels of csrc/cv_pileup.hip an input reaches, and the long-read / sparse inputs that reach the second.

Both kernels give a workgroup a TILE of 512 consecutive segments of one uploaded batch and keep a window of counters in
LDS: evc_count the EVC_WIN positions from (POS of the tile's first segment) - 1 on, pileup_scatter the SC_CANDS centres at
or after (POS of the tile's first segment) - 16.  A column whose counter is not in the window goes to HBM with an atomic
of its own.  The restatement below is written from cv_pileup.hip's header comment, `emit`, `parse_record`,
`absorb_parts` and the index arithmetic of the two kernels, in the style of bam_device_cases.py_parse: it computes no
count, only WHERE the kernels book one."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, ".."))

SC_SEGS, SC_CANDS, EVC_SEGS, EVC_WIN = 512, 40, 512, 1536
SEG_MAX, FLANK = 64, 16
T_MATCH, T_INS, T_DEL = 0, 1, 2
_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")


def source_constants():
    """the four `constexpr int` of csrc/cv_pileup.hip the helper restates"""
    src = open(os.path.join(HERE, "..", "clairvoyante_amd", "csrc", "cv_pileup.hip")).read()
    out = {}
    for name in ("SC_SEGS", "SC_CANDS", "EVC_SEGS", "EVC_WIN"):
        m = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


def segments(lines, minMQ=0, dcov=250, evc=True, evc_minMQ=0, contig="ctgA"):
    """the segment list ONE batch of these SAM lines makes, in read order -> dict of int64 arrays, one entry per
    segment: type, r0, n (columns), first (first piece of its run), pos (the read's 0-based POS), ct / evc (which pass
    takes the read; the depth cap of the tensor pass applied), q0 (offset into `seq`), and `seq`, the SEQ bytes."""
    typ, r0, n, first, pos_, ct_, evc_, q0 = [], [], [], [], [], [], [], []
    seq = bytearray()
    prev_pos, cap = 0, 0
    for line in lines:
        f = line.split()
        if not f or f[0].startswith("@"):
            continue
        pos, mq = int(f[3]) - 1, int(f[4])
        runs = [(int(v), op) for v, op in _CIGAR.findall(f[5])]
        need = sum(v for v, op in runs if op in "MIS=X")
        total = sum(v for v, _ in runs)
        clipped = sum(v for v, op in runs if op == "S")
        ct_ok = mq >= minMQ
        evc_ok = bool(evc) and mq >= evc_minMQ and (contig is None or f[2] == contig)
        if evc_ok and 1.0 - float(clipped) / float(total + 1) < 0.55:
            evc_ok = False
        if not ct_ok and not evc_ok:
            continue                                        # the record makes no segment at all
        if ct_ok:                                           # absorb_parts: at most dcov reads of one POS
            if prev_pos != pos:
                prev_pos, cap = pos, 0
            else:
                cap += 1
                ct_ok = cap < dcov
        base = len(seq)
        s = f[9].encode()
        seq += s + b"?" * max(need - len(s), 0)
        r, q = pos, 0
        for v, op in runs:
            if op == "S":
                q += v
                continue
            if op in "NHP":
                continue                                    # nothing moves
            t = T_MATCH if op in "M=X" else T_INS if op == "I" else T_DEL
            done = 0
            while done < v:
                ln = min(v - done, SEG_MAX)
                typ.append(t); n.append(ln); first.append(done == 0); pos_.append(pos); ct_.append(ct_ok); evc_.append(evc_ok)
                r0.append(r if t == T_INS else r + done)
                q0.append(0 if t == T_DEL else base + q + done)
                done += ln
            if t != T_INS:
                r += v
            if t != T_DEL:
                q += v
    a = lambda x, d=np.int64: np.asarray(x, dtype=d)
    return {"type": a(typ), "r0": a(r0), "n": a(n), "first": a(first, bool), "pos": a(pos_), "ct": a(ct_, bool),
            "evc": a(evc_, bool), "q0": a(q0), "seq": np.frombuffer(bytes(seq), dtype=np.uint8)}


def _columns(sg, keep):
    """per alignment column of the kept segments: (segment index, lane)"""
    idx = np.nonzero(keep)[0]
    seg = np.repeat(idx, sg["n"][idx])
    start = np.repeat(np.cumsum(sg["n"][idx]) - sg["n"][idx], sg["n"][idx])
    return seg, np.arange(len(seg), dtype=np.int64) - start


def evc_paths(sg, ref_first=None, ref_len=None):
    """evc_count: a match column books at r0 + lane when its SEQ byte is one of ACGTN, an insertion / deletion run once,
    at r0 - 1 of its first piece.  -> dict(inside, outside: bookings whose position is inside / outside
    [base, base + EVC_WIN) of their tile, base = POS of the tile's first segment - 1; tiles; and, with a reference slice,
    outside_off_slice: the outside bookings the `ri` test must drop)"""
    m = sg["evc"] & (sg["type"] == T_MATCH)
    seg, lane = _columns(sg, m)
    ch = sg["seq"][sg["q0"][seg] + lane]
    ok = np.isin(ch, np.frombuffer(b"ACGTN", dtype=np.uint8))
    seg, r = seg[ok], (sg["r0"][seg] + lane)[ok]
    run = np.nonzero(sg["evc"] & (sg["type"] != T_MATCH) & sg["first"])[0]
    seg = np.concatenate([seg, run])
    r = np.concatenate([r, sg["r0"][run] - 1])
    base = sg["pos"][(seg // EVC_SEGS) * EVC_SEGS] - 1
    off = r - base
    out = (off < 0) | (off >= EVC_WIN)
    res = {"inside": int((~out).sum()), "outside": int(out.sum()), "tiles": int((len(sg["n"]) + EVC_SEGS - 1) // EVC_SEGS)}
    if ref_first is not None:
        ri = r - ref_first
        res["outside_off_slice"] = int((out & ((ri < 0) | (ri >= ref_len))).sum())
        res["inside_off_slice"] = int((~out & ((ri < 0) | (ri >= ref_len))).sum())
    return res


def scatter_paths(sg, centers, left=True):
    """pileup_scatter: the (column, centre) pairs the local rule of the header comment lets through (the tests of the
    reference base and the query base aside), split by whether the centre's index lies in [i0, i0 + SC_CANDS) of the
    column's tile, i0 = the first centre >= POS of the tile's first segment - FLANK.  -> dict(inside, outside, tiles)"""
    c = np.asarray(centers, dtype=np.int64)
    seg, lane = _columns(sg, sg["ct"])
    t = sg["type"][seg]
    r = np.where(t == T_INS, sg["r0"][seg], sg["r0"][seg] + lane)
    pos = sg["pos"][seg]
    # 0 <= p <= 32 (match) or 1 <= p <= 32 (insert, delete; and r > POS) with p = r - c + 17
    lo_c = r - (FLANK - 1)
    hi_c = np.where(t == T_MATCH, r + FLANK + 1, r + FLANK)
    if not left:
        lo_c = np.maximum(lo_c, pos + FLANK + 1)
    live = (t == T_MATCH) | (r > pos)
    lo = np.searchsorted(c, lo_c, "left")
    hi = np.maximum(np.searchsorted(c, hi_c, "right"), lo)
    lo, hi = lo[live], hi[live]
    i0 = np.searchsorted(c, sg["pos"][(seg // SC_SEGS) * SC_SEGS] - FLANK, "left")[live]
    pairs = hi - lo
    inside = np.maximum(np.minimum(hi, i0 + SC_CANDS) - np.maximum(lo, i0), 0)
    return {"inside": int(inside.sum()), "outside": int((pairs - inside).sum()),
            "tiles": int((len(sg["n"]) + SC_SEGS - 1) // SC_SEGS)}


# ---- the inputs -------------------------------------------------------------------------------------------------------
G = os.path.join(HERE, "golden", "pileup")


def golden_alignments(name):
    """(reference, SAM records) of a committed alignment case (tests/golden/make_golden_pileup.py)"""
    from test_pileup_oracle import load_case
    contigs, sam, _can, _opts, _want = load_case(name)
    return contigs["ctgA"], [l for l in sam if not l.startswith("@")]


def mix_alignments():
    """a short-read stack that one 9 000-base read spans.  The long read comes first in the file and fills the first
    tiles on its own: each of them has its window at the read's POS, so all of its columns more than 1 536 positions
    in are booked in HBM, on the very positions where the short reads' tiles later book theirs from LDS."""
    from clairvoyante_amd import synth_pileup as sp
    ref, short = sp.make_alignments(seed=4243, ref_len=12000, n_reads=260, start_lo=3000, start_hi=6500, stack=6)
    cigar, seq, _span = sp.make_read(np.random.RandomState(4242), ref, 700, 9000, sp.NOISY_PROFILE)
    long_read = "\t".join(["long0", "0", "ctgA", "701", "60", cigar, "*", "0", "0", seq, "*"])
    lines = sorted([long_read] + short, key=lambda l: int(l.split("\t")[3]))
    return ref, lines


def dense_centres(ref_len):
    """every third position of the first 3 kbp, and every position of the 1 kbp behind them.  A tile of long-read
    segments spans thousands of positions, so it reaches hundreds of these centres: only the first 40 from its first
    segment's POS - 16 on have their counters in LDS, every pair with a later centre is booked in HBM."""
    c = set(range(20, min(ref_len - 20, 3000), 3)) | set(range(3000, 4000))
    return np.asarray(sorted(c), dtype=np.int64)


_inputs = {}


def inputs(name):
    """(reference, SAM records) of `long`, `sparse` (committed) or `mix`"""
    if name not in _inputs:
        _inputs[name] = mix_alignments() if name == "mix" else golden_alignments(name)
    return _inputs[name]


# per long-read input a region (ctgStart, ctgEnd) whose reads hang over both of its ends: the GPU test loads exactly the positions
# the region test lets through as the reference slice, so what the reads book off the slice must vanish
SLICES = {"long": (3000, 6999), "mix": (3500, 6000)}

OLD_RANDOM_SHAPE = dict(ref_len=8000, n_reads=1500, stack=6)      # test_extract_candidates_equals_oracle_on_random_alignments
