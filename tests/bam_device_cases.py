"""Shared by tests/test_bam_core_host.py (CPU) and tests/test_gpu_bam_device.py (GPU): the inputs of the device BAM
reader's tests, BAM files with a chosen layout, and a short Python restatement of what the reader must make of a
record -- the walk of cv_bam_view_records (csrc/cv_bam.cpp) and emit / parse_bam_record (csrc/cv_pileup.hip), written
from those two and from the SAM/BAM specification (4.2), not from csrc/cv_bam_core.hpp."""
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, ".."))
import bam_writer  # noqa: E402

F_CT, F_EVC, F_LATE, F_FIRST = 1 << 10, 1 << 11, 1 << 12, 1 << 13
T_MATCH, T_INS, T_DEL = 0, 1, 2
S_LANDED, S_END, S_PARTIAL, S_MISS, S_BAD = 0, 1, 2, 3, 4
C_NONE, C_READ, C_RANGE, C_BIG = 0, 1, 2, 3
NT = b"=ACMGRSVTWYHKDBN"
MAX_RECORD = 1 << 30

CORNER_REF = "ACGTTGCA" * 40


def corner_records():
    """the records of test_bam_records_feed_equals_the_sam_text_feed_on_corner_cases, plus runs of exactly 64, 65 and
    128 columns, an odd l_seq, an operation code above 8 (record `op9`: see write_bam) and a read on the second contig"""
    ref = CORNER_REF
    return [
        "a\t0\tctgA\t1\t60\t20M\t*\t0\t0\t" + ref[0:20] + "\t*",
        "b\t0\tctgA\t1\t60\t10M5I10M\t*\t0\t0\t" + ref[0:10] + "GGGGG" + ref[10:20] + "\t*",
        "c\t0\tctgA\t3\t60\t30M\t*\t0\t0\t*\t*",
        "c2\t0\tctgA\t4\t60\t*\t*\t0\t0\tACGT\t*",
        "d\t0\tctgA\t5\t60\t70I1M\t*\t0\t0\t" + "A" * 70 + "C\t*",
        "d2\t0\tctgA\t5\t7\t2I6=1X3D4M\t*\t0\t0\tTT" + ref[4:10] + "G" + ref[14:18] + "\t*",
        "e\t0\tctgA\t9\t60\t5S100M20D50M3H\t*\t0\t0\t" + "T" * 5 + ref[8:108] + ref[128:178] + "\t*",
        "f\t0\tctgA\t9\t60\t8S\t*\t0\t0\tACGTACGT\t*",
        "r64\t0\tctgA\t20\t60\t64M\t*\t0\t0\t" + ref[19:83] + "\t*",
        "r65\t0\tctgA\t20\t60\t65M\t*\t0\t0\t" + ref[19:84] + "\t*",
        "r128\t0\tctgA\t20\t60\t128M1I64D3M\t*\t0\t0\t" + ref[19:147] + "T" + ref[211:214] + "\t*",
        "odd\t0\tctgA\t33\t60\t7M\t*\t0\t0\t" + ref[32:39] + "\t*",
        "g\t0\tctgA\t40\t60\t3M2P4M\t*\t0\t0\t" + ref[39:46] + "\t*",
        "g2\t0\tctgA\t40\t60\t3M5N4M\t*\t0\t0\t" + ref[39:42] + ref[47:51] + "\t*",
        "g3\t1024\tctgA\t41\t60\t9M\t*\t0\t0\t" + ref[40:49] + "\t*",            # a duplicate: a mask with 1024 drops it
        "op9\t0\tctgA\t60\t60\t5M3N4M\t*\t0\t0\t" + ref[59:64] + ref[64:68] + "\t*",
        "h\t0\tctgA\t300\t60\t12M\t*\t0\t0\t" + ref[299:311].lower() + "\t*",
        "z\t0\tzzz\t5\t60\t10M\t*\t0\t0\tACGTACGTAC\t*",
    ]


CORNER_CENTERS = np.asarray([1, 2, 5, 6, 17, 18, 19, 25, 33, 40, 44, 60, 64, 83, 84, 100, 129, 147, 150, 211, 300, 310, len(CORNER_REF)],
                            dtype=np.int64)


def corner_refs():
    return [("ctgA", len(CORNER_REF)), ("zzz", 50)]


def random_alignments():
    """24 000 noisy reads over 40 kbp: three 16 kbp windows of the linear index"""
    from clairvoyante_amd import synth_pileup as sp
    return sp.make_alignments(seed=902, ref_len=40000, n_reads=24000, profile=sp.NOISY_PROFILE, stack=9, read_len=(40, 120))


def _encode(fields, tid_of, _orig=bam_writer.encode_record):
    blob, tid, beg, end = _orig(fields, tid_of)
    if fields[0] == "op9":          # the second CIGAR operation gets code 9, which no SAM text can spell
        at = 4 + 32 + blob[4 + 8] + 4
        word = struct.unpack_from("<I", blob, at)[0]
        blob = blob[:at] + struct.pack("<I", (word & ~15) | 9) + blob[at + 4:]
    if fields[0].startswith("ph"):  # the long-read placeholder <l_seq>S<span>N inline, the real operations in a CG:B,I tag
        l_name, n = blob[4 + 8], struct.unpack_from("<H", blob, 4 + 12)[0]
        l_seq = struct.unpack_from("<i", blob, 4 + 16)[0]
        c0 = 4 + 32 + l_name
        ops = blob[c0:c0 + 4 * n]
        span = sum(w >> 4 for w in struct.unpack("<%dI" % n, ops) if (w & 15) in (0, 2, 3, 7, 8)) or 1
        body = blob[4:c0] + struct.pack("<II", (l_seq << 4) | 4, (span << 4) | 3) + blob[c0 + 4 * n:] + b"CGBI" + struct.pack("<i", n) + ops
        body = body[:12] + struct.pack("<H", 2) + body[14:]
        blob = struct.pack("<i", len(body)) + body
    return blob, tid, beg, end


def write_bam(path, recs, refs, block_payload=60000, index=True):
    """bam_writer.write_bam with the record `op9` patched and records named `ph...` written with a placeholder CIGAR
    -> [(offset in the inflated stream, length)] of the records"""
    keep = bam_writer.encode_record
    bam_writer.encode_record = _encode
    try:
        bam_writer.write_bam(path, recs, refs, block_payload=block_payload, index=index)
    finally:
        bam_writer.encode_record = keep
    tid_of = {n: i for i, (n, _l) in enumerate(refs)}
    at = first_record_offset(refs)
    out = []
    for line in recs:
        blob = _encode(line.rstrip("\n").split("\t"), tid_of)[0]
        out.append((at, len(blob)))
        at += len(blob)
    return out


def first_record_offset(refs):
    text = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)).encode()
    return 12 + len(text) + sum(8 + len(n.encode()) + 1 for n, _l in refs)


def members(path):
    """[(file offset, size, inflated offset, inflated size)] of the BGZF members of a file"""
    blob = open(path, "rb").read()
    out, off, at = [], 0, 0
    while off < len(blob):
        bsize = struct.unpack_from("<H", blob, off + 16)[0] + 1
        isize = struct.unpack_from("<I", blob, off + bsize - 4)[0]
        out.append((off, bsize, at, isize))
        off += bsize; at += isize
    return out


def inflated(path):
    blob = open(path, "rb").read()
    out = bytearray()
    for off, bsize, _at, _n in members(path):
        xlen = struct.unpack_from("<H", blob, off + 10)[0]
        out += zlib.decompress(blob[off + 12 + xlen:off + bsize - 8], -15)
    return bytes(out)


# ---- the restatement -------------------------------------------------------------------------------------------

def py_walk(d, first, view):
    """cv_bam_view_records' loop over d[first:]: -> (status, stop, [offsets of the records to take, at refID]); a record
    the device reader does not vouch for (block_size, layout, placeholder CIGAR) is S_BAD"""
    tid0, exclude, beg0, end0 = view
    at, lim, offs = first, len(d), []
    while at < lim:
        if lim - at < 4:
            return S_PARTIAL, at, offs
        bs = struct.unpack_from("<i", d, at)[0]
        if bs < 32:
            return S_BAD, at, offs
        if lim - at < 4 + bs:
            return S_PARTIAL, at, offs
        tid, pos, l_name, _mq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", d, at + 4)
        if l_seq < 0 or bs > MAX_RECORD or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
            return S_BAD, at, offs
        if tid < 0 or tid > tid0 or (tid == tid0 and pos >= end0):
            return S_END, at, offs
        take = tid == tid0 and not (flag & exclude)
        cig = struct.unpack_from("<%dI" % n_cig, d, at + 4 + 32 + l_name)
        if take and pos < beg0:
            span = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8)) or 1
            take = pos + span > beg0
        if take and n_cig == 2 and (cig[0] & 15) == 4 and (cig[0] >> 4) == l_seq and (cig[1] & 15) == 3:
            return S_BAD, at, offs
        if take:
            offs.append(at + 4)
        at += 4 + bs
    return S_LANDED, at, offs


def py_parse(d, off, filt, q0):
    """parse_bam_record + emit() on the record at d[off] (refID first) -> (C_NONE,) | (C_RANGE,) |
    (C_READ, pos, rf, leading, cols, [(r0, q0, info, adv0, pos)], SEQ bytes); flags as before the running state"""
    min_mq, evc, evc_min_mq, contig_pass = filt
    _tid, pos, l_name, mq, _bin, n_cig, _flag, l_seq = struct.unpack_from("<iiBBHHHi", d, off)
    cig = struct.unpack_from("<%dI" % n_cig, d, off + 32 + l_name)
    sq = d[off + 32 + l_name + 4 * n_cig:off + 32 + l_name + 4 * n_cig + (l_seq + 1) // 2]
    need = sum(c >> 4 for c in cig if (c & 15) in (0, 1, 4, 7, 8))
    total = sum(c >> 4 for c in cig if (c & 15) <= 8)
    clipped = sum(c >> 4 for c in cig if (c & 15) == 4)
    ct_ok = mq >= min_mq
    evc_ok = bool(evc) and mq >= evc_min_mq and bool(contig_pass)
    if evc_ok and 1.0 - float(clipped) / float(total + 1) < 0.55:
        evc_ok = False
    if not ct_ok and not evc_ok:
        return (C_NONE,)
    if pos < -(1 << 30) or pos > (1 << 31) - (1 << 24) or need > (1 << 31) or total > (1 << 40):
        return (C_RANGE,)
    rf = (F_CT if ct_ok else 0) | (F_EVC if evc_ok else 0)
    nseq = max(l_seq if l_seq > 0 else 1, need)
    nseg = sum(((c >> 4) + 63) // 64 for c in cig if (c & 15) in (0, 1, 2, 7, 8))
    if nseg > (1 << 16) or nseq > (1 << 20):            # damage that asks for much: the counts only
        cols = sum(c >> 4 for c in cig if (c & 15) in (0, 1, 2, 7, 8))
        r, leading = pos, 0
        for c in cig:
            if (c & 15) in (1, 2) and evc_ok and r == pos:
                leading = 1
            if (c & 15) in (0, 2, 7, 8):
                r += c >> 4
        return (C_BIG, pos, rf, leading, cols, nseg, nseq)
    seq = bytes(NT[(sq[k >> 1] >> (4 if k % 2 == 0 else 0)) & 15] for k in range(l_seq)) if l_seq > 0 else b"*"
    if need > len(seq):
        seq += b"?" * (need - len(seq))
    segs, leading, cols = [], 0, 0
    r, q = pos, 0

    def emit(typ, flags, r0, qq, n, ref_advances):
        done = 0
        while done < n:
            ln = min(n - done, 64)
            segs.append(((r0 + done if ref_advances else r0) & 0xffffffff, (0 if typ == T_DEL else qq + done) & 0xffffffff,
                         ln | (typ << 8) | flags | (F_FIRST if done == 0 else 0), done if typ == T_INS else 0, pos & 0xffffffff))
            done += ln
    for c in cig:
        op, v = c & 15, c >> 4
        lf = rf | (F_LATE if evc_ok and r == pos else 0)
        if op == 4:
            q += v
        elif op in (0, 7, 8):
            emit(T_MATCH, rf, r, q0 + q, v, True); r += v; q += v; cols += v
        elif op == 1:
            leading |= 1 if lf & F_LATE else 0
            emit(T_INS, lf, r, q0 + q, v, False); q += v; cols += v
        elif op == 2:
            leading |= 1 if lf & F_LATE else 0
            emit(T_DEL, lf, r, 0, v, True); r += v; cols += v
    return (C_READ, pos, rf, leading, cols, segs, seq)


def pack_case(d, first, view, filt, anchors=()):
    hdr = [len(d), first, view[0], view[1], view[2], view[3], filt[0], filt[1], filt[2], filt[3], len(anchors), 0]
    return struct.pack("<12q", *hdr) + struct.pack("<%dq" % len(anchors), *anchors) + bytes(d)


def unpack_result(out, at):
    """one case of the driver's output -> (dict, next offset)"""
    status, stop, taken = struct.unpack_from("<iqi", out, at); at += 16
    offs = list(struct.unpack_from("<%dI" % taken, out, at)); at += 4 * taken
    refused, used = struct.unpack_from("<ii", out, at); at += 8
    recs = []
    if status not in (S_BAD, S_MISS):
        for _ in range(taken):
            what = struct.unpack_from("<i", out, at)[0]; at += 4
            if what not in (C_READ, C_BIG):
                recs.append((what,))
                continue
            pos, rf, leading, nseg, nseq, cols = struct.unpack_from("<iiiqqq", out, at); at += 36
            if what == C_BIG:
                recs.append((what, pos, rf, leading, cols, nseg, nseq))
                continue
            segs = [struct.unpack_from("<IIiiI", out, at + 20 * k) for k in range(nseg)]; at += 20 * nseg
            seq = out[at:at + nseq]; at += nseq
            recs.append((what, pos, rf, leading, cols, segs, seq))
    return dict(status=status, stop=stop, offs=offs, refused=refused, walkers=used, recs=recs), at


def mutations(d, starts, n, seed):
    """n damaged copies of the stream d (records at `starts`, block_size first): bytes flipped in block_size,
    l_read_name, n_cigar_op or l_seq of one record, or the stream cut short"""
    rng = np.random.RandomState(seed)
    fields = ((0, 4), (4 + 8, 1), (4 + 12, 2), (4 + 16, 4))
    for _ in range(n):
        m = bytearray(d)
        kind = rng.randint(0, 5)
        if kind == 4:
            m = m[:rng.randint(starts[0], len(d))]
        else:
            s = starts[rng.randint(0, len(starts))]
            lo, ln = fields[kind]
            k = s + lo + rng.randint(0, ln)
            m[k] = (m[k] ^ (1 << rng.randint(0, 8))) if rng.randint(0, 2) else rng.randint(0, 256)
        yield bytes(m)
