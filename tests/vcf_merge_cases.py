"""Inputs of the VCF merge tests: chunk files of the shape callVarBamParallel --run leaves behind, their lines of the shape
callVar's _format_record prints.

The regular set is six chunk files over three contigs of the .fai (chr1, chr2, chr10) plus one contig it lacks (chrUn_7);
chr3 is in the .fai and has no record anywhere.  The files come in lexicographic order, which is not genome order
(chr10 before chr1, chr1_100000000 before chr1_10000000); one file holds a header alone.  Among the records: equal POS in
two files, beg = 16 383 and 16 384, a 5-base REF from 16 382 (straddles a window and a leaf bin), REFs that straddle 2^17
and 2^20, one record near 2^29, <INS> / <DEL> with SVTYPE=, LENGUESS=, multi-base REF deletions, PASS / LowQual / '.'."""
import gzip
import os

import numpy as np

COUNTS = (0, 1, 63, 64, 65, 257, 2000)
BLOCKS = (512, 4096, None)
FAI = "chr1\t536870912\t6\t60\t61\nchr2\t242193529\t253404903\t60\t61\nchr3\t198295559\t499634997\t60\t61\nchr10\t133797422\t701235322\t60\t61\n"
FAI_NAMES = [b"chr1", b"chr2", b"chr3", b"chr10"]
HEADER = ("\n".join(['##fileformat=VCFv4.1', '##FILTER=<ID=PASS,Description="All filters passed">',
                     '##FILTER=<ID=LowQual,Description="Confidence in this variant being real is below calling threshold.">',
                     '##ALT=<ID=DEL,Description="Deletion">', '##ALT=<ID=INS,Description="Insertion of novel sequence">',
                     '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
                     '##INFO=<ID=LENGUESS,Number=.,Type=Integer,Description="Best guess of the indel length">',
                     '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
                     '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype Quality">',
                     '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read Depth">',
                     '##FORMAT=<ID=AF,Number=1,Type=Float,Description="Estimated allele frequency in the range (0,1)">']
                    + ["##contig=<ID=%s,length=%s>" % tuple(ln.split("\t")[:2]) for ln in FAI.splitlines()]
                    + ['#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE']) + "\n").encode()
FILE_NAMES = ("p.chr10_0_10000000.vcf", "p.chr1_0_10000000.vcf", "p.chr1_100000000_110000000.vcf",
              "p.chr1_10000000_20000000.vcf", "p.chr2_0_10000000.vcf", "p.chr2_10000000_20000000.vcf")
EMPTY_FILE = 4
assert list(FILE_NAMES) == sorted(FILE_NAMES)


def rec(ctg, pos, ref, alt, qual=30, filt=".", info=".", gt="0/1", dp=40, af=0.5):
    """one line in the shape of callVar._format_record, with its newline"""
    return ("%s\t%d\t.\t%s\t%s\t%d\t%s\t%s\tGT:GQ:DP:AF\t%s:%d:%d:%.4f\n" % (ctg, pos, ref, alt, qual, filt, info, gt, qual, dp, af)).encode()


# (file, line): the records every set from 14 records on holds (a smaller set: the first of them)
SPECIAL = [
    (1, rec("chr1", 16384, "A", "G", 51, "PASS")),                                  # beg 16 383: last base of window 0
    (1, rec("chr1", 16385, "C", "T", 12, "LowQual")),                               # beg 16 384: first base of window 1
    (1, rec("chr1", 16383, "ACGTA", "A", 33, "PASS", gt="1/1")),                    # [16 382, 16 387): two windows, two leaves
    (1, rec("chr1", 131071, "ACGT", "A", 20, info="LENGUESS=3")),                   # [131 070, 131 074) straddles 2^17
    (1, rec("chr1", 1048575, "ACGTAC", "A", 44, "PASS")),                           # [1 048 574, 1 048 580) straddles 2^20
    (1, rec("chr1", 10000000, "T", "<INS>", 18, "LowQual", "SVTYPE=INS")),          # equal POS, this one comes first
    (3, rec("chr1", 10000000, "T", "TA", 61, "PASS", gt="1/1")),                    # ... and this one behind it
    (2, rec("chr1", 100000000, "G", "<DEL>", 9, "LowQual", "SVTYPE=DEL")),          # equal POS across files given in the wrong order
    (3, rec("chr1", 100000000, "G", "C", 70, "PASS")),
    (2, rec("chr1", (1 << 29) - 10, "AC", "A", 25, info="LENGUESS=1")),             # near the end of what a .tbi addresses
    (0, rec("chr10", 7, "N", "A", 1, "LowQual", dp=4, af=0.25)),
    (5, rec("chr2", 12345678, "GATTACA", "G", 40, "PASS", "LENGUESS=6")),
    (5, rec("chrUn_7", 99, "A", "AT", 15, gt="0/1")),                               # a contig the .fai lacks
    (5, rec("chrUn_7", 3, "C", "G", 15, gt="1/1")),                                 # (its file is not sorted: the merge is)
]
FILLER = {0: ("chr10", 1, 10000000), 1: ("chr1", 1, 10000000), 2: ("chr1", 100000000, 110000000),
          3: ("chr1", 10000000, 20000000), 5: ("chr2", 10000000, 20000000)}


def records(total):
    """-> the record lines of each of the six files for a set of `total` records"""
    per = [[] for _ in FILE_NAMES]
    for f, ln in SPECIAL[:total]:
        per[f].append(ln)
    left = total - min(total, len(SPECIAL))
    rs = np.random.RandomState(1000 + total)
    keys = sorted(FILLER)
    for k, f in enumerate(keys):
        n = left // len(keys) + (1 if k < left % len(keys) else 0)
        ctg, lo, hi = FILLER[f]
        # a dense stretch (neighbours share leaf bins and windows) and a sparse one
        pos = np.sort(np.concatenate((rs.randint(lo, lo + 40000, n - n // 2), rs.randint(lo, hi, n // 2))))
        for p in pos.tolist():
            kind = rs.randint(0, 6)
            ref = "ACGT"[p % 4]
            if kind == 0:
                ln = rec(ctg, p, ref + "ACGTTGCA"[:1 + p % 7], ref, 10 + p % 80, ("PASS", "LowQual", ".")[p % 3], "LENGUESS=%d" % (1 + p % 7))
            elif kind == 1:
                ln = rec(ctg, p, ref, ("<INS>", "<DEL>")[p % 2], p % 50, "LowQual", ("SVTYPE=INS", "SVTYPE=DEL")[p % 2])
            else:
                ln = rec(ctg, p, ref, "ACGT"[(p + 1 + kind) % 4], p % 100, ("PASS", "LowQual", ".")[p % 3], gt=("0/1", "1/1")[p % 2],
                         dp=4 + p % 97, af=(1 + p % 99) / 100.0)
            per[f].append(ln)
    assert sum(len(x) for x in per) == total and not per[EMPTY_FILE]
    return per


def write_file(fn, data, form):
    """form: "plain", "gz" (one ordinary gzip member) or "bgzf" (members of 1 000 bytes: records straddle the seams)"""
    if form == "plain":
        with open(fn, "wb") as fh:
            fh.write(data)
    elif form == "gz":
        with gzip.open(fn, "wb") as fh:
            fh.write(data)
    else:
        from clairvoyante_amd import utils_v2
        with utils_v2.BgzfWriter(fn, block=1000, threads=1) as w:
            w.write(data)


def build(folder, total, form="plain", header=HEADER):
    """writes the set -> (files in the order given to the merge, .fai file, records per file)"""
    per = records(total)
    files = []
    for name, lines in zip(FILE_NAMES, per):
        fn = os.path.join(str(folder), name + ("" if form == "plain" else ".gz"))
        write_file(fn, header + b"".join(lines), form)
        files.append(fn)
    fai = os.path.join(str(folder), "ref.fa.fai")
    with open(fai, "w") as fh:
        fh.write(FAI)
    return files, fai, per


def expected_order(per, names=FAI_NAMES):
    """the records sorted by (contig rank, POS, input index), computed without the code under test"""
    rank = {n: i for i, n in enumerate(names)}
    flat = [ln for lines in per for ln in lines]
    for ln in flat:
        rank.setdefault(ln.split(b"\t")[0], len(rank))
    key = lambda t: (rank[t[1].split(b"\t")[0]], int(t[1].split(b"\t")[1]), t[0])
    return [ln for _i, ln in sorted(enumerate(flat), key=key)]


def interval(ln):
    """(contig, beg, end) of a line, restated: END= of INFO counts when it lies behind beg"""
    c = ln.rstrip(b"\n").split(b"\t")
    beg = int(c[1]) - 1
    end = beg + len(c[3])
    for kv in c[7].split(b";"):
        if kv[:4] == b"END=" and int(kv[4:]) > beg:
            end = int(kv[4:])
    return c[0], beg, end


# ---- the C ABI: the arrays of the item line pass, and the host forms over them ------------------------------------------------
def line_arrays(per, names=FAI_NAMES):
    """the record bytes of all files end to end and cv_item_lines_host_form's rows over them -> dict (text: uint8 array,
    16-byte aligned, 16 spare bytes behind n_text)"""
    import ctypes
    from clairvoyante_amd import _lib
    lib = _lib.load()
    data = b"".join(ln for lines in per for ln in lines)
    n_text = len(data)
    raw = np.zeros(n_text + 48, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16
    text = raw[at:at + n_text + 16]
    text[:n_text] = np.frombuffer(data, dtype=np.uint8)
    max_lines = n_text // 16 + 16
    pos, off, ln = (np.zeros(max_lines, dtype=np.int64) for _ in range(3))
    run, tok, info = np.zeros(max_lines, dtype=np.int32), np.zeros((max_lines, 2), dtype=np.int64), np.zeros(8, dtype=np.int64)
    V = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(lib.cv_item_lines_host_form(V(text), n_text, max_lines, V(pos), V(run), V(off), V(ln), V(tok), V(info)))
    used, lines, rows, _skipped, host, runs = info.tolist()[:6]
    assert used == n_text and rows == lines and host == 0
    names = list(names)
    rank = {n: i for i, n in enumerate(names)}
    run_rank = np.zeros(max(runs, 1), dtype=np.int32)
    for k in range(runs):
        name = data[int(tok[k, 0]):int(tok[k, 0] + tok[k, 1])]
        if name not in rank:
            rank[name] = len(names)
            names.append(name)
        run_rank[k] = rank[name]
    return {"text": text, "n_text": n_text, "n": rows, "pos": pos[:rows], "run": run[:rows], "off": off[:rows], "len": ln[:rows],
            "run_rank": run_rank, "nruns": runs, "names": names, "nrank": max(len(names), 1), "_raw": raw}


def host_form(a, out_cap=None, fill=0):
    """cv_vcf_merge_host_form + cv_vcf_windows_host_form over line_arrays' dict -> dict of every output; out_cap: the room
    the call is told the output text has (default: all of it), fill: what the output text holds before the call"""
    import ctypes
    from clairvoyante_amd import _lib
    lib = _lib.load()
    n, nrank = a["n"], a["nrank"]
    V = lambda x: ctypes.c_void_p(x.ctypes.data)
    o = {"srank": np.zeros(max(n, 1), dtype=np.int32), "sbeg": np.zeros(max(n, 1), dtype=np.int64), "send": np.zeros(max(n, 1), dtype=np.int64),
         "ooff": np.zeros(n + 1, dtype=np.int64), "text": np.full(a["n_text"] + 1, fill, dtype=np.uint8),
         "chunks": np.zeros((4, max(n, 1)), dtype=np.int64), "stats": np.zeros((4, nrank), dtype=np.int64), "info": np.zeros(8, dtype=np.int64)}
    _lib.check(lib.cv_vcf_merge_host_form(V(a["text"]), a["n_text"], n, V(a["pos"]), V(a["run"]), V(a["off"]), V(a["len"]), V(a["run_rank"]),
                                          a["nruns"], nrank, V(o["srank"]), V(o["sbeg"]), V(o["send"]), V(o["ooff"]), V(o["text"]),
                                          a["n_text"] if out_cap is None else out_cap, V(o["chunks"]), V(o["stats"]), V(o["info"])))
    count, maxend = o["stats"][2], o["stats"][3]
    o["win_off"] = np.concatenate(([0], np.cumsum(np.where(count > 0, ((maxend - 1) >> 14) + 1, 0)))).astype(np.int64)
    o["win"] = np.zeros(max(int(o["win_off"][-1]), 1), dtype=np.int64)
    _lib.check(lib.cv_vcf_windows_host_form(n, V(o["srank"]), V(o["sbeg"]), V(o["send"]), V(o["ooff"]), nrank, V(o["win_off"]), V(o["win"]),
                                            int(o["win_off"][-1])))
    return o
