"""Inputs shared by tests/test_bed_items_host.py, tests/test_bed_items_core_host.py and tests/test_gpu_bed_items.py: item
files (short truth-style lines and tensor-shaped lines of 2.0-3.6 KB), the host loop's answer over them, the definition
applied to ONE item line (what format ITEM of csrc/cv_truth_core.hpp is held to) and the sampler's BED."""
import io

import numpy as np

import truth_cases as tc

ROW, SKIP, HOST = tc.ROW, tc.SKIP, tc.HOST
LACKING = "chrUn"                                             # a contig the BED of tc.bed_lines() lacks
# what "%0.1f" prints, by width: a line of 528 of them is 2.1 KB from the first pool and 3.6 KB from the last
_VALUES = (("0.0", "1.0"), ("0.0", "1.0", "12.0", "3.0"), ("104.0", "-23.0", "12.0", "57.0"), ("-104.0", "-123.0", "1024.0", "-23.0"))


def item_lines(seed=21, n=2000, contigs=tc.CONTIGS + (LACKING,), spread=6000, short_every=4):
    """n item lines in runs of one contig: every fourth a short truth-style line, the rest "ctg pos SEQ" and 528 values
    printed with %0.1f, 2.0-3.6 KB each; positions inside and outside the intervals of tc.bed_lines(); tab and blank separators"""
    rng = np.random.RandomState(seed)
    out = []
    ctg = contigs[0]
    for i in range(n):
        if i % 53 == 0:
            ctg = contigs[rng.randint(0, len(contigs))]
        pos = int(rng.randint(0, spread))
        if i % short_every == 0:
            out.append(("%s %d A C 0 1" % (ctg, pos)) if i % 8 else ("%s\t%d\tAC\tA\t1\t1" % (ctg, pos)))
            continue
        vals = rng.choice(_VALUES[rng.randint(0, 4)], 528)
        out.append("%s %d %s %s" % (ctg, pos, "ACGTACGTACGTACGTACGTACGTACGTACGTA", " ".join(vals)))
    return [l.encode() for l in out]


def host_answer(items_fn, bed_fn):
    """(bytes written, (lines, kept), exception or None) of the host loop"""
    from clairvoyante_amd import bed_items
    out = io.BytesIO()
    try:
        tally, raised = bed_items.choose_items_host(items_fn, bed_fn, out), None
    except Exception as e:                                   # noqa: BLE001 -- whatever the definition raises
        tally, raised = None, e
    return out.getvalue(), tally, raised


def define_item_line(line):
    """bed_items._host_lines' body over the file that holds just `line` -> ("ROW", contig bytes, pos) | ("RAISE", exception) |
    ("LINES",): the loop reads other lines there"""
    if b"\n" in line:
        return ("LINES",)
    try:
        tok = line.split()
        return ("ROW", tok[0], int(tok[1]))
    except Exception as e:                                   # noqa: BLE001
        return ("RAISE", e)


def check_item_verdict(line, status, ctg, pos):
    """the core's verdict against the definition: a ROW has the loop's (contig, position), canonically spelt; a line the
    loop raises on (or reads as several) is HOST; there is no SKIP -> None or what is wrong"""
    want = define_item_line(line)
    if status == HOST:
        return None
    if status != ROW:
        return "status %d: format ITEM has no SKIP" % status
    if want[0] != "ROW":
        return "the core vouches where the definition gives %r" % (want,)
    if ctg != want[1] or pos != want[2] or not 0 <= pos < 10 ** 12:
        return "(%r, %r) against %r" % (ctg, pos, want)
    if line.split()[1] != str(pos).encode():
        return "the position token %r is not canonical" % line.split()[1]
    return None


def bed_tables(bed_fn):
    """(names as bytes, bed_off, bed_begin, bed_emax) of the host's reading of a BED file, in the layout of cv_bed_table_dev"""
    from clairvoyante_amd import bed_items
    tree = bed_items.bed_tree(bed_fn)
    names = sorted(tree)
    off, begin, emax = [0], [], []
    for k in names:
        b, e = tree[k].table()
        begin.append(b); emax.append(e)
        off.append(off[-1] + len(b))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    return [k.encode("ascii") for k in names], np.array(off, dtype=np.int64), cat(begin), cat(emax)


def sample_intervals(end=100000, n=60, seed=3):
    """n half-open intervals over a contig of `end` positions: some overlap, some are nested, one reaches past the end"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n - 1):
        b = int(rng.randint(0, end))
        out.append((b, b + int(rng.choice((1, 2, 50, 700, 3000)))))
        if i % 9 == 0:
            out.append((b + 10, b + 20))                     # nested or overlapping
    out.append((end - 500, end + 800))
    return out[:n - 1] + [out[-1]]
