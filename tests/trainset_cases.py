"""Inputs shared by tests/test_gpu_trainset.py and tests/test_trainset_host.py: small tensor / truth / BED files that
exercise every rule of utils_v2.GetTrainingArray's loop (built from textparse_cases.good_row's vocabulary), and the
host loop's result over them, computed once per (case, shuffle)."""
import functools
import gzip
import os
import random
import re

import numpy as np

import textparse_cases as tc

SEED = 1234
PRODUCER_LINE = re.compile(rb"^[^ \t\r\v\f]+ [^ \t\r\v\f]+ [^ \t\r\v\f]+( -?[0-9]{1,9}(\.[0-9])?){528}$")


def host_lines_of(text):
    """lines the device parser must leave to the host: not empty and not in the producer's format"""
    return sum(1 for l in text.split(b"\n") if l and not (len(l) <= tc.LINE_CAP and PRODUCER_LINE.match(l)))


def _seq(rng, centre=None):
    s = "".join("ACGT"[k] for k in rng.randint(0, 4, 33))
    return s if centre is None else s[:16] + centre + s[17:]


def _row(rng, vocab, ctg, pos, seq):
    return "%s %s %s %s" % (ctg, pos, seq, " ".join(vocab[rng.randint(0, len(vocab), tc.NV)]))


def small_text(seed=17):
    """about 1 300 rows: contigs chr1, chr10, chr2, 1 in runs (chr1 comes back at the end); coordinates of 1 to 12 digits
    among ordinary ones; three keys that occur 2 or 3 times with other values and other centre bases (chr10:1600 is
    also a truth row); three lines with tab separators; lower-case and N centre bases.  -> (bytes, planted HOST lines)"""
    rng = np.random.RandomState(seed)
    vocab = tc._vocabulary()
    lines, planted = [], 0

    def add(ctg, pos, centre=None, lower=False, tabs=False):
        nonlocal planted
        s = _seq(rng, centre)
        line = _row(rng, vocab, ctg, pos, s.lower() if lower else s)
        if tabs:
            line = line.replace(" ", "\t", 2); planted += 1
        lines.append(line)

    for p in (9, 10, 99, 100, 1000):
        add("chr1", p)
    for i in range(400):
        p = 1001 + 3 * i
        add("chr1", p, centre="N" if i % 53 == 7 else None, lower=i % 41 == 3, tabs=i in (50, 333))
        if p == 1301:
            add("chr1", 1300, centre="A")                    # first arrival of a key that returns in the last run
    for p in (1998, 1999, 5000, 5001, 3000):                 # BED edges: end-1 is out, the one-base interval, a truth row outside
        add("chr1", p)
    for i in range(300):
        add("chr10", 1000 + 7 * i, lower=i % 37 == 5, tabs=i == 120)
        if i in (90, 200):
            add("chr10", 1600, centre="ACGT"[i % 4])         # (not on the grid of 7s: a key of its own, twice)
    for i in range(300):
        add("chr2", 1000 + 5 * i, centre="N" if i % 59 == 11 else None)
        if i in (10, 150, 290):
            add("chr2", 2001, centre="CGT"[i % 3])           # three arrivals, three centre bases
    for p in (123456789012, 123456789013, 999999999999, 100000000000):
        add("chr2", p)
    for i in range(200):
        add("1", 10 + 11 * i)
    for i in range(100):
        add("chr1", 1300 + 2 * i, centre="G" if i == 0 else None)      # chr1 again: 1300 a second time, other keys twice
    return ("\n".join(lines) + "\n").encode(), planted


TRUTH = """chr1 1004 A C 0 1
chr1 1007 A G 1 1
chr1 1010 A AT 0 1
chr1 1013 A ATT 1 1
chr1 1016 A ATTT 0 1
chr1 1019 A ATTTT 1 1
chr1 1022 A ATTTTTT 0 1
chr1 1025 AT A 0 1
chr1 1028 ATT A 1 1
chr1 1031 ATTT A 0 1
chr1 1034 ATTTT A 1 1
chr1 1037 ATTTTTTT A 0 1
chr1 1040 C T 0 1
chr1 1040 C G 1 1
chr1 3000 A C 0 1
chr1 9 G T 1 1
chr1 5000 T A 0 1
chr10 1600 A T 0 1
chr10 1007 C CA 1 1
chr2 2001 G C 1 1
chr2 123456789012 A C 0 1
chrX 5 A C 0 1
"""

BED = """chr1 1000 1500
chr1 1100 1200
chr1 1400 2000
chr1 5000 5001
chr1 0 150
chr10 1000 3000
chr2 1000 2500
chr2 123456789000 123456789100
chrX 0 100
"""


def simple_text(n, seed=29):
    """n rows with n distinct keys on two contigs, every one kept"""
    rng = np.random.RandomState(seed)
    vocab = tc._vocabulary()
    return ("\n".join(_row(rng, vocab, "chr1" if i < n // 2 else "chr3", 500 + 2 * i, _seq(rng)) for i in range(n)) + "\n").encode()


CASES = ("full", "nobed", "notruth", "k1000", "k0", "k499")
FORMATS = ("plain", "gz", "bgzf")


@functools.lru_cache(maxsize=None)
def _texts():
    small, planted = small_text()
    return {"small": (small, planted), "k1000": (simple_text(1000), 0), "k499": (simple_text(499), 0)}


def write_case(dirname, case):
    """-> {"plain" / "gz" / "bgzf": tensor file, "var": truth file or None, "bed": BED file or None, "planted": HOST
    lines, "rows": lines of the tensor file}; the files are written once per directory"""
    from clairvoyante_amd import utils_v2
    text, planted = _texts()["small" if case in ("full", "nobed", "notruth", "k0") else case]
    out = {"planted": planted, "rows": text.count(b"\n")}
    base = os.path.join(dirname, case)
    out["plain"], out["gz"], out["bgzf"] = base + ".txt", base + ".txt.gz", base + ".bgzf.gz"
    if not os.path.exists(out["bgzf"]):
        with open(out["plain"], "wb") as fh:
            fh.write(text)
        with gzip.open(out["gz"], "wb", compresslevel=1) as fh:
            fh.write(text)
        with utils_v2.BgzfWriter(out["bgzf"], level=1) as fh:
            fh.write(text)
    truth = TRUTH if case in ("full", "nobed") else None
    bed = {"full": BED, "notruth": BED, "k0": "chrX 0 100\nchrY 5 9\n"}.get(case)
    for tag, content in (("var", truth), ("bed", bed)):
        out[tag] = None
        if content is not None:
            out[tag] = "%s.%s.gz" % (base, tag)
            if not os.path.exists(out[tag]):
                with gzip.open(out[tag], "wt") as fh:
                    fh.write(content)
    return out


def arrays_of(blocks):
    """(total, XC, YC, PC) -> (total, number of blocks, X bits [total,528] uint32, Y float64 [total,16], keys [str])"""
    from clairvoyante_amd import utils_v2
    total, XC, YC, PC = blocks
    assert len(XC) == len(YC) == len(PC)
    if total == 0:
        return 0, len(XC), np.zeros((0, tc.NV), np.uint32), np.zeros((0, 16)), []
    X = np.asarray(utils_v2.DecompressArray(XC, 0, total, total)[0])
    Y = np.asarray(utils_v2.DecompressArray(YC, 0, total, total)[0])
    P = utils_v2.DecompressArray(PC, 0, total, total)[0]
    assert X.dtype == np.float32 and Y.dtype == np.float64
    return total, len(XC), np.ascontiguousarray(X).reshape(total, tc.NV).view(np.uint32), Y, [str(k) for k in P]


_host = {}


def host_result(files, case, shuffle):
    """the host loop over the case's files under SEED, computed once: arrays_of(...)"""
    from clairvoyante_amd import utils_v2
    key = (case, shuffle)
    if key not in _host:
        random.seed(SEED)
        got = arrays_of(utils_v2._training_array_host(files["gz"], files["var"], files["bed"], shuffle))
        for a in got[2:4]:
            a.setflags(write=False)
        _host[key] = got
    return _host[key]
