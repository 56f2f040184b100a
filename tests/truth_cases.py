"""Inputs shared by tests/test_truth_core_host.py, tests/test_truth_tables_host.py and tests/test_gpu_truth_tables.py:
truth lists, BED files and truth VCFs that exercise every rule of utils_v2._read_bed_truth / _label / GetTruth, the
irregular lines the device route must leave to the host, and the Python definition applied to ONE line (what
csrc/cv_truth_core.hpp is held to)."""
import gzip
import io
import os

import numpy as np

VAR, BED, VCF = 0, 1, 2
ROW, SKIP, HOST = 0, 1, 2
# contigs that alternate, names that are prefixes of each other, chr10 before chr2
CONTIGS = ("chr1", "chr10", "chr2", "chr", "1")
_BASES = "ACGT"


def _allele(rng, n):
    return "".join(_BASES[k] for k in rng.randint(0, 4, n))


def truth_lines(seed=5, n=1500, contigs=CONTIGS):
    """n truth rows, unsorted, with repeated keys (other alleles: the last one wins), runs of one contig and stretches
    where the contigs alternate line by line; SNPs, insertions and deletions of every length class, genotypes with and
    without a zygosity, tab and multi-blank separators, trailing columns, a blank line now and then"""
    rng = np.random.RandomState(seed)
    out = []
    gts = (("0", "1"), ("1", "1"), ("1", "2"), ("0", "0"), ("2", "2"), ("1", "0"), ("01", "1"), ("0", "1"), ("1", "1"))
    ctg = contigs[0]
    for i in range(n):
        if i % 97 == 0 or (300 <= i < 420):                  # a new run / the alternating stretch
            ctg = contigs[rng.randint(0, len(contigs))]
        pos = int(rng.choice((rng.randint(1, 3000), rng.randint(1, 3000), rng.randint(0, 10 ** 12))))
        if i % 11 == 0 and out:                              # a key again
            prev = out[rng.randint(0, len(out))].split()
            if len(prev) >= 2:
                ctg, pos = prev[0], int(prev[1])
        kind = rng.randint(0, 6)
        rl, al = ((1, 1), (1, rng.randint(2, 9)), (rng.randint(2, 9), 1), (rng.randint(2, 5), rng.randint(2, 5)), (1, 1), (1, 2))[kind]
        g = gts[rng.randint(0, len(gts))]
        sep = ("\t", "  ", " \t ")[i % 3] if i % 13 == 0 else " "
        row = sep.join((ctg, str(pos), _allele(rng, rl), _allele(rng, al), g[0], g[1]))
        if i % 17 == 0:
            row += sep + "extra column"
        if i % 29 == 0:
            row = " " + row + " \t"
        out.append(row)
        if i % 211 == 0:
            out.append(("", "   ", "\t")[i % 3])
    # the same base where no branch reads it: N as the first base of a hom indel and of a genotype without zygosity
    out += ["chr2 77 N NT 1 1", "chr2 78 NA N 1 2", "chr2 79 n a 0 0"]
    return [l.encode() for l in out]


def bed_lines(seed=6, n=400, contigs=CONTIGS, spread=3000):
    """n intervals over the contigs, unsorted and alternating: nested, overlapping, equal, one-base (end == begin + 1:
    the += 1 rule), end == begin, end < begin, begin 0 with end 0; some far out; tab separators and trailing columns"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        ctg = contigs[rng.randint(0, len(contigs))]
        b = int(rng.randint(0, spread)) if i % 19 else int(rng.randint(0, 10 ** 12 - 1000))
        e = b + int(rng.choice((0, 1, 1, 2, 5, 40, 200, -3)))
        e = max(e, 0)
        sep = "\t" if i % 2 else " "
        row = sep.join((ctg, str(b), str(e)))
        if i % 7 == 0:
            row += sep + "name\t0 +"
        out.append(row)
        if i % 31 == 0:
            out.append(out[rng.randint(0, len(out))])        # an interval twice
        if i % 101 == 0:
            out.append("")
    for ctg in contigs:                                      # every truth contig has an interval
        out.append("%s 0 0" % ctg)
        out.append("%s 100 2500" % ctg)
    return [l.encode() for l in out]


def vcf_lines(seed=7, n=600, contigs=("chr1", "chr10", "chr2")):
    """a truth VCF: a header that carries non-ASCII bytes, records of several contigs (sorted per contig), phased and
    unphased genotypes, ./., 1|2 with 2-3 ALT alleles of equal and unequal length, extra sample columns"""
    rng = np.random.RandomState(seed)
    out = [b"##fileformat=VCFv4.2", "##source=caf\xe9 \xb5-benchmark".encode("latin1"), b"##contig=<ID=chr1>",
           b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1"]
    gts = ("0/1", "1/1", "0|1", "1|0", "1|1", "./.", "1/2", "2|1", ".|1", "0/0", "1/2", "2/2")
    for ctg in contigs:
        pos = 0
        for i in range(n // len(contigs)):
            pos += int(rng.randint(1, 12))
            gt = gts[rng.randint(0, len(gts))]
            ref = _allele(rng, int(rng.choice((1, 1, 1, 2, 4))))
            if "2" in gt:
                k = int(rng.randint(2, 4))
                lens = [int(rng.choice((1, 2, 3)))] * k if i % 2 else [int(rng.randint(1, 5)) for _ in range(k)]
                alt = ",".join(_allele(rng, l) for l in lens)
            else:
                alt = _allele(rng, int(rng.choice((1, 1, 2, 6))))
            cols = [ctg, str(pos), ".", ref, alt, "50", "PASS", ".", "GT:DP"]
            if i % 5 == 0:
                cols.append("0/1:9")                         # another sample in front of the last column
            cols.append(gt + ":%d" % rng.randint(5, 60))
            out.append("\t".join(cols).encode())
            if i % 173 == 0:
                out.append(b"")
    return out


def write_lines(path, lines, how="plain", last_newline=True):
    """the lines as a file: plain text, ordinary gzip, or BGZF (small members, so that a file has several)"""
    from clairvoyante_amd import utils_v2
    text = b"\n".join(lines) + (b"\n" if last_newline and lines else b"")
    if how == "plain":
        with open(path, "wb") as fh:
            fh.write(text)
    elif how == "gz":
        with gzip.open(path, "wb", compresslevel=1) as fh:
            fh.write(text)
    else:
        with utils_v2.BgzfWriter(path, level=1, block=6000, threads=1) as fh:
            fh.write(text)
    return path


# ---- irregular lines: (name, format the line goes into, line, stays on the device) ------------------------------------------
IRREGULAR = (
    ("noncanonical_integer", VAR, b"chr1 01070 A C 0 1", False),
    ("carriage_return", VAR, b"chr1 1071 A C 0 1\r", False),
    ("x1c_separator", VAR, b"chr1 1072 A C 0\x1c1 1", False),
    ("high_byte_in_contig", VAR, b"chr\xe91 1073 A C 0 1", False),
    ("five_token_truth_row", VAR, b"chr1 1074 A C 0", False),
    ("two_token_bed_row", BED, b"chr1 500", False),
    ("n_first_base_of_het_indel", VAR, b"chr1 1075 NA N 0 1", False),
    ("n_where_no_branch_reads_it", VAR, b"chr1 1076 NA N 1 1", True),
    ("overlong_line", VAR, b"chr1 1077 A " + b"C" * 9000 + b" 0 1", False),
    ("haploid_genotype_on_the_wanted_contig", VCF, b"chr1\t301\t.\tA\tC\t50\tPASS\t.\tGT\t1", False),
    ("haploid_genotype_on_another_contig", VCF, b"chrM\t301\t.\tA\tC\t50\tPASS\t.\tGT\t1", True),
)
# sources of format VCF: (contig, ctgStart, ctgEnd) as GetTruth.variant_rows takes them (both bounds or none)
VCF_FILTERS = ((b"chr1", 100, 700), (b"chr10", None, None))


# ---- the definition over ONE line -----------------------------------------------------------------------------------------
def define_line(line, fmt, filt=None):
    """utils_v2._read_bed_truth's loop body over the file that holds just `line` ->
    ("ROW", contig str, pos, end or label) | ("SKIP",) | ("RAISE", exception) | ("LINES", k): the definition reads k != 1
    lines there (universal newlines), so no verdict over the bytes as ONE line can stand for it.  Format VCF: the line
    goes through GetTruth.variant_rows for the source `filt` = (contig, ctgStart, ctgEnd) first, its row through that loop"""
    from clairvoyante_amd import GetTruth, utils_v2
    if fmt == VCF:
        stream = list(io.BytesIO(line + b"\n"))
        if len(stream) != 1:
            return ("LINES", len(stream))
        try:
            rows = list(GetTruth.variant_rows(stream, filt[0].decode("ascii"), filt[1], filt[2]))
        except Exception as e:                               # noqa: BLE001
            return ("RAISE", e)
        if not rows:
            return ("SKIP",)
        row = rows[0].decode("ascii", "replace").split()     # (vcf_truth_rows hands the row to the loop as a str)
    else:
        rows = list(io.TextIOWrapper(io.BytesIO(line + b"\n"), encoding="ascii", errors="replace"))
        if len(rows) != 1:
            return ("LINES", len(rows))
        row = rows[0].split()
        if not row:
            return ("SKIP",)
    try:
        if fmt == BED:
            begin = int(row[1]); end = int(row[2]) - 1
            if end == begin:
                end += 1
            return ("ROW", row[0], begin, end)
        pos = int(row[1])
        return ("ROW", row[0], pos, utils_v2._label(row))
    except Exception as e:                                   # noqa: BLE001 -- whatever the definition raises
        return ("RAISE", e)


def check_verdict(line, fmt, status, ctg, pos, end, label, filt=None):
    """the core's verdict over `line` against the definition: where it says ROW or SKIP the definition agrees exactly;
    where the definition raises (or reads other lines) it says HOST.  -> None or what is wrong"""
    from clairvoyante_amd import utils_v2
    want = define_line(line, fmt, filt)
    if status == HOST:
        return None
    if want[0] in ("RAISE", "LINES"):
        return "the core vouches (%d) where the definition gives %r" % (status, want)
    if status == SKIP:
        return None if want[0] == "SKIP" else "SKIP against %r" % (want,)
    if status != ROW or want[0] != "ROW":
        return "status %d against %r" % (status, want)
    name = want[1]
    if ctg != name.encode("ascii", "replace") or not utils_v2.contig_token_ok(ctg):
        return "contig %r against %r" % (ctg, name)
    # the tables key on contig + ":" + str(int(token)): the token must be its own canonical spelling
    if pos != want[2] or not 0 <= pos < 10 ** 12:
        return "pos %r against %r" % (pos, want[2])
    if fmt == BED:
        return None if end == want[3] else "end %r against %r" % (end, want[3])
    if [float(v) for v in label] != [float(v) for v in want[3]]:
        return "label %r against %r" % (list(label), want[3])
    return None


def mutated_lines(regular, fmt, n=20000, seed=11):
    """about n lines made from the regular ones: random bytes of all 256 values put in, bytes dropped, truncations at
    every token boundary, the integer forms Python's int() takes and str() does not give back"""
    rng = np.random.RandomState(seed + fmt)
    regular = [l for l in regular if l.strip()]
    ints = (b"+5", b"-5", b"007", b"1_0", b"1234567890123", b"", b"0", b"00", b" 5", b"5.0", b"1e3", b"999999999999")
    out = []
    for l in regular[:300]:                                  # truncations at every token boundary, with and without the blank
        toks = l.split()
        for k in range(len(toks) + 1):
            out.append(b" ".join(toks[:k]))
            out.append(b" ".join(toks[:k]) + b" ")
    for l in regular[:400]:                                  # integer forms in the coordinate tokens
        toks = l.split()
        for field in ((1, 2) if fmt == BED else (1,)):
            for form in ints:
                if len(toks) <= field:
                    continue
                t = list(toks)
                t[field] = form
                out.append(b" ".join(t))
    while len(out) < n:
        l = bytearray(regular[rng.randint(0, len(regular))])
        for _ in range(int(rng.randint(1, 4))):
            how = rng.randint(0, 4)
            at = int(rng.randint(0, len(l) + 1))
            if how == 0 and len(l):
                l[min(at, len(l) - 1)] = int(rng.randint(0, 256))
            elif how == 1:
                l.insert(at, int(rng.randint(0, 256)))
            elif how == 2 and len(l):
                del l[min(at, len(l) - 1)]
            else:
                l.insert(at, int(rng.choice((9, 10, 11, 12, 13, 28, 29, 30, 31, 32, 58, 0, 127, 128, 133, 160, 255))))
        out.append(bytes(l))
    return out


def definition_tables(var_fn, bed_fn):
    """(names, tables, every) of the host loop over the files"""
    from clairvoyante_amd import utils_v2
    every = {}
    tree, Y = utils_v2._read_bed_truth(var_fn, bed_fn, every)
    names, tables = utils_v2._trainset_tables(tree, Y, bed_fn is not None)
    return names, tables, {k: np.array(sorted(v), dtype=np.int64) for k, v in every.items()}


def same_tables(got, want, what=""):
    """got: a TruthTables; want: definition_tables(...)"""
    names, tables, every = want
    assert got.names == names, what
    mine = got.cpu()
    assert sorted(mine) == sorted(tables), what
    for k, v in tables.items():
        assert mine[k].dtype == v.dtype and mine[k].shape == v.shape, (what, k, mine[k].dtype, mine[k].shape, v.dtype, v.shape)
        assert np.array_equal(mine[k], v), (what, k)
    if every is not None:
        assert sorted(got.every) == sorted(every), what
        for k, v in every.items():
            assert got.every[k].dtype == np.int64 and np.array_equal(got.every[k], v), (what, k)
