"""Inputs and two definitions of the result for utils_v2.GetTrainingSetFromBam (tests/test_gpu_bam_trainset.py):

  recipe()  the file recipe of dataPrepScripts/PrepDataBeforeDemo.sh run through this project's own command-line modules
            (ExtractVariantCandidates --gen4Training --seed, CreateTensor twice per source, the files concatenated,
            PairWithNonVariants --seed, the host loop of GetTrainingArray)
  model()   the same set from the CPU oracles alone (oracle/extract_candidates.py, oracle/create_tensor.py) and a plain
            restatement of the pairing and the labels: nothing in it ever ran on a GPU

Synthetic alignments of clairvoyante_amd/synth_pileup.py; planted truth rows (SNP, insertion, deletion, het and hom,
one longer than 4); a BED over about two thirds of the contig with one interval of length 1; outputProb 0.3."""
import argparse
import gzip
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FAKE = "%s %s" % (sys.executable, os.path.join(HERE, "golden", "fake_samtools.py"))
CANDIDATES, GENOME = 15, 100                    # outputProb = 2 * 15 / 100 = 0.3
PROB = (CANDIDATES * 2.) / GENOME
FLANK = 16
_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")
BASE2NUM = dict(zip("ACGT", (0, 1, 2, 3)))


def make_source(d, tag, ctg, seed, ref_len=6000, n_reads=900, region=(None, None), read_len=None, profile=None):
    """one source on disk: SAM text (the stand-in's "BAM"), FASTA + .fai -> dict; read_len / profile: those of
    synth_pileup.make_alignments (default: its own)"""
    from clairvoyante_amd import synth_pileup as sp
    kw = {} if read_len is None else {"read_len": read_len}
    ref, lines = sp.make_alignments(seed, ref_len=ref_len, n_reads=n_reads, ctg=ctg, start_hi=ref_len - 600, profile=profile, **kw)
    sam, fa = os.path.join(d, tag + ".sam"), os.path.join(d, tag + ".fa")
    with open(sam, "w") as fh:
        fh.write("@SQ\tSN:%s\tLN:%d\n" % (ctg, ref_len) + "\n".join(lines) + "\n")
    head = ">%s\n" % ctg
    with open(fa, "w") as fh:
        fh.write(head + "".join(ref[i:i + 60] + "\n" for i in range(0, ref_len, 60)))
    with open(fa + ".fai", "w") as fh:
        fh.write("%s\t%d\t%d\t60\t61\n" % (ctg, ref_len, len(head)))
    return {"tag": tag, "ctg": ctg, "ref": ref, "lines": lines, "sam": sam, "fa": fa, "cs0": region[0], "ce0": region[1]}


def source_tuple(s, bam=None):
    return (bam or s["sam"], s["fa"], s["ctg"], s["cs0"], s["ce0"])


def truth_rows(ctg, ref, seed, n=100, extra=()):
    """planted truth rows `ctg pos ref alt gt1 gt2` at n random positions + `extra`, the five kinds in turn"""
    rng = np.random.RandomState(seed)
    pos = sorted(set(int(p) for p in rng.randint(30, len(ref) - 30, n)) | set(extra))
    rows = []
    for k, p in enumerate(pos):
        b = ref[p - 1].upper()
        b = b if b in BASE2NUM else "A"
        alt = "ACGT"[(BASE2NUM[b] + 1 + k % 3) % 4]
        kind = k % 5
        if kind == 0:
            rows.append((ctg, p, b, alt, "0", "1"))
        elif kind == 1:
            rows.append((ctg, p, b, alt, "1", "1"))
        elif kind == 2:
            rows.append((ctg, p, b, b + "GT"[k % 2] * (1 + k % 3), "0", "1"))
        elif kind == 3:
            rows.append((ctg, p, b + "AC", b, "1", "1"))
        else:
            rows.append((ctg, p, b + "ACGTAC", b, "0", "1"))         # length 6 > 4
    return rows


def bed_rows(ctg, ref_len, single):
    """six intervals over about two thirds of the contig; `single` gets an interval of length 1 (the end == begin rule)"""
    step = ref_len // 6
    rows = [(ctg, k * step + step // 6, k * step + step // 6 + (2 * step) // 3) for k in range(6)]
    rows = [r for r in rows if not (r[1] <= single < r[2])]
    rows.append((ctg, single, single + 1))
    return rows


def write_rows(fn, rows):
    with gzip.open(fn, "wt") as fh:
        for r in rows:
            fh.write(" ".join(str(x) for x in r) + "\n")
    return fn


# ---- the file recipe through the project's own modules ----------------------------------------------------------------
_files_memo = {}


def source_files(sources, var_fn, seed, d, samtools=FAKE):
    """steps 1-4 of the recipe per source, once per (sources, seed): -> (tensor files of the truth rows, of the sampled rows)"""
    key = (tuple(sources), var_fn, seed, samtools)
    if key in _files_memo:
        return _files_memo[key]
    from clairvoyante_amd import CreateTensor, ExtractVariantCandidates
    tvs, tcs = [], []
    tag = "s%d" % len(_files_memo)
    for k, (bam, fa, ctg, cs0, ce0) in enumerate(sources):
        region = [] if cs0 is None else ["--ctgStart", str(cs0), "--ctgEnd", str(ce0)]
        common = ["--bam_fn", bam, "--ref_fn", fa, "--ctgName", ctg, "--samtools", samtools] + region
        can = os.path.join(d, "%s_can_%d.gz" % (tag, k))
        ExtractVariantCandidates.MakeCandidates(ExtractVariantCandidates.build_parser().parse_args(
            common + ["--can_fn", can, "--gen4Training", "--candidates", str(CANDIDATES), "--genomeSize", str(GENOME),
                      "--seed", str(seed)]))
        for src, out, acc in ((var_fn, "%s_tensor_var_%d.gz" % (tag, k), tvs), (can, "%s_tensor_can_%d.gz" % (tag, k), tcs)):
            out = os.path.join(d, out)
            CreateTensor.OutputAlnTensor(CreateTensor.build_parser().parse_args(common + ["--can_fn", src, "--tensor_fn", out]))
            acc.append(out)
    _files_memo[key] = (tvs, tcs)
    return tvs, tcs


def recipe(sources, var_fn, bed_fn, amp, seed, d, samtools=FAKE):
    """-> dict(arrays = trainset_cases.arrays_of(host loop, unshuffled), pair = what Pair() returned, mix = its file)"""
    import trainset_cases as cases
    from clairvoyante_amd import PairWithNonVariants, utils_v2
    tvs, tcs = source_files(sources, var_fn, seed, d, samtools)
    tv, tc_, mix = (os.path.join(d, n) for n in ("tensor_var.gz", "tensor_can.gz", "mix.gz"))
    for out, parts in ((tv, tvs), (tc_, tcs)):                          # `cat`: gzip members one behind the other
        with open(out, "wb") as fh:
            for p in parts:
                fh.write(open(p, "rb").read())
    pair = PairWithNonVariants.Pair(argparse.Namespace(tensor_can_fn=tc_, tensor_var_fn=tv, bed_fn=bed_fn, output_fn=mix,
                                                       amp=amp, seed=seed))
    arrays = cases.arrays_of(utils_v2._training_array_host(mix, var_fn, bed_fn, shuffle=False))
    return {"arrays": arrays, "pair": pair, "mix": mix}


# ---- the same set from the CPU oracles ---------------------------------------------------------------------------------
def _view(lines, ctg, cs, ce):
    out = []
    for line in lines:
        f = line.split("\t")
        if f[2] != ctg or (int(f[1]) & 2308):
            continue
        if cs is not None:
            p = int(f[3])
            span = sum(int(n) for n, op in _CIGAR.findall(f[5]) if op in "MDN=X")
            if p + max(span, 1) - 1 < cs or p > ce:
                continue
        out.append(line)
    return out


def label(row):
    ref, alt, g1, g2 = row[2], row[3], row[4], row[5]
    v = [0.0] * 16
    snp = len(ref) == 1 and len(alt) == 1
    if (g1, g2) == ("0", "1"):
        v[BASE2NUM[ref[0]]] = 0.5
        if snp:
            v[BASE2NUM[alt[0]]] = 0.5
        v[4] = 1.0
    elif (g1, g2) == ("1", "1"):
        if snp:
            v[BASE2NUM[alt[0]]] = 1.0
        v[5] = 1.0
    v[9 if len(ref) > 1 and len(alt) == 1 else 8 if len(alt) > 1 and len(ref) == 1 else 7] = 1.0
    d = abs(len(ref) - len(alt))
    v[15 if d > 4 else 10 + d] = 1.0
    return v


def bed_hit(bed, ctg, p):
    for c, b, e in bed:
        e -= 1
        if e == b:
            e += 1
        if c == ctg and b <= p < e:
            return True
    return False


_rows_memo = {}


def source_rows(s, truth, seed):
    """source_rows_once, computed once per (source, region, seed): the oracle pileup takes seconds"""
    key = (s["tag"], s["cs0"], s["ce0"], seed, len(truth))
    if key not in _rows_memo:
        _rows_memo[key] = source_rows_once(s, truth, seed)
    return _rows_memo[key]


def source_rows_once(s, truth, seed):
    """per source, from the oracles: the rows of its two tensor files as [(pos, X [33,4,4] fp32, centre base)] -> (var
    rows, can rows, sampled positions, truth positions inside the range)"""
    from clairvoyante_amd import draws
    from oracle import create_tensor as ct
    from oracle import extract_candidates as evc
    ctg, ref, cs0, ce0 = s["ctg"], s["ref"], s["cs0"], s["ce0"]
    cs, ce, rs, re_ = ct.region_bounds(cs0, ce0)
    rows = evc.candidates(ctg, ref, s["lines"], cs0, ce0, 0, 0, 0)
    pos, late, seen = [], [], set()
    for r in rows:
        p = int(r.split()[1])
        late.append(1 if p in seen else 0)                              # a position's second row is its late entry
        seen.add(p)
        pos.append(p)
    u = draws.draws(seed, draws.SAMPLE, ctg, pos, late)
    sampled = sorted(set(p for p, ui in zip(pos, u) if not ui > PROB and (cs is None or cs <= p <= ce)))
    tpos = sorted(set(r[1] for r in truth if r[0] == ctg and (cs is None or cs <= r[1] <= ce)))
    ref_seq = ref if rs is None else ref[rs - 1:re_]
    shift = 0 if rs is None else rs - 1
    acc = ct.pileup(ref_seq, rs, _view(s["lines"], ctg, cs, ce), sorted(set(sampled) | set(tpos)), 0, 250, True)

    def made(plist):
        out = []
        for p in plist:
            if p in acc and p - shift - (FLANK + 1) >= 0:
                x = np.asarray(acc[p].counts, dtype=np.float32).reshape(33, 4, 4).copy()
                x[:, :, 1:] -= x[:, :, 0:1]
                out.append((p, x, ref_seq[p - shift - 1].upper()))
        return out
    return made(tpos), made(sampled), sampled, tpos


def model(sources, truth, bed, amp, seed):
    """-> dict(keys sorted, X [n,528] uint32 bits, Y [n,16] float64, v, c, r, and what the tests assert about the inputs)"""
    from clairvoyante_amd import draws
    per = [(s["ctg"],) + source_rows(s, truth, seed) for s in sources]
    var = [(ctg, p, x, b) for ctg, vr, _cr, _s, _t in per for p, x, b in vr]
    can = [(ctg, p, x, b) for ctg, _vr, cr, _s, _t in per for p, x, b in cr]
    d = set((ctg, p) for ctg, p, _x, _b in var)
    inbed = lambda ctg, p: bed is None or bed_hit(bed, ctg, p)
    usable = [(ctg, p, x, b) for ctg, p, x, b in can if inbed(ctg, p) and (ctg, p) not in d]
    v, c = len(var), len(usable)
    r = min(1.0, (v * amp) / c) if c else 1.0
    picked = [row for row in usable if draws.draws(seed, draws.PAIR, row[0], [row[1]])[0] < r]
    Y = {}
    for row in truth:
        if inbed(row[0], row[1]):
            Y["%s:%d" % (row[0], row[1])] = label(row)
    X = {}
    for ctg, p, x, b in var + picked:                                   # the mixed file, through the reader and the host loop
        if b not in BASE2NUM or not inbed(ctg, p):
            continue
        key = "%s:%d" % (ctg, p)
        X[key] = x
        if key not in Y:
            y = [0.0] * 16
            y[5] = y[6] = y[10] = 1.0
            y[BASE2NUM[b]] = 1.0
            Y[key] = y
    keys = sorted(X)
    n = len(keys)
    truth_pos = set((r_[0], r_[1]) for r_ in truth)
    return {
        "keys": keys, "v": v, "c": c, "r": r, "picked": len(picked),
        "X": (np.stack([X[k] for k in keys]) if n else np.zeros((0, 33, 4, 4), np.float32)).reshape(n, 528).view(np.uint32),
        "Y": np.array([Y[k] for k in keys], dtype=np.float64).reshape(n, 16),
        # about the inputs
        "truth_kept": sum(1 for ctg, p, _x, b in var if inbed(ctg, p) and b in BASE2NUM),
        "truth_without_row": sum(len(t) for _c, _vr, _cr, _s, t in per) - len(var),
        "truth_outside_bed": sum(1 for ctg, p in truth_pos if not inbed(ctg, p)),
        "nonvariants_kept": sum(1 for row in picked if row[3] in BASE2NUM),
        "nonvariants_dropped": c - len(picked),
        "sampled_at_truth": sum(len(set(s_) & set(t)) for _c, _vr, _cr, s_, t in per),
        "centres_at_N": sum(1 for _ctg, _p, _x, b in var + can if b == "N"),
    }
