"""Randomly sampled genome positions: command line and output rows of /root/reference/dataPrepScripts/RandomSampling.py
(MakeCandidates :16-73, main :76-111).

    python -m clairvoyante_amd.RandomSampling --ref_fn REF.fa --ctgName chr21 [--ctgStart S --ctgEnd E] [--bed_fn B] \
           [--candidates 7000000 --genomeSize 3000000000] [--seed N] [--can_fn OUT.gz] > POSITIONS

One row "<ctg>\\t<pos>" per position of range(start, end) (:26-39: start 1 or --ctgStart, end the contig's length in
REF.fa.fai or --ctgEnd, exclusive as the reference's xrange) that lies in the BED, when there is one (:41-61), and that
the draw keeps with probability candidates * 2 / genomeSize (:63-68).  The reference draws from Python's unseeded generator
once per position; here the draw is keyed by (seed, contig, position) -- draws.py, stream RANDOM --, so --seed N repeats a
run and the GPU can draw the same positions (CV_BED_ITEMS=device, csrc/cv_beditems_dev.hip).  --can_fn FILE writes through
`gzip -c` as ExtractVariantCandidates does; the reference's own branch for it refers to a handle it never opens (:70-73).
"""
import os
import shlex
import subprocess
import sys

if __package__ in (None, ""):      # run as `python <dir>/RandomSampling.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import bed_items, draws
from .ExtractVariantCandidates import read_bed


def MakeCandidates(args):
    fai_fn = "%s.fai" % args.ref_fn
    if not os.path.isfile(fai_fn):
        sys.stderr.write("Fasta index %s.fai doesn't exist.\n" % args.ref_fn)
        sys.exit(1)
    if args.ctgName is None:
        sys.stderr.write("Please define --ctgName. Exiting ...\n")
        sys.exit(1)
    start, end = 1, -1
    with open(fai_fn, "r") as f:
        for l in f:
            s = l.strip().split()
            if s[0] == args.ctgName:
                end = int(s[1])
    if end == -1:
        sys.stderr.write("Chromosome %s not found in %s\n" % (args.ctgName, fai_fn))
    if args.ctgEnd is not None and args.ctgEnd < end:
        end = args.ctgEnd
    if args.ctgStart is not None and args.ctgStart > start:
        start = args.ctgStart
    intervals = read_bed(args.bed_fn, args.ctgName) if args.bed_fn is not None else None
    args.outputProb = (args.candidates * 2.) / args.genomeSize
    seed = draws.resolve_seed(getattr(args, "seed", None), "RandomSampling")
    pos = bed_items.sample_positions(args.ctgName, start, end, args.outputProb, intervals, seed)
    head = "%s\t" % args.ctgName
    text = "".join([head + "%d\n" % p for p in pos.tolist()]).encode()
    if args.can_fn != "PIPE":
        fpo = open(args.can_fn, "wb")
        fp = subprocess.Popen(shlex.split("gzip -c"), stdin=subprocess.PIPE, stdout=fpo, stderr=sys.stderr, bufsize=8388608)
        fp.stdin.write(text)
        fp.stdin.close()
        fp.wait()
        fpo.close()
    else:
        sys.stdout.buffer.write(text)
        sys.stdout.buffer.flush()
    return pos


_CLI = (
    ("--ref_fn", str, "ref.fa", "Reference fasta file input, mandatory, default: %(default)s"),
    ("--ctgName", str, None, "The name of the sequence to be processed, mandatory, default: %(default)s"),
    ("--can_fn", str, "PIPE", "Randomly sampled genome position output, use PIPE for standard output, optional, "
                              "default: %(default)s"),
    ("--candidates", int, 7000000, "For the whole genome, the number of variant candidates to be generated, optional, "
                                   "default: %(default)s"),
    ("--genomeSize", int, 3000000000, "The size of the genome, optional, default: %(default)s"),
    ("--bed_fn", str, None, "Generate positions only in these regions, works in intersection with ctgName, ctgStart and "
                            "ctgEnd, optional, default: as defined by ctgName, ctgStart and ctgEnd"),
    ("--ctgStart", int, None, "The 1-bsae starting position of the sequence to be processed, optional"),
    ("--ctgEnd", int, None, "The inclusive ending position of the sequence to be processed, optional"),
    ("--seed", int, None, "Keep positions by draws keyed by this seed, position and contig (repeatable); default: 64 bits "
                          "of Python's generator, logged"),
)


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Generate variant candidates using alignments")
    for flag, typ, default, text in _CLI:
        parser.add_argument(flag, type=typ, default=default, help=text)
    return parser


def main():
    parser = build_parser()
    args = parser.parse_args()
    if not sys.argv[1:]:
        parser.print_help()
        sys.exit(1)
    MakeCandidates(args)


if __name__ == "__main__":
    main()
