"""Writes the `.bin` training file: four back-to-back pickles (total, X blocks, Y blocks, position
blocks) of 500-item blosc chunks -- same command line and layout as
/root/reference/clairvoyante/tensor2Bin.py (Convert :16-28).

    python -m clairvoyante_amd.tensor2Bin --tensor_fn T.gz --var_fn V.gz --bed_fn B.bed --bin_fn OUT.bin
    python -m clairvoyante_amd.tensor2Bin --bam_fn A.bam,B.bam --ref_fn A.fa,B.fa --ctgName chr21,chr22 \
           --ctgStart S1,S2 --ctgEnd E1,E2 --var_fn V.gz --bed_fn B.bed --seed N --bin_fn OUT.bin
    (--vcf_fn TRUTH.vcf.gz in place of --var_fn: the truth rows of each source by GetTruth's rules)

The second form (not in the reference) builds the set from the BAMs on the GPU, utils_v2.GetTrainingSetFromBam.
"""
import argparse
import logging
import pickle
import sys

if __package__ in (None, ""):      # run as `python <dir>/tensor2Bin.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import param

logging.basicConfig(format='%(message)s', level=logging.INFO)


def Convert(args, utils):
    logging.info("Loading the dataset ...")
    sources = utils.bam_sources(args) if hasattr(utils, "bam_sources") else None
    if sources is not None:
        var_fn, vcf_fn = utils.truth_inputs(args)
        total, XC, YC, PC = utils.GetTrainingSetFromBam(
            sources, var_fn, args.bed_fn, amp=args.amp, candidates=args.candidates, genomeSize=args.genomeSize,
            seed=args.seed, samtools=args.samtools, minMQ=args.minMQ, dcov=args.dcov, vcf_fn=vcf_fn).blocks()
    else:
        total, XC, YC, PC = utils.GetTrainingArray(args.tensor_fn, args.var_fn, args.bed_fn)
    logging.info("Writing to binary ...")
    with open(args.bin_fn, "wb") as fh:
        for obj in (total, XC, YC, PC):
            pickle.dump(obj, fh)


def Run(args):
    from . import utils_v2 as utils
    utils.SetupEnv()
    if getattr(args, "blosc_blocksize", None):
        utils.PACK_BLOCKSIZE = int(args.blosc_blocksize)
    if getattr(args, "pack", None):
        utils.PACK_ROUTE = args.pack
    Convert(args, utils)


def build_parser():
    parser = argparse.ArgumentParser(description="Generate a binary format input tensor")
    for flag, default, text in (("--tensor_fn", "vartensors", "Tensor input"), ("--var_fn", "truthvars", "Truth variants list input"),
                                ("--bed_fn", None, "High confident genome regions input in the BED format"),
                                ("--bin_fn", None, "Output a binary tensor file")):
        parser.add_argument(flag, type=str, default=default, help=text)
    for flag, default, text in (("--v3", True, "Use Clairvoyante version 3"), ("--v2", False, "Use Clairvoyante version 2")):
        parser.add_argument(flag, type=param.str2bool, nargs='?', const=True, default=default, help=text)
    parser.add_argument("--blosc_blocksize", type=int, default=None,
                        help="Write c-blosc's multi-block layout with blocks of this many bytes (e.g. 65536: many short "
                             "streams per chunk, what the device decoder likes); default: one stream per chunk")
    parser.add_argument("--pack", type=str, default=None, choices=("host", "device"),
                        help="Where the X blocks of a set built on the GPU are compressed: host (the default; the file is "
                             "byte for byte what it has always been) or device (only the compressed form crosses to the host; "
                             "c-blosc's multi-block layout, blocks of 65536 bytes unless --blosc_blocksize names another)")
    from .utils_v2 import BAM_FLAGS
    for flag, typ, default, text in BAM_FLAGS:
        parser.add_argument(flag, type=typ, default=default, help=text)
    return parser


def main():
    parser = build_parser()
    args = parser.parse_args()
    from .utils_v2 import bam_sources
    try:
        bam_sources(args)
    except ValueError as e:
        parser.error(str(e))
    if not sys.argv[1:]:
        parser.print_help()
        sys.exit(1)
    Run(args)


if __name__ == "__main__":
    main()
