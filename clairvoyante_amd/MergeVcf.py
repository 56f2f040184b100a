"""The end of the whole-genome recipe, `vcfcat PREFIX*.vcf | vcfstreamsort | bgziptabix OUT.vcf.gz`, in one command:

    python -m clairvoyante_amd MergeVcf --vcf_glob 'hg001*.vcf' --ref_fn REF.fa --out_fn hg001.vcf.gz

The chunk VCFs (plain, .gz or BGZF) become one VCF sorted by the contig order of REF.fa.fai and by position, written as
BGZF with a tabix index (OUT.vcf.gz.tbi) beside it; an --out_fn that ends in .vcf is written as plain text without an
index.  vcf_merge.py holds the definition; CV_VCF_MERGE=device runs the sort, the gather and the index tables on the GPU.
"""
import argparse
import sys

from . import vcf_merge


def build_parser():
    parser = argparse.ArgumentParser(description="Merge chunk VCFs into one sorted, BGZF-compressed, tabix-indexed VCF")
    parser.add_argument("--vcf_fn", type=str, default=None, help="Input VCF files, separated by commas, in the order given")
    parser.add_argument("--vcf_glob", type=str, default=None, help="Input VCF files as a glob pattern (quote it)")
    parser.add_argument("--ref_fn", type=str, default=None,
                        help="Reference fasta: REF.fai gives the contig order, default: the header's ##contig lines")
    parser.add_argument("--out_fn", type=str, default=None, help="Output file, .vcf.gz (BGZF + .tbi) or .vcf (plain text)")
    parser.add_argument("--block", type=int, default=None, help="Uncompressed bytes per BGZF member, default: 65280")
    parser.add_argument("--threads", type=int, default=None, help="Members compressed at a time, default: min(16, usable cores)")
    return parser


def Run(args):
    if (args.vcf_fn is None) == (args.vcf_glob is None):
        sys.exit("Error: give one of --vcf_fn and --vcf_glob")
    if args.out_fn is None:
        sys.exit("Error: --out_fn is required")
    files = args.vcf_fn.split(",") if args.vcf_fn is not None else vcf_merge.chunk_files(args.vcf_glob)
    files = [f for f in files if f != args.out_fn]
    if not files:
        sys.exit("Error: no input VCF found")
    return vcf_merge.merge(files, args.out_fn, fai_fn=args.ref_fn + ".fai" if args.ref_fn else None, block=args.block,
                           threads=args.threads)


def main():
    parser = build_parser()
    args = parser.parse_args()
    if not sys.argv[1:]:
        parser.print_help()
        sys.exit(1)
    Run(args)


if __name__ == "__main__":
    main()
