"""Count the lines of a file that lie in the BED regions: command line and log lines of
/root/reference/dataPrepScripts/CountNumInBed.py (Calc :13-48, main :51-67).

    python -m clairvoyante_amd.CountNumInBed --input_fn ITEMS --bed_fn REGIONS.bed

Logs "Total: %d, Overlapped: %d, Percentage: %.3f" (:48); an empty input divides by zero there, as in the reference.
bed_items.count_items_host is the loop; with CV_BED_ITEMS=device the lines are tested on the GPU and only the two counters
come back (csrc/cv_beditems_dev.hip).  The reference as shipped does not run (it never imports subprocess and shlex, :17).
"""
import logging
import sys

if __package__ in (None, ""):      # run as `python <dir>/CountNumInBed.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import bed_items


def Calc(args):
    logging.info("Loading BED file ...")
    logging.info("Counting number of records in bed regions ...")
    a, o = bed_items.count_items(args.input_fn, args.bed_fn)
    logging.info("Total: %d, Overlapped: %d, Percentage: %.3f" % (a, o, float(o) / a * 100))


def Run(args):
    Calc(args)


_CLI = (
    ("--input_fn", str, None, "Input with 1st column as contig name and 2nd column as position"),
    ("--bed_fn", str, None, "High confident genome regions input in the BED format"),
)


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Calculate the number of variants in the bed regions")
    for flag, typ, default, text in _CLI:
        parser.add_argument(flag, type=typ, default=default, help=text)
    return parser


def main():
    logging.basicConfig(format="%(message)s", level=logging.INFO)
    parser = build_parser()
    args = parser.parse_args()
    if not sys.argv[1:]:
        parser.print_help()
        sys.exit(1)
    Run(args)


if __name__ == "__main__":
    main()
