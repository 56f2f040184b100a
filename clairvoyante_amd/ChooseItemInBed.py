"""Print the lines of a file that lie in the BED regions: command line and output of
/root/reference/dataPrepScripts/ChooseItemInBed.py (Calc :11-39, main :42-58).

    python -m clairvoyante_amd.ChooseItemInBed --input_fn ITEMS --bed_fn REGIONS.bed > KEPT

ITEMS is any file whose first two columns are contig and position (a text tensor, a truth list), plain or gzip; a line is
written unchanged when a BED interval [begin, end - 1) covers its position (:13-23, :30-36).  bed_items.choose_items_host
is the loop; with CV_BED_ITEMS=device the lines are tested and gathered on the GPU (csrc/cv_beditems_dev.hip) and the
bytes written are the same.  The reference as shipped does not run (it never imports shlex, :14).
"""
import sys

if __package__ in (None, ""):      # run as `python <dir>/ChooseItemInBed.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import bed_items


def Calc(args):
    out = sys.stdout.buffer
    try:
        bed_items.choose_items(args.input_fn, args.bed_fn, out)
    finally:
        out.flush()


def Run(args):
    Calc(args)


_CLI = (
    ("--input_fn", str, None, "Input with 1st column as contig name and 2nd column as position"),
    ("--bed_fn", str, None, "High confident genome regions input in the BED format"),
)


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Print the variants in the bed regions")
    for flag, typ, default, text in _CLI:
        parser.add_argument(flag, type=typ, default=default, help=text)
    return parser


def main():
    parser = build_parser()
    args = parser.parse_args()
    if not sys.argv[1:]:
        parser.print_help()
        sys.exit(1)
    Run(args)


if __name__ == "__main__":
    main()
