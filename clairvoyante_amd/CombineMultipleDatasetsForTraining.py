"""Combine the training inputs of several genomes: command line and outputs of
/root/reference/dataPrepScripts/CombineMultipleDatasetsForTraining.py (CombineDatasets :11-53, main :55-80).

    python -m clairvoyante_amd.CombineMultipleDatasetsForTraining --input_list LIST --tensor_can_out A --tensor_var_out B \
           --var_out C --bed_out D [--bgzf]

Every line of LIST names four files: tensors at random positions, variant tensors, truth variants, BED regions.  Each line
of the four files of dataset k gets the one-byte prefix chr(ord("a") + k) (:22, :29-47) -- the contigs of different genomes
become different contigs -- and goes to the four outputs through `gzip -c -1` (:13-20).  The prefix is put in whole blocks
at a time (bed_items.prefix_lines), not line by line.  A file whose last line has no newline is followed directly by the
next dataset's prefix and first line, as the reference's byte-wise writes leave it.  --bgzf (not in the reference) writes
the outputs as BGZF (utils_v2.BgzfWriter): the same bytes once inflated, in members the device readers downstream inflate
on the GPU.  Host only: there is nothing here for a kernel.
"""
import shlex
import subprocess
import sys

if __package__ in (None, ""):      # run as `python <dir>/CombineMultipleDatasetsForTraining.py`: make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import bed_items, param

BLOCK = 8388608                    # bytes per read of an input pipe


class _GzipOut(object):
    """:13-14: `gzip -c -1` into the file"""

    def __init__(self, fn):
        self.fpo = open(fn, "wb")
        self.fh = subprocess.Popen(shlex.split("gzip -c -1"), stdin=subprocess.PIPE, stdout=self.fpo, stderr=sys.stderr, bufsize=8388608)

    def write(self, data):
        self.fh.stdin.write(data)

    def close(self):
        self.fh.stdin.close()
        self.fh.wait()
        self.fpo.close()


def _open_out(fn, bgzf):
    if bgzf:
        from .utils_v2 import BgzfWriter
        return BgzfWriter(fn, level=1)
    return _GzipOut(fn)


def _combine_one(fn, prefix, out):
    """:28-30: every row of `gzip -fdc fn` behind the prefix"""
    sys.stderr.write("Combining %s ...\n" % fn)
    f = subprocess.Popen(shlex.split("gzip -fdc %s" % fn), stdout=subprocess.PIPE, bufsize=8388608)
    at_line_start = True
    while True:
        block = f.stdout.read(BLOCK)
        if not block:
            break
        data, at_line_start = bed_items.prefix_lines(block, prefix, at_line_start)
        out.write(data)
    f.stdout.close()
    f.wait()


def CombineDatasets(args):
    bgzf = bool(getattr(args, "bgzf", False))
    outs = [_open_out(fn, bgzf) for fn in (args.tensor_can_out, args.tensor_var_out, args.var_out, args.bed_out)]
    prefix = ord("a")
    with open(args.input_list, "r") as l:
        for d in l:
            s = d.strip().split()
            for k in range(4):
                _combine_one(s[k], prefix, outs[k])
            prefix += 1
    for o in outs:
        o.close()


def Run(args):
    CombineDatasets(args)


_CLI = (
    ("--input_list", str, None, "A list with 4 columns of filenames. <Tensors generated at randome genome positions genearted by "
                                "ExtractVariantCandidates.py+CreateTensor.py> <Variant tensors generated GetTruth.py+CreateTensor.py> "
                                "<Truth variants genearted by GetTruth.py> <Usable genome regions in BED format>"),
    ("--tensor_can_out", str, None, "Combined tensors generated at randome genome positions"),
    ("--tensor_var_out", str, None, "Combined variant tensors output"),
    ("--var_out", str, None, "Combined Truth variants list output"),
    ("--bed_out", str, None, "Combined usable genome regions output"),
)


def build_parser():
    import argparse
    parser = argparse.ArgumentParser(description="Combine datasets for model training")
    for flag, typ, default, text in _CLI:
        parser.add_argument(flag, type=typ, default=default, help=text)
    parser.add_argument("--bgzf", type=param.str2bool, nargs="?", const=True, default=False,
                        help="Write the four outputs as BGZF (the same bytes once inflated), default: %(default)s")
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
