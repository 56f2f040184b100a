"""Tensor generation from a sorted BAM and a candidate list: command line, inputs and output rows of
/root/reference/dataPrepScripts/CreateTensor.py (GetCandidate :56-77, OutputAlnTensor :93-258,
main :261-308), computed on the GPU (clairvoyante_amd/pileup.py, csrc/cv_pileup.hip).

    python -m clairvoyante_amd.CreateTensor --bam_fn IN.bam --ref_fn REF.fa --can_fn CANDIDATES \
           --tensor_fn OUT.gz --ctgName chr21 [--ctgStart S --ctgEnd E]

Like the reference it shells out to `samtools faidx` for the reference window (ctgStart-1Mb ..
ctgEnd+1Mb, :99-104) and to `samtools view -F 2308` for the alignments (:128-130), reads candidates
from --can_fn (through `gzip -fdc`) or standard input, and writes one row per candidate that some
read reached: "<ctg> <pos> <33 reference bases> <528 counts %0.1f>" (:52), to `gzip -c > tensor_fn`
or standard output; with --bgzf (not in the reference) the file is written as BGZF members instead, the form callVar
inflates on the GPU.  Differences: candidates are read completely before the alignments are streamed
(the reference interleaves the two, :160-162) and rows come out in ascending position order (the
reference: dict order, :232-246).  `pileup_region()` returns the tensors in HBM instead of text --
callVarBam feeds them to the network without the text round trip.
"""
import argparse
import shlex
import subprocess
import sys

import numpy as np

if __package__ in (None, ""):      # run as `python <dir>/CreateTensor.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import param
from .pileup import FLANK, Pileup, format_row_blocks

EXPAND = 1000000          # dataPrepScripts/param.py:3 expandReferenceRegion
READ_CHUNK = 8 << 20


def region_of(args):
    """CreateTensor.py:99-109: (ctgStart 1-based, ctgEnd, refStart, refEnd) or four None"""
    if args.ctgStart is not None and args.ctgEnd is not None:
        cs = args.ctgStart + 1
        return cs, args.ctgEnd, max(cs - EXPAND, 1), args.ctgEnd + EXPAND
    return None, None, None, None


def load_reference(args, refStart, refEnd):
    if args.samtools == "native":                       # REF.fai + a seek instead of `samtools faidx`
        from .bam import faidx
        seq = faidx(args.ref_fn, args.ctgName, refStart, refEnd)
        if len(seq) == 0:
            sys.stderr.write("Failed to load reference seqeunce. Please check if the provided reference fasta %s and the "
                             "ctgName %s are correct.\n" % (args.ref_fn, args.ctgName))
            sys.exit(1)
        return seq
    where = args.ctgName if refStart is None else "%s:%d-%d" % (args.ctgName, refStart, refEnd)
    p = subprocess.Popen(shlex.split("%s faidx %s %s" % (args.samtools, args.ref_fn, where)), stdout=subprocess.PIPE,
                         bufsize=8388608)
    out = p.stdout.read()
    p.stdout.close()
    p.wait()
    lines = out.split(b"\n")
    seq = b"".join(l.rstrip() for l in lines[1:])
    if p.returncode != 0 or len(seq) == 0:
        sys.stderr.write("Failed to load reference seqeunce. Please check if the provided reference fasta %s and the "
                         "ctgName %s are correct.\n" % (args.ref_fn, args.ctgName))
        sys.exit(1)
    return seq


_CAN_KEYS = ("host_calls", "device_calls", "handed_over_calls", "device_lines")
_can_counts = dict.fromkeys(_CAN_KEYS, 0)
CAN_TIMES = None                    # the probe: a dict that receives the milliseconds of the device calls by name (HIP events)


def candidate_list_counts(reset=False):
    """calls of read_candidates per side so far, the calls the device route began and gave to the host loop, and the lines
    the device read"""
    out = dict(_can_counts)
    if reset:
        _can_counts.update(dict.fromkeys(_CAN_KEYS, 0))
    return out


def candidate_list_route(can_fn):
    """"host" or "device": CV_CANDIDATE_LIST when it is set (any other value raises), else the host; PIPE and a run
    without a GPU are always "host" """
    import os
    forced = os.environ.get("CV_CANDIDATE_LIST")
    if forced not in (None, "", "host", "device"):
        raise ValueError("CV_CANDIDATE_LIST must be 'host' or 'device', got %r" % forced)
    if forced != "device" or can_fn == "PIPE":
        return "host"
    from .utils_v2 import _gpu_present
    return "device" if _gpu_present() else "host"


def read_candidates(args, ctgStart, ctgEnd):
    """GetCandidate :56-62: 1-based positions of this contig inside [ctgStart, ctgEnd], ascending and unique -- by the
    host loop read_candidates_host (the definition), or with CV_CANDIDATE_LIST=device by the device's line pass
    (read_candidates_device), which hands the whole call to the host loop when it meets a line it does not vouch for"""
    if candidate_list_route(args.can_fn) == "device":
        from .utils_v2 import _TruthHandOver
        try:
            got = read_candidates_device(args, ctgStart, ctgEnd)
            _can_counts["device_calls"] += 1
            return got
        except _TruthHandOver:
            _can_counts["handed_over_calls"] += 1
    _can_counts["host_calls"] += 1
    return read_candidates_host(args, ctgStart, ctgEnd)


def read_candidates_device(args, ctgStart, ctgEnd, device=None):
    """read_candidates on the device: the file in slabs through utils_v2._SlabWalk (plain text memory-mapped, BGZF
    inflated on the device, an ordinary .gz inflated natively on the host), cv_item_lines_dev for position, contig run
    and the run-start tokens, which the host compares with --ctgName; the positions of the contig's runs inside the
    bounds are kept on the device, sorted and made unique there.  Raises utils_v2._TruthHandOver for a file or a line
    only the host loop answers (a blank line, one token, "007", "+5", "1_0", '\\r', a byte outside printable ASCII)."""
    import ctypes
    import torch
    from . import _lib, utils_v2
    from .utils_v2 import _SlabWalk, _TruthHandOver, _TruthReader, _truth_chunks, _while_table_full
    device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
    name = args.ctgName.encode()
    kept = []
    with torch.cuda.device(device):
        rd = _TruthReader(device)
        lib, st, P = rd.lib, _lib.stream_arg(device), _lib.ptr
        E = lambda n, dt=torch.int64: torch.empty(n, dtype=dt, device=device)
        state = {"bytes_per_line": 16.0}

        def slab(buf, lo, hi, _padded_end):
            def line_pass(at, n, max_lines):
                need = _lib.workspace(lib.cv_item_lines_workspace, n, max_lines)
                ws = E(need, torch.uint8)
                pos, run, off, ln = E(max_lines), E(max_lines, torch.int32), E(max_lines), E(max_lines)
                tok, info_dev = E((max_lines, 2)), E(8)
                if CAN_TIMES is not None:
                    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                    ev[0].record()
                _lib.check(lib.cv_item_lines_dev(ctypes.c_void_p(buf.data_ptr() + at), n, max_lines, P(pos), P(run), P(off), P(ln),
                                                 P(tok), P(info_dev), P(ws), need, st))
                if CAN_TIMES is not None:
                    ev[1].record()
                used, lines, rows, _skipped, host, runs = info_dev.cpu().tolist()[:6]
                if CAN_TIMES is not None:
                    CAN_TIMES["lines"] = CAN_TIMES.get("lines", 0.0) + ev[0].elapsed_time(ev[1])
                if host:
                    raise _TruthHandOver("%d line(s) only the host loop defines the result for" % host)
                if rows:
                    # which runs are the contig's: the host compares their start tokens
                    mine = [t == name for t in rd.run_names(buf, at, n, tok, runs)]
                    if any(mine):
                        p = pos[:rows]
                        keep = torch.tensor(mine, dtype=torch.bool, device=device)[run[:rows].long()]
                        if ctgStart is not None:
                            keep &= p >= ctgStart
                        if ctgEnd is not None:
                            keep &= p <= ctgEnd
                        kept.append(p[keep])
                _can_counts["device_lines"] += lines
                if lines:
                    state["bytes_per_line"] = max(used / float(lines), 2.0)
                return used, lines

            return _while_table_full(lo, hi, lambda n: min(int(n / state["bytes_per_line"] * 1.25) + 1024, n), line_pass)

        slab_bytes = max(int(utils_v2.TRUTH_SLAB_BYTES), 1)
        walk = _SlabWalk(torch, device, _truth_chunks(args.can_fn, slab_bytes), slab_bytes, rd._inflate, pad_always=False,
                         join_unbroken=True, whole_lines=True)
        walk.run(slab)
        if not kept:
            return np.zeros(0, dtype=np.int64)
        return torch.unique(torch.cat(kept), sorted=True).cpu().numpy()


def read_candidates_host(args, ctgStart, ctgEnd):
    """GetCandidate :56-62: 1-based positions of this contig inside [ctgStart, ctgEnd]"""
    if args.can_fn != "PIPE":
        f = subprocess.Popen(shlex.split("gzip -fdc %s" % args.can_fn), stdout=subprocess.PIPE, bufsize=8388608)
        fo = f.stdout
    else:
        f = None
        fo = sys.stdin.buffer
    name = args.ctgName.encode()
    pos = []
    for row in fo:
        row = row.split()
        if not row or row[0] != name:
            continue
        p = int(row[1])
        if ctgStart is not None and p < ctgStart:
            continue
        if ctgEnd is not None and p > ctgEnd:
            continue
        pos.append(p)
    if f is not None:
        fo.close()
        f.wait()
    return np.unique(np.asarray(pos, dtype=np.int64))


def pileup_region(args, subtract=False, device=None):
    """-> dict(centers [k] int64, tensors [k,33,4,4] fp32 on the device, ref_seq bytes, shift, stats) for the
    candidates that get a row (reached by a read, window inside the loaded reference, centre depth >=
    minCoverage; :50-51)."""
    import torch
    ctgStart, ctgEnd, refStart, refEnd = region_of(args)
    ref_seq = load_reference(args, refStart, refEnd)
    shift = 0 if refStart is None else refStart - 1
    centers = read_candidates(args, ctgStart, ctgEnd)
    pl = Pileup(device=device, minMQ=args.minMQ, dcov=args.dcov, considerleftedge=args.considerleftedge)
    pl.set_reference(ref_seq, shift)
    pl.set_candidates(centers)
    from .ExtractVariantCandidates import stream_alignments
    stream_alignments(args, pl, ctgStart, ctgEnd)
    t, depth, touched = pl.finish(subtract=subtract)
    inside = torch.from_numpy((pl.centers - shift - (FLANK + 1)) >= 0).to(t.device)
    keep = touched & inside & (depth >= args.minCoverage)
    idx = torch.nonzero(keep).squeeze(1)
    out = {"centers": pl.centers[idx.cpu().numpy()], "tensors": t.index_select(0, idx), "ref_seq": ref_seq,
           "shift": shift, "stats": pl.stats(), "reads": pl.reads_kept}
    pl.close()
    return out


class TensorStdout(object):
    def __init__(self, handle):
        self.stdin = handle


def OutputAlnTensor(args):
    res = pileup_region(args, subtract=False)
    bgzf = None
    if args.tensor_fn != "PIPE" and getattr(args, "bgzf", False):      # the same text as BGZF members (utils_v2.BgzfWriter)
        from .utils_v2 import BgzfWriter
        bgzf = BgzfWriter(args.tensor_fn)
        fpo, fp = None, TensorStdout(bgzf)
    elif args.tensor_fn != "PIPE":
        fpo = open(args.tensor_fn, "wb")
        fp = subprocess.Popen(shlex.split("gzip -c"), stdin=subprocess.PIPE, stdout=fpo, stderr=sys.stderr,
                              bufsize=8388608)
    else:
        fpo = None
        fp = TensorStdout(sys.stdout.buffer)
    # the rows are made on the device, one block and one write per 32 768 of them, or by format_rows on the host, row by
    # row (pileup.format_row_blocks: CV_ROW_FORMAT, else pileup.ROWTEXT_DEVICE_MIN_ROWS) -- the same bytes either way
    # With the device BGZF writer (CV_BGZF_DEFLATE=device) a block the kernel printed stays in HBM and is compressed there.
    in_hbm = bgzf is not None and bgzf.deflate == "device"
    for block in format_row_blocks(args.ctgName, res["centers"], res["ref_seq"], res["shift"], res["tensors"], in_hbm=in_hbm):
        bgzf.write_device(block) if hasattr(block, "is_cuda") else fp.stdin.write(block)
    if bgzf is not None:
        bgzf.close()
    elif fpo is not None:
        fp.stdin.close()
        fp.wait()
        fpo.close()
    else:
        fp.stdin.flush()
    return res


_CLI = (
    ("--bam_fn", str, "input.bam", "Sorted bam file input, default: %(default)s"),
    ("--ref_fn", str, "ref.fa", "Reference fasta file input, default: %(default)s"),
    ("--can_fn", str, "PIPE", "Variant candidate list generated by ExtractVariantCandidates.py or true variant list "
                              "generated by GetTruth.py, use PIPE for standard input, default: %(default)s"),
    ("--tensor_fn", str, "PIPE", "Tensor output, use PIPE for standard output, default: %(default)s"),
    ("--minMQ", int, 0, "Minimum Mapping Quality. Mapping quality lower than the setting will be filtered, "
                        "default: %(default)d"),
    ("--ctgName", str, "chr17", "The name of sequence to be processed, default: %(default)s"),
    ("--ctgStart", int, None, "The 1-bsae starting position of the sequence to be processed"),
    ("--ctgEnd", int, None, "The inclusive ending position of the sequence to be processed"),
    ("--samtools", str, "samtools", "Path to the 'samtools', default: %(default)s"),
    ("--dcov", int, 250, "Cap depth per position at %(default)d"),
    ("--minCoverage", int, 0, "Minimum coverage required to generate a tensor, default: %(default)d"),
)


def build_parser():
    parser = argparse.ArgumentParser(description="Generate tensors summarizing local alignments from a BAM file and "
                                                 "a list of candidate locations")
    for flag, typ, default, text in _CLI:
        parser.add_argument(flag, type=typ, default=default, help=text)
    parser.add_argument("--considerleftedge", type=param.str2bool, nargs="?", const=True, default=True,
                        help="Count the left-most base-pairs of a read for coverage even if the starting position of "
                             "a read is after the starting position of a tensor, default: %(default)s")
    parser.add_argument("--bgzf", type=param.str2bool, nargs="?", const=True, default=False,
                        help="Write --tensor_fn as BGZF (independent gzip members, as bgzip writes them; any gzip reads "
                             "it, callVar inflates it on the GPU) instead of through `gzip -c`, default: %(default)s")
    return parser


def main():
    parser = build_parser()
    args = parser.parse_args()
    if not sys.argv[1:]:
        parser.print_help()
        sys.exit(1)
    OutputAlnTensor(args)


if __name__ == "__main__":
    main()
