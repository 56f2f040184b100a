"""Pairs the truth-variant tensors with a share of the non-variant tensors: command line, inputs, output rows and log
lines of /root/reference/dataPrepScripts/PairWithNonVariants.py (Pair :33-128), plus --seed.

    python -m clairvoyante_amd.PairWithNonVariants --tensor_can_fn CAN.gz --tensor_var_fn VAR.gz --bed_fn B.bed \
           --output_fn MIX.gz --amp 2 [--seed N]

All rows of --tensor_var_fn are written; a row of --tensor_can_fn is usable when the BED covers it (when there is one)
and no truth row has its contig and position; of the usable ones the share r = min(1, amp * v / c) is written.  The
reference picks them with Python's unseeded generator in file order (:119); here a row is kept when its keyed draw
(clairvoyante_amd/draws.py, stream PAIR: a function of seed, contig and position alone) is below r, so the same seed
gives the same file and the device route of utils_v2.GetTrainingSetFromBam, which is held to this loop, the same set.
Deliberate deviation: with no usable non-variant (c == 0) r is 1, where the reference divides by zero (:88).

Pair_host(args, seed=None) is that loop, callable on its own; Pair resolves the seed and runs it.  --bgzf (not in the
reference) writes --output_fn as BGZF through utils_v2.BgzfWriter instead of the `gzip -c` child: the same bytes once
inflated, and a file the device training-set builder takes (tensor2Bin --tensor_fn), which an ordinary .gz never is.

CV_PAIR=device (opt-in; unset or "host": the loop, as ever) runs the step on the GPU from kernels the other tools own
(bed_items._PairWalk): the same file once inflated, the same dict and the same log lines.  A line whose raw bytes are not
row.strip() + "\n", or that only int() and split() can judge, sends the whole call to Pair_host before a byte is written.
counts() says what ran where.
"""
import argparse
import logging
import os
import shlex
import subprocess
import sys

if __package__ in (None, ""):      # run as `python <dir>/PairWithNonVariants.py` (the reference's way): make the package importable
    import os as _os, sys as _sys
    _sys.path[0] = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
    import clairvoyante_amd  # noqa: F401
    __package__ = "clairvoyante_amd"
from . import draws, param

logging.basicConfig(format='%(message)s', level=logging.INFO)


def _rows(fn):
    f = subprocess.Popen(shlex.split("gzip -fdc %s" % fn), stdout=subprocess.PIPE, bufsize=8388608)
    for row in f.stdout:
        yield row.strip()
    f.stdout.close()
    f.wait()


def _usable(args, tree, truth):
    """(raw row, contig, position) of the rows of --tensor_can_fn the pairing may pick (:106-118)"""
    for raw in _rows(args.tensor_can_fn):
        row = raw.split()
        if not row:
            continue
        ctg, pos = row[0].decode(), int(row[1])
        if args.bed_fn is not None and (ctg not in tree or not tree[ctg].hit(pos)):
            continue
        if (ctg, pos) in truth:
            continue
        yield raw, ctg, pos


class _Output(object):
    """--output_fn: BGZF members with --bgzf (utils_v2.BgzfWriter), else the `gzip -c` child"""

    def __init__(self, args):
        self.bgzf = self.fpo = self.fh = self.pinned = None
        if getattr(args, "bgzf", False):
            from .utils_v2 import BgzfWriter
            self.bgzf = BgzfWriter(args.output_fn)
            self.write = self.bgzf.write
        else:
            self.fpo = open(args.output_fn, "wb")
            self.fh = subprocess.Popen(shlex.split("gzip -c"), stdin=subprocess.PIPE, stdout=self.fpo, stderr=sys.stderr, bufsize=8388608)
            self.write = self.fh.stdin.write

    def write_device(self, text):
        """a uint8 tensor in HBM (the device route's gathered lines).  --bgzf with CV_BGZF_DEFLATE=device compresses it
        where it lies; else one pinned copy brings it over for write()"""
        if self.bgzf is not None and self.bgzf.deflate == "device":
            return self.bgzf.write_device(text)
        import torch
        n = int(text.numel())
        if self.pinned is None or self.pinned.numel() < n:
            self.pinned = torch.empty(max(n, 1 << 20), dtype=torch.uint8).pin_memory()
        self.pinned[:n].copy_(text)
        self.write(self.pinned[:n].numpy().data)

    def close(self, failed=False):
        """failed: the loop raised -- the file stays cut short, and a BGZF one gets no end marker that would hide it"""
        if self.bgzf is not None:
            self.bgzf.close(abandon=failed)
        else:
            self.fh.stdin.close()
            self.fh.wait()
            self.fpo.close()


def Pair_host(args, seed=None):
    """the loop that defines the result (the reference's, with the keyed draws); seed None: resolved here as Pair does"""
    from .utils_v2 import _Intervals
    if seed is None:
        seed = draws.resolve_seed(getattr(args, "seed", None), "PairWithNonVariants")
    tree = {}
    if args.bed_fn is not None:
        logging.info("Loading BED file ...")
        for row in _rows(args.bed_fn):
            row = row.split()
            if not row:
                continue
            begin, end = int(row[1]), int(row[2]) - 1
            if end == begin:
                end += 1
            tree.setdefault(row[0].decode(), _Intervals()).addi(begin, end)

    logging.info("Counting the number of Truth Variants in %s ..." % args.tensor_var_fn)
    v = 0
    truth = set()
    for row in _rows(args.tensor_var_fn):
        row = row.split()
        if not row:
            continue
        v += 1
        truth.add((row[0].decode(), int(row[1])))
    logging.info("%d Truth Variants" % v)
    t = v * args.amp
    logging.info("%d non-variants to be picked" % t)

    logging.info("Counting the number of usable non-variants in %s ..." % args.tensor_can_fn)
    c = sum(1 for _ in _usable(args, tree, truth))
    logging.info("%d usable non-variant" % c)
    r = float(t) / c if c else 1.0
    r = r if r <= 1 else 1
    logging.info("%.2f of all non-variants are selected" % r)

    o1 = o2 = 0
    out = _Output(args)
    try:
        for row in _rows(args.tensor_var_fn):
            out.write(row)
            out.write(b"\n")
            o1 += 1
        batch = []

        def drain():
            n = 0
            by_ctg = {}
            for k, (_raw, ctg, pos) in enumerate(batch):
                by_ctg.setdefault(ctg, []).append(k)
            keep = [False] * len(batch)
            for ctg, ks in by_ctg.items():
                u = draws.draws(seed, draws.PAIR, ctg, [batch[k][2] for k in ks])
                for k, uk in zip(ks, u):
                    keep[k] = uk < r
            for k, (raw, _ctg, _pos) in enumerate(batch):
                if keep[k]:
                    out.write(raw)
                    out.write(b"\n")
                    n += 1
            del batch[:]
            return n

        for item in _usable(args, tree, truth):
            batch.append(item)
            if len(batch) >= 65536:
                o2 += drain()
        o2 += drain()
    except BaseException:
        out.close(failed=True)                               # (the child reaped, the handles closed; no BGZF end marker)
        raise
    out.close()
    logging.info("%.2f/%.2f Truth Variants/Non-variants outputed" % (o1, o2))
    return {"v": v, "c": c, "r": r, "o1": o1, "o2": o2, "seed": seed}


_COUNT_KEYS = ("device_calls", "host_calls", "handed_over_calls", "device_lines_bed", "device_lines_var", "device_lines_can")
_counts = dict.fromkeys(_COUNT_KEYS, 0)


def counts(reset=False):
    """what ran where so far: calls the device route finished, calls the loop ran (handed_over_calls of them begun by the
    device route), and the lines the device read per file in the calls it finished (of the BED: its intervals)"""
    out = dict(_counts)
    if reset:
        _counts.update(dict.fromkeys(_COUNT_KEYS, 0))
    return out


def route():
    """"host" or "device": CV_PAIR (unset or "host": the loop; "device": the GPU; anything else raises); always "host"
    without a GPU.  No floor is set: nothing about this step's time makes the device the default (tools/gpu_pair_probe.py)"""
    forced = os.environ.get("CV_PAIR")
    if forced not in (None, "", "host", "device"):
        raise ValueError("CV_PAIR must be 'host' or 'device', got %r" % forced)
    if forced != "device":
        return "host"
    from .utils_v2 import _gpu_present
    return "device" if _gpu_present() else "host"


def _pair_device(args, seed):
    """Pair_host's file, dict and log lines from the device (bed_items._PairWalk) -> the dict, or None: a line only the
    loop answers, met before anything was logged or written -- the whole call is Pair_host's"""
    import torch
    from . import bed_items
    from .utils_v2 import _TruthHandOver
    device = torch.device("cuda:%d" % torch.cuda.current_device())
    with torch.cuda.device(device):
        try:
            w = bed_items._PairWalk(device, args.bed_fn)
            v = w.count_variants(args.tensor_var_fn)
            w.count_candidates(args.tensor_can_fn)
            got_v, c, r_dev, picked = w.pair(seed, args.amp)
        except _TruthHandOver:
            return None
        t = v * args.amp
        r = float(t) / c if c else 1.0
        r = r if r <= 1 else 1
        if got_v != v or float(r) != r_dev:
            raise RuntimeError("PairWithNonVariants: the device pairs %d variants at r = %r, the loop %d at %r" % (got_v, r_dev, v, r))
        if args.bed_fn is not None:
            logging.info("Loading BED file ...")
        logging.info("Counting the number of Truth Variants in %s ..." % args.tensor_var_fn)
        logging.info("%d Truth Variants" % v)
        logging.info("%d non-variants to be picked" % t)
        logging.info("Counting the number of usable non-variants in %s ..." % args.tensor_can_fn)
        logging.info("%d usable non-variant" % c)
        logging.info("%.2f of all non-variants are selected" % r)
        out = _Output(args)
        try:
            o1 = w.gather(w.var, w.keep[:v], out.write_device)
            o2 = w.gather(w.can, w.keep[v:], out.write_device)
            if (o1, o2) != (v, picked):
                raise RuntimeError("PairWithNonVariants: %d + %d lines written where %d + %d were paired" % (o1, o2, v, picked))
        except BaseException:
            out.close(failed=True)
            raise
        out.close()
    logging.info("%.2f/%.2f Truth Variants/Non-variants outputed" % (o1, o2))
    _counts["device_lines_bed"] += w.bed_lines
    _counts["device_lines_var"] += w.var.rows
    _counts["device_lines_can"] += w.can.rows
    return {"v": v, "c": c, "r": r, "o1": o1, "o2": o2, "seed": seed}


def Pair(args):
    """the tool's entry: the seed resolved once, then the loop, or with CV_PAIR=device the device route held to it"""
    how = route()
    seed = draws.resolve_seed(getattr(args, "seed", None), "PairWithNonVariants")
    if how == "device":
        got = _pair_device(args, seed)
        if got is not None:
            _counts["device_calls"] += 1
            return got
        _counts["handed_over_calls"] += 1
    _counts["host_calls"] += 1
    return Pair_host(args, seed)


def build_parser():
    parser = argparse.ArgumentParser(description="Pair the truth variants with non-variants")
    parser.add_argument('--tensor_can_fn', type=str, default=None,
                        help="Tensors generated at randome genome positions by ExtractVariantCandidates.py+CreateTensor.py")
    parser.add_argument('--tensor_var_fn', type=str, default=None, help="Variant tensors generated by GetTruth.py+CreateTensor.py")
    parser.add_argument('--bed_fn', type=str, default=None, help="Usable genome regions input in BED format")
    parser.add_argument('--output_fn', type=str, default=None, help="Tensors output filename")
    parser.add_argument('--amp', type=float, default=2,
                        help="Pick ((# of the Truth Variants)*amp) non-variants to pair with the Truth Variants, default: 2")
    parser.add_argument('--seed', type=int, default=None,
                        help="Seed of the keyed draws (repeatable output); default: 64 bits taken from Python's generator once")
    parser.add_argument('--bgzf', type=param.str2bool, nargs='?', const=True, default=False,
                        help="Write --output_fn as BGZF (the device readers downstream take it), default: an ordinary .gz")
    return parser


def main():
    parser = build_parser()
    args = parser.parse_args()
    if len(sys.argv[1:]) == 0:
        parser.print_help()
        sys.exit(1)
    Pair(args)


if __name__ == "__main__":
    main()
