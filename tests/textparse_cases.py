"""Inputs and the host checker shared by tests/test_gpu_text_parse.py and tests/test_text_parse_device_host.py: text
tensor files in the producer's format (CreateTensor.py:56) and out of it, cv_parse_tensor_text with one thread, and a
stand-in for the device side of utils_v2.GetTensorDevice that marks every line HOST."""
import ctypes
import functools
import gzip
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NV = 528
SKIP, ROW, HOST = 0, 1, 2
LINE_CAP = 8192


def golden_text(which):
    return gzip.open(os.path.join(GOLD, "gettensor_%s.txt.gz" % which), "rb").read()


def host_parse(text, max_rows=None):
    """cv_parse_tensor_text, one thread -> (consumed, bad, X [rows,528], meta [rows,6])"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    lib.cv_set_host_threads(1)
    if max_rows is None:
        max_rows = text.count(b"\n") + 1
    x = np.zeros((max_rows, NV), dtype=np.float32); meta = np.zeros((max_rows, 6), dtype=np.int64)
    c = ctypes.c_int64(); r = ctypes.c_int64(); b = ctypes.c_int64()
    _lib.check(lib.cv_parse_tensor_text(text, len(text), max_rows, x.ctypes.data_as(ctypes.c_void_p),
                                        meta.ctypes.data_as(ctypes.c_void_p), ctypes.byref(c), ctypes.byref(r), ctypes.byref(b)))
    return c.value, b.value, x[:r.value].copy(), meta[:r.value].copy()


def _vocabulary():
    """value tokens written with "%0.1f": negatives, -0.0, one- to nine-digit integers, every tenth .0 ... .9"""
    vals = [0.0, -0.0]
    for digits in range(1, 10):
        lo = 10 ** (digits - 1)
        for tenth in range(10):
            v = float(lo + (7 * tenth * lo) // 10 % (9 * lo)) + tenth / 10.0
            vals += [v, -v]
    vals += [float(v) for v in range(0, 60)] * 4            # most of a real file is small counts
    tok = ["%0.1f" % v for v in vals]
    assert "-0.0" in tok and any(len(t) == 11 and t[0] != "-" for t in tok) and {t[-1] for t in tok} == set("0123456789")
    return np.array(tok, dtype=object)


def good_row(rng, vocab, i, seq=None, ctg=None):
    if seq is None:
        seq = "".join("ACGT"[k] for k in rng.randint(0, 4, 33))
    return "%s %d %s %s" % (ctg or "chr%d" % (i % 3), 1000 + i, seq, " ".join(vocab[rng.randint(0, len(vocab), NV)]))


@functools.lru_cache(maxsize=2)
def volume_text(n=70000, seed=3):
    """>= 70 000 lines in the producer's format; lower-case and N centre bases, sequences of 16 and 17 bases, blank
    lines.  -> bytes"""
    rng = np.random.RandomState(seed)
    vocab = _vocabulary()
    lines = []
    for i in range(n):
        seq = "".join("ACGT"[k] for k in rng.randint(0, 4, 33))
        if i % 97 == 5:
            seq = seq[:16] + "N" + seq[17:]                  # dropped: centre base
        if i % 211 == 7:
            seq = seq.lower()                                # kept: upper-cased before the test
        if i % 389 == 11:
            seq = seq[:16]                                   # dropped: no centre base
        if i % 401 == 13:
            seq = seq[:17]                                   # kept: the centre base is its last
        lines.append(good_row(rng, vocab, i, seq))
        if i % 500 == 3:
            lines.append("")
    return ("\n".join(lines) + "\n").encode()


def off_format_lines(seed=5):
    """-> [(line bytes without newline, status the device must give it)]: every kind of line that is not in the
    producer's format on a line of its own among good rows, and the edge cases that are in the format"""
    rng = np.random.RandomState(seed)
    vocab = _vocabulary()
    n = [0]

    def good(**kw):
        n[0] += 1
        return good_row(rng, vocab, n[0], **kw)

    def with_value(tok, at=100):
        f = good().split(" ")
        f[3 + at] = tok
        return " ".join(f)

    out = []

    def add(line, status):
        out.append((good().encode(), ROW))
        out.append((line if isinstance(line, bytes) else line.encode(), status))

    add(good().replace(" ", "\t", 2), HOST)                   # tabs between the header tokens
    add(good() + "\r", HOST)                                  # CR in front of the newline
    add(good().replace(" ", "  ", 1), HOST)                   # double blank in the header
    f = good().split(" "); add(" ".join(f[:200]) + " " + " ".join(f[200:]).replace(" ", "  ", 1), HOST)   # ... among the values
    add(" " + good(), HOST)                                   # leading blank
    add(good() + " ", HOST)                                   # trailing blank
    for tok in ("+5", "1e1", "nan", ".5", "5.", "1.25", "1234567890", "1234567890.5", "-", "--1", "1-", "0x10", "inf", "1,5"):
        add(with_value(tok), HOST)
        add(with_value(tok, at=527), HOST)
    add(with_value("123456789.9"), ROW)                       # nine digits: in the format
    add(with_value("-000000000.0"), ROW)
    add(good().rsplit(" ", 1)[0], HOST)                       # 527 values
    add(good() + " 1.0", HOST)                                # 529 values
    add("chr1 100", HOST)                                     # fewer than three header tokens
    add("chr1", HOST)
    add("   ", HOST)                                          # blanks only: the host calls it a blank line
    add("", SKIP)
    add(good(seq="ACGTACGTACGTACGTNACGTACGTACGTACGTA"), SKIP)
    add(good(seq="acgtacgtacgtacgtaacgtacgtacgtacgta"), ROW)
    add(b"x" * (1 << 20), HOST)                               # 1 MB without blanks
    base = good(ctg="c")
    add("c" * (LINE_CAP - len(base)) + base, ROW)             # a long contig name: a line at the cap ...
    add("c" * (LINE_CAP + 1 - len(base)) + base, HOST)        # ... and one byte over
    g = good().encode(); add(b"ch\x00r" + g[4:], ROW)         # NUL and 0xFF in header tokens: bytes of the token
    g = good().encode(); add(b"\xffhr" + g[3:], ROW)
    f = good().encode().split(b" "); f[2] = f[2][:5] + b"\x00\xff" + f[2][7:]; add(b" ".join(f), ROW)
    assert len(out[-9][0]) == LINE_CAP and len(out[-7][0]) == LINE_CAP + 1
    return out


def off_format_text():
    lines = off_format_lines()
    return b"\n".join(l for l, _s in lines) + b"\n", np.array([s for _l, s in lines], dtype=np.uint8)


def blank_then_rows_text(nblank=10000, nrows=300, seed=9):
    rng = np.random.RandomState(seed)
    vocab = _vocabulary()
    return b"\n" * nblank + ("\n".join(good_row(rng, vocab, i) for i in range(nrows)) + "\n").encode()


def collect(batches):
    """-> (X [rows,528] as uint32 bits, [(ctg, pos, seq) bytes], end flags, batch sizes) of a GetTensor-like generator"""
    xs, pos, flags, sizes = [], [], [], []
    for end, c, x, p in batches:
        x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        assert x.shape[0] == c == len(p)
        xs.append(np.ascontiguousarray(x, dtype=np.float32).reshape(c, NV).view(np.uint32))
        for _s, rows, buf, meta in p.pieces():
            for m in meta[:rows]:
                pos.append(tuple(bytes(buf[m[2 * k]:m[2 * k] + m[2 * k + 1]]) for k in range(3)))
        flags.append(end); sizes.append(c)
    return (np.concatenate(xs) if xs else np.zeros((0, NV), np.uint32)), pos, flags, sizes


class AllHostDevice(object):
    """Stand-in for utils_v2._TextSlabDevice without a GPU: indexes the lines, marks EVERY one HOST, parses and copies
    nothing -- the worst case of GetTensorDevice's fallback."""

    def __init__(self, device, cap):
        self.cap = cap

    def upload(self, slab):
        return slab

    def parse(self, up, start):
        text = up[start:]
        ends = np.flatnonzero(text == 10)[:self.cap]
        lines = len(ends)
        info = np.array([ends[-1] + 1 if lines else 0, lines, 0, lines], dtype=np.int64)
        return {"x": np.full((self.cap, NV), np.nan, dtype=np.float32), "info": info,
                "status": np.full(lines, HOST, dtype=np.uint8), "meta": np.full((lines, 6), -1, dtype=np.int64)}

    def collect(self, job):
        return job["info"], job["status"], job["meta"]

    def patch(self, job, slots, rows):
        job["x"][slots] = rows

    def rows(self, job, lines, index):
        x = job["x"][:lines] if index is None else job["x"][index]
        return x.reshape(-1, 33, 4, 4)

    def empty(self):
        return np.zeros((0, 33, 4, 4), dtype=np.float32)
