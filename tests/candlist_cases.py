"""Shared by test_candidate_list_host.py and test_gpu_candidate_rows.py: the arguments of the two commands over the golden
inputs, the hand-made candidate lists of the hand-over rules, and cv_candidate_rows_host_form through ctypes."""
import ctypes
import gzip
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from test_pileup_oracle import EVC_CASES, G, load_evc_case  # noqa: E402,F401

FAKE = "%s %s" % (sys.executable, os.path.join(HERE, "golden", "fake_samtools.py"))


def evc_args(aln, can_fn, **over):
    base = os.path.join(G, aln)
    a = dict(bam_fn=base + ".sam", ref_fn=base + ".fa", bed_fn=None, can_fn=str(can_fn), threshold=0.125, minCoverage=4,
             minMQ=0, gen4Training=False, candidates=7000000, genomeSize=3000000000, ctgName="ctgA", ctgStart=None,
             ctgEnd=None, samtools=FAKE, seed=None, bgzf=False)
    a.update(over)
    return types.SimpleNamespace(**a)


def golden_evc_args(name, can_fn, **over):
    aln, _, _, opts, _, want = load_evc_case(name)
    opts = dict(opts)
    meta = __import__("json").load(open(os.path.join(G, name + ".evc.args.json")))["options"]
    if "bed_fn" in meta:
        opts["bed_fn"] = os.path.join(G, meta["bed_fn"])
    opts.update(over)
    return evc_args(aln, can_fn, **opts), want


def can_args(can_fn, ctgName="ctgA"):
    return types.SimpleNamespace(can_fn=str(can_fn), ctgName=ctgName)


# one line of each kind the device does not vouch for, inside a list that is otherwise plain: (name, file bytes).  The
# host loop skips a blank line and a one-token line of another contig, and raises IndexError for the contig's own
HAND_OVER = [
    ("leading_zero", b"ctgA 5 x\nctgA 007 x\nctgA 9 x\n"),
    ("plus_sign", b"ctgA 5 x\nctgA +5 x\n"),
    ("underscore", b"ctgA 5 x\nctgA 1_0 x\nctgA 3\n"),
    ("carriage_return", b"ctgA 5 x\r\nctgA 6 x\r\n"),
    ("high_byte", b"ctgA 5 \xc3\xa9\nctgA 4 x\n"),
    ("tab_and_vt", b"ctgA\t5\x0bx\nctgA 4 x\n"),
    ("blank_line", b"ctgA 5 x\n\nctgA 4 x\n"),
    ("one_token_other_contig", b"ctgA 5 x\nctgB\nctgA 4 x\n"),
    ("one_token_own_contig", b"ctgA 5 x\nctgA\nctgA 4 x\n"),
    ("not_a_number_own_contig", b"ctgA 5 x\nctgA five x\n"),
    ("not_a_number_other_contig", b"ctgA 5 x\nctgB five x\nctgA 2 x\n"),
]
# lists the device takes whole: (name, file bytes)
PLAIN_LISTS = [
    ("empty", b""),
    ("duplicates", b"ctgA 7 x\nctgA 3 y\nctgA 7 z\nctgA 3 y\nctgA 12 A 1 2 3\n"),
    ("no_final_newline", b"ctgA 7 x\nctgA 3 y"),
    ("bounds", b"ctgA 99 x\nctgA 100 x\nctgA 101 x\nctgA 199 x\nctgA 200 x\nctgA 201 x\n"),
    ("three_contigs", b"".join(b"ctgA %d a\nctgB %d b\nctgAA %d c\n" % (p, p + 1, p + 2) for p in (50, 10, 50, 30, 10, 150, 120))),
    ("other_contig_only", b"ctgB 7 x\nctgB 8 x\n"),
]
ids = lambda cases: [name for name, _ in cases]
BOUNDS = [(None, None), (100, 200), (101, 199), (100, None), (None, 120), (300, 400)]


def outcome(fn, *args):
    """("ok", array) or ("raised", exception type)"""
    try:
        return "ok", fn(*args)
    except (IndexError, ValueError) as e:
        return "raised", type(e)


def same_outcome(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == "raised":
        return a[1] is b[1]
    return a[1].dtype == b[1].dtype == np.int64 and np.array_equal(a[1], b[1])


def host_form(ctg, order, pos0, counts7, ref, ref_first0, text_cap=None, late=None):
    """cv_candidate_rows_host_form -> (text bytes, off [rows + 1], status [rows]); text_cap None: exactly the bytes"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    pos0 = np.ascontiguousarray(pos0, dtype=np.int64)
    c7 = np.ascontiguousarray(counts7, dtype=np.int32).reshape(-1, 7)
    n = len(pos0)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
    rows = n if order is None else len(order)
    refa = np.frombuffer(bytes(ref) or b"\0", dtype=np.uint8)
    off = np.zeros(rows + 1, dtype=np.int64)
    status = np.zeros(max(rows, 1), dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    def call(text, cap):
        _lib.check(lib.cv_candidate_rows_host_form(ctg, len(ctg), P(order), rows, n, P(pos0), None, P(c7), P(refa), int(ref_first0),
                                                   len(ref), P(off), P(status), P(text), cap))
    call(None, 0)
    total = int(off[rows])
    cap = total if text_cap is None else text_cap
    text = np.full(total + 1, 0xEE, dtype=np.uint8)
    call(text, cap)
    assert text[total] == 0xEE
    return text[:total].tobytes(), off, status[:rows]


def parse_golden_rows(rows):
    """the rows of a golden candidate list -> (pos0 [n], counts [n,7] in A,C,G,T,I,D,N order, reference byte per row)"""
    pos0, c7, rb = [], [], []
    for r in rows:
        t = r.split(" ")
        pos0.append(int(t[1]) - 1)
        rb.append(t[2].encode())
        d = dict(zip(t[4::2], (int(v) for v in t[5::2])))
        c7.append([d[s] for s in "ACGTIDN"])
        assert int(t[3]) == sum(c7[-1])
    return np.array(pos0, dtype=np.int64), np.array(c7, dtype=np.int32).reshape(-1, 7), rb


def inflate(fn):
    return gzip.open(str(fn), "rb").read()
