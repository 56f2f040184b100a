"""Inputs of the tests of cv_items_copy_dev / cv_items_copy_host_form (tests/test_pair_route_host.py, tests/test_gpu_pair.py):
texts cut into lines, the lengths a caller keeps, and a Python restatement of the gather."""
import numpy as np

FILL = 0xA5


def restated(text, off, kept_len, out_cap):
    """the gather over bytes `text`: lines of kept_len[i] > 0 bytes at off[i], one behind the other in a room of out_cap bytes
    that starts as FILL; a line that does not lie inside the text or would not fit is not written but takes its room
    -> (the room's bytes, [0, 0, sum of the lengths, 0])"""
    room = bytearray([FILL]) * out_cap
    at = 0
    for o, m in zip(off.tolist(), kept_len.tolist()):
        if m > 0 and 0 <= o and o + m <= len(text) and 0 <= at and at + m <= out_cap:
            room[at:at + m] = text[o:o + m]
        at += m
    return bytes(room), [0, 0, at, 0]


def lines_text(lengths, seed=1, gap=0):
    """lines of the given lengths (each ends with a newline; every byte else is printable) with `gap` bytes between them
    -> (text, off)"""
    rng = np.random.RandomState(seed)
    n, lengths = len(lengths), np.asarray(lengths, dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lengths + gap)[:-1])).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    total = int((lengths + gap).sum())
    text = rng.randint(0x21, 0x7F, total).astype(np.uint8)
    if n:
        text[off + lengths - 1] = 10
    return text.tobytes(), off


def cases():
    """name -> (text, off, kept_len, out_cap): none, all, alternating, lengths 1 .. 300 at mixed source alignments (a gap of
    0 .. 2 lines shifts them), a room one byte short"""
    out = {"n = 0": (b"abc\n", np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 4)}
    rng = np.random.RandomState(7)
    lengths = np.arange(1, 301, dtype=np.int64)
    rng.shuffle(lengths)
    text, off = lines_text(lengths, seed=2, gap=3)
    total = int(lengths.sum())
    alt = lengths * (np.arange(300) % 2)
    mixed = lengths * (rng.randint(0, 3, 300) > 0)
    out["none kept"] = (text, off, np.zeros(300, dtype=np.int64), 64)
    out["all kept"] = (text, off, lengths.copy(), total)
    out["alternating"] = (text, off, alt, int(alt.sum()))
    out["lengths 1 to 300, mixed alignments"] = (text, off, mixed, int(mixed.sum()) + 17)
    out["one byte short"] = (text, off, lengths.copy(), total - 1)
    return out
