"""Format ITEM of csrc/cv_truth_core.hpp and csrc/cv_beditems_core.hpp (the stabbing test, the two slab passes, the lane's
share of the line copy) in a stand-alone program built here with AddressSanitizer and UBSan
(tests/native/bed_items_driver.cpp: every line, text and array in a heap block of exactly its bytes; nothing is loaded into
this interpreter under a sanitizer).  Held to the host loop of clairvoyante_amd/bed_items.py: over the regular and the
mutated lines a ROW has the loop's (contig, position), a line the loop raises on is HOST and there is no SKIP; over slabs the
kept text and the counters are the loop's; the copy is exact at all 16 x 16 source and destination alignments."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bed_items_cases as bc
import truth_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
REC = 12 + 8


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("bed_items_core") / "bed_items_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "bed_items_driver.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def corpus():
    regular = [l for l in tc.truth_lines() if l.strip()] + bc.item_lines(n=80) + [b"%s 150 A C 0 1" % bc.LACKING.encode()]
    named = [b"", b" \t", b"c", b"c 007", b"c +5", b"c 5\r", b"c 5 \x80", b"c 5 " + b"x" * 8188, b"c 5 " + b"x" * 8189, b"a 1", b"a:b 1"]
    return regular, named, regular + named + [l for l in tc.mutated_lines(regular[:1400], tc.VAR) if b"\n" not in l]


def _run(driver, args, payload, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    if payload is not None:
        with open(src, "wb") as f:
            f.write(payload)
    p = subprocess.run([driver] + args + ([src, dst] if payload is not None else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    return p.stdout.decode(), (open(dst, "rb").read() if payload is not None else b"")


def test_the_copy_at_every_alignment(driver, tmp_path):
    said, _raw = _run(driver, ["copy"], None, tmp_path)
    m = re.match(r"ok (\d+) copies", said)
    assert m and int(m.group(1)) == 26 * 16 * 16, said


def test_format_item_under_sanitizers_is_the_host_loop(driver, corpus, tmp_path):
    regular, named, lines = corpus
    assert len(lines) >= 20000 and set(b"".join(lines)) | {10} == set(range(256))
    payload = struct.pack("<i", len(lines)) + b"".join(struct.pack("<i", len(l)) + l for l in lines)
    said, raw = _run(driver, ["lines"], payload, tmp_path)
    m = re.match(r"ok (\d+) lines, (\d+) rows, (\d+) skipped, (\d+) host", said)
    assert m and int(m.group(1)) == len(lines) and int(m.group(3)) == 0 and len(raw) == REC * len(lines)
    status = []
    for i, l in enumerate(lines):
        st, off, ln = struct.unpack_from("<iii", raw, REC * i)
        pos, = struct.unpack_from("<q", raw, REC * i + 12)
        wrong = bc.check_item_verdict(l, st, l[off:off + ln], pos)
        assert wrong is None, (l, wrong)
        status.append(st)
    kinds = [bc.define_item_line(l)[0] for l in lines]
    assert kinds.count("RAISE") > 1000 and status.count(bc.ROW) > 5000
    assert all(s == bc.ROW for s in status[:len(regular)])                    # no regular line goes to the host
    assert status[len(regular):len(regular) + len(named)] == [2, 2, 2, 2, 2, 2, 2, 0, 2, 0, 0]


def _slab_payload(text, tables, max_lines, want_text):
    names, off, begin, emax = tables
    return (struct.pack("<iiq", max_lines, want_text, len(text)) + text + struct.pack("<i", len(names)) +
            b"".join(struct.pack("<i", len(n)) + n for n in names) + off.astype("<i8").tobytes() + struct.pack("<q", len(begin)) +
            begin.astype("<i8").tobytes() + emax.astype("<i8").tobytes())


def _slab(driver, text, tables, max_lines, want_text, tmp_path):
    _said, raw = _run(driver, ["slab"], _slab_payload(text, tables, max_lines, want_text), tmp_path)
    info = np.frombuffer(raw, dtype="<i8", count=8)
    rows, runs = int(info[2]), int(info[5])
    at = 64
    pos = np.frombuffer(raw, dtype="<i8", count=rows, offset=at); at += 8 * rows
    run = np.frombuffer(raw, dtype="<i4", count=rows, offset=at); at += 4 * rows
    off = np.frombuffer(raw, dtype="<i8", count=rows, offset=at); at += 8 * rows
    ln = np.frombuffer(raw, dtype="<i8", count=rows, offset=at); at += 8 * rows
    tok = np.frombuffer(raw, dtype="<i8", count=2 * runs, offset=at).reshape(runs, 2); at += 16 * runs
    run_ctg = np.frombuffer(raw, dtype="<i4", count=runs, offset=at); at += 4 * runs
    counts = np.frombuffer(raw, dtype="<i8", count=4, offset=at); at += 32
    return info.tolist(), pos, run, off, ln, tok, run_ctg, counts.tolist(), raw[at:]


def test_the_slab_passes_under_sanitizers_are_the_host_loop(driver, corpus, tmp_path):
    regular, _named, lines = corpus
    bed = tc.write_lines(str(tmp_path / "conf.bed"), tc.bed_lines(), "plain")
    tables = bc.bed_tables(bed)
    fn = tc.write_lines(str(tmp_path / "items"), regular, "plain")
    want, tally, raised = bc.host_answer(fn, bed)
    assert raised is None and 0.1 * len(regular) < tally[1] < 0.9 * len(regular)
    text = open(fn, "rb").read()
    # the whole file as one slab, with and without the text; then slab by slab as the device route walks it
    info, pos, run, off, ln, tok, run_ctg, counts, kept = _slab(driver, text, tables, len(regular) + 5, 1, tmp_path)
    assert info[:6] == [len(text), len(regular), len(regular), 0, 0, info[5]] and counts == [tally[0], tally[1], len(want), 0] and kept == want
    assert [text[o:o + l] for o, l in zip(off, ln)] == [l + b"\n" for l in regular]
    assert [int(p) for p in pos] == [int(l.split()[1]) for l in regular]
    assert [text[tok[r, 0]:tok[r, 0] + tok[r, 1]] for r in run] == [l.split()[0] for l in regular] and (run_ctg == -1).sum() >= 1
    _i, _p, _r, _o, _l, _t, _c, counts, kept = _slab(driver, text, tables, len(regular) + 5, 0, tmp_path)
    assert counts == [tally[0], tally[1], 0, 0] and kept == b""
    out, lo, total = [], 0, 0
    while lo < len(text):
        hi = min(lo + 4099, len(text))
        info, _p, _r, _o, _l, _t, _c, counts, kept = _slab(driver, text[lo:hi], tables, 7, 1, tmp_path)    # a line table that fills up
        assert info[4] == 0 and info[1] <= 7
        if info[0] == 0:                                     # no line ends in the window: a wider one, as the walk grows its slab
            hi = min(lo + 3 * 4099, len(text))
            info, _p, _r, _o, _l, _t, _c, counts, kept = _slab(driver, text[lo:hi], tables, 7, 1, tmp_path)
        out.append(kept); total += info[1]; lo += info[0]
    assert b"".join(out) == want and total == tally[0]
    # mutated lines in one text: the HOST lines are exactly those that are no ROW, and nothing is kept of them
    mixed = b"\n".join(lines[:3000] + lines[-3000:]) + b"\nchr1 5 unfinished"
    info, pos, run, off, ln, tok, run_ctg, counts, kept = _slab(driver, mixed, tables, 1 << 20, 1, tmp_path)
    assert info[0] == len(mixed) - len(b"chr1 5 unfinished") and info[1] == 6000 and info[2] + info[4] == 6000 and info[4] > 300
    assert counts[0] == info[2] and 0 < counts[1] < info[2] and len(kept) == counts[2]
    for o, l, p, r in zip(off, ln, pos, run):
        piece = mixed[o:o + l - 1]
        assert mixed[o + l - 1:o + l] == b"\n" and bc.check_item_verdict(piece, bc.ROW, mixed[tok[r, 0]:tok[r, 0] + tok[r, 1]], int(p)) is None
    # degenerate texts
    for text, max_lines in ((b"", 5), (b"\n\n\n", 2), (b"a 1\n", 1), (b"a 1", 4)):
        info, _p, _r, _o, _l, _t, _c, counts, kept = _slab(driver, text, tables, max_lines, 1, tmp_path)
        assert info[:6] == {b"": [0, 0, 0, 0, 0, 0], b"\n\n\n": [2, 2, 0, 0, 2, 0], b"a 1\n": [4, 1, 1, 0, 0, 1], b"a 1": [0, 0, 0, 0, 0, 0]}[text]
        assert kept == b"" and counts[1] == 0
