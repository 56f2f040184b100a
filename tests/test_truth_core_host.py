"""One line of a truth list / BED file in the core's host form (csrc/cv_truth_core.hpp), held to the Python definition
applied to that single line (truth_cases.define_line: utils_v2._read_bed_truth's loop body and utils_v2._label).  The
core runs twice: in a stand-alone program built here with AddressSanitizer and UBSan (tests/native/truth_core_driver.cpp:
every line in a heap block of exactly its length; nothing is loaded into this interpreter under a sanitizer), and as the
library's cv_truth_lines_host_form over the lines joined into slabs.  The corpus is the regular cases plus about 20 000
mutated lines per format: bytes of all 256 values, truncations at every token boundary, the integer forms int() takes.
Condition: wherever the core says ROW or SKIP the definition agrees exactly; wherever the definition raises, or would read
the bytes as other lines, the core says HOST; and no regular line is HOST.  The kernels run the same text and are held to
the whole tables by test_gpu_truth_tables.py."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import truth_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
REC = 12 + 16 + 64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("truth_core") / "truth_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "truth_core_driver.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def corpus():
    """(format, source of format VCF or None) -> (regular lines, all lines)"""
    out = {}
    for fmt, regular in ((tc.VAR, tc.truth_lines()), (tc.BED, tc.bed_lines())):
        extra = [l for _n, f, l, _d in tc.IRREGULAR if f == fmt]
        out[fmt, None] = (regular, regular + extra + tc.mutated_lines(regular, fmt))
    regular = tc.vcf_lines()
    extra = [l for _n, f, l, _d in tc.IRREGULAR if f == tc.VCF]
    extra += [b"chr1\t300\t.\tA\t" + alt + b"\t50\tPASS\t.\tGT\t" + gt for alt in (b"C,G", b"CT,G,TTT", b"C,,G", b"C" * 99 + b",G" + b"T" * 99, b"C" * 99 + b"," + b"T" * 100, b"N,C")
              for gt in (b"1|2", b"2/1:7", b"1/2/3", b"12", b"1|", b"|", b"./.", b".", b"1|x", b"1|2|", b"0/1", b"1/1")]
    # (a VCF line is skipped by its first token whatever else it holds, so a "line" with a newline inside has no single
    # verdict: the line pass never makes one, and the corpus holds none)
    mutated = [l for l in tc.mutated_lines(regular, tc.VCF, n=21000) if b"\n" not in l]
    for filt in tc.VCF_FILTERS:
        out[tc.VCF, filt] = (regular, regular + extra + mutated)
    return out


def _head(fmt, filt):
    ctg, lo, hi = filt if filt is not None else (b"", None, None)
    return struct.pack("<iiqqi", fmt, int(lo is not None), lo or 0, hi or 0, len(ctg)) + ctg


def _run(driver, mode, payload, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(payload)
    p = subprocess.run([driver, mode, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    m = re.match(r"ok (\d+) lines, (\d+) rows, (\d+) skipped, (\d+) host", p.stdout.decode())
    assert m, p.stdout
    return [int(g) for g in m.groups()], open(dst, "rb").read()


def _verdicts(driver, fmt, lines, tmp_path, filt=None):
    payload = _head(fmt, filt) + struct.pack("<i", len(lines)) + b"".join(struct.pack("<i", len(l)) + l for l in lines)
    counts, raw = _run(driver, "lines", payload, tmp_path)
    assert counts[0] == len(lines) and len(raw) == REC * len(lines)
    out = []
    for i, l in enumerate(lines):
        status, off, ln = struct.unpack_from("<iii", raw, REC * i)
        pos, end = struct.unpack_from("<qq", raw, REC * i + 12)
        label = struct.unpack_from("<16f", raw, REC * i + 28)
        out.append((status, l[off:off + ln], pos, end, label))
    return out


def test_the_corpus_is_worth_the_name(corpus):
    for (fmt, filt), (regular, lines) in corpus.items():
        assert len(lines) >= 20000 and set(b"".join(lines)) | {10} == set(range(256))
        kinds = [tc.define_line(l, fmt, filt)[0] for l in lines]
        if fmt == tc.VCF:                                     # most mutated lines are another contig's: skipped, whatever they hold
            assert kinds.count("RAISE") > 100 and kinds.count("LINES") == 0 and kinds.count("ROW") > 500 and kinds.count("SKIP") > 5000
        else:
            assert kinds.count("RAISE") > 1000 and kinds.count("LINES") > 300 and kinds.count("ROW") > 5000 and kinds.count("SKIP") > 10
        assert all(tc.define_line(l, fmt, filt)[0] in ("ROW", "SKIP") for l in regular)
    labels = {tuple(tc.define_line(l, tc.VAR)[3]) for l in corpus[tc.VAR, None][0] if l.strip()}
    assert len(labels) > 40                                   # het / hom / neither x SNP / INS / DEL x the length classes
    raw = b"\n".join(corpus[tc.VCF, tc.VCF_FILTERS[0]][0])    # the regular VCF: what the issue lists
    assert any(b >= 0x80 for b in raw) and b"./." in raw and b"1|0" in raw and b"0/1:9\t" in raw
    multi = [l.split(b"\t") for l in raw.split(b"\n") if b"," in l and (b"\t1/2:" in l or b"\t2|1:" in l)]
    assert {len(l[4].split(b",")) for l in multi} == {2, 3}
    assert any(len(set(map(len, l[4].split(b",")))) == 1 for l in multi) and any(len(set(map(len, l[4].split(b",")))) > 1 for l in multi)


def test_the_core_under_sanitizers_is_the_definition(driver, corpus, tmp_path):
    for (fmt, filt), (regular, lines) in corpus.items():
        got = _verdicts(driver, fmt, lines, tmp_path, filt)
        for l, (status, ctg, pos, end, label) in zip(lines, got):
            wrong = tc.check_verdict(l, fmt, status, ctg, pos, end, label, filt)
            assert wrong is None, (fmt, filt, l, wrong)
        # the regular cases are the device's: no line of them goes to the host, and a good part of the rest stays too
        assert all(s[0] != tc.HOST for s in got[:len(regular)]), [l for l, s in zip(regular, got) if s[0] == tc.HOST][:5]
        assert sum(1 for s in got[len(regular):] if s[0] == tc.ROW) > (100 if fmt == tc.VCF else 2000)
        if fmt == tc.VCF:
            assert sum(1 for s in got[:len(regular)] if s[0] == tc.ROW) > 50
    wanted = {name: stays for name, _f, _l, stays in tc.IRREGULAR}
    for name, fmt, line, stays in tc.IRREGULAR:
        filt = tc.VCF_FILTERS[0] if fmt == tc.VCF else None
        (status, _c, _p, _e, _l), = _verdicts(driver, fmt, [line], tmp_path, filt)
        assert (status != tc.HOST) == wanted[name], name


def _slabs(lines, fmt):
    """the corpus as texts: the lines without a newline of their own, joined; one text also ends without a newline"""
    lines = [l for l in lines if b"\n" not in l]
    third = len(lines) // 3
    yield b"\n".join(lines[:third]) + b"\n", 1 << 20
    yield b"\n".join(lines[third:2 * third]) + b"\nchr1 5 A", 1 << 20         # the last piece is no line yet
    yield b"\n".join(lines[2 * third:]) + b"\n", 1000                          # a line table that fills up
    yield b"", 5
    yield b"\n\n\n", 2


def _expected(text, fmt, max_lines):
    """cv_truth_lines_*'s outputs from the per-line definition (HOST where the definition has no single-line answer:
    there the outputs are compared only in their counts)"""
    pieces = text.split(b"\n")[:-1][:max_lines]
    return pieces, sum(len(p) + 1 for p in pieces)


def _check_slab(text, fmt, filt, max_lines, info, pos, aux, run, tok):
    pieces, used = _expected(text, fmt, max_lines)
    assert info[0] == used and info[1] == len(pieces) and info[6] == 0 and info[7] == 0
    rows = runs = skipped = host = 0
    at, prev = 0, None
    for p in pieces:
        want = tc.define_line(p, fmt, filt)
        # the status of this line, from the rows the pass wrote: a ROW is there, in order, with the definition's fields
        status = _status[(fmt, filt, p)]
        if status == tc.ROW:
            assert rows < info[2] and want[0] == "ROW", p
            o, ln = int(tok[run[rows]][0]), int(tok[run[rows]][1])
            ctg = p.split()[0]
            assert text[o:o + ln] == ctg and pos[rows] == want[2], (p, rows)
            assert (aux[rows] == want[3]) if fmt == tc.BED else ([float(v) for v in aux[rows]] == [float(v) for v in want[3]]), p
            new_run = prev != ctg
            runs += new_run
            assert run[rows] == runs - 1 and (not new_run or o == at + p.index(ctg)), p
            prev = ctg
            rows += 1
        else:
            prev = None
            skipped += status == tc.SKIP
            host += status == tc.HOST
        at += len(p) + 1
    assert [rows, skipped, host, runs] == [int(info[2]), int(info[3]), int(info[4]), int(info[5])]


_status = {}                                                  # (format, line) -> the core's verdict, from the stand-alone program


def test_the_slab_forms_are_the_definition(driver, corpus, tmp_path):
    """cvt::host_form under the sanitizers and the library's cv_truth_lines_host_form, over the same texts"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for (fmt, filt), (_regular, lines) in corpus.items():
        for l, v in zip(lines, _verdicts(driver, fmt, lines, tmp_path, filt)):
            _status[(fmt, filt, l)] = v[0]
        _status[(fmt, filt, b"")] = tc.SKIP
        ctg, lo, hi = filt if filt is not None else (None, None, None)
        for text, max_lines in _slabs(lines, fmt):
            # the stand-alone program
            _c, raw = _run(driver, "slab", _head(fmt, filt) + struct.pack("<iq", max_lines, len(text)) + text, tmp_path)
            info = np.frombuffer(raw, dtype="<i8", count=8)
            rows, runs = int(info[2]), int(info[5])
            at = 64
            pos = np.frombuffer(raw, dtype="<i8", count=rows, offset=at); at += 8 * rows
            if fmt == tc.BED:
                aux = np.frombuffer(raw, dtype="<i8", count=rows, offset=at); at += 8 * rows
            else:
                aux = np.frombuffer(raw, dtype="<f4", count=16 * rows, offset=at).reshape(rows, 16); at += 64 * rows
            run = np.frombuffer(raw, dtype="<i4", count=rows, offset=at); at += 4 * rows
            tok = np.frombuffer(raw, dtype="<i8", count=2 * runs, offset=at).reshape(runs, 2)
            assert at + 16 * runs == len(raw)
            _check_slab(text, fmt, filt, max_lines, info, pos, aux, run, tok)
            # the library: the same bytes, and nothing behind the rows
            n = max_lines
            lpos = np.full(n + 1, -7, np.int64); lend = np.full(n + 1, -7, np.int64); llab = np.full((n + 1, 16), -7, np.float32)
            lrun = np.full(n + 1, -7, np.int32); ltok = np.full((n + 1, 2), -7, np.int64); linfo = np.full(8, -7, np.int64)
            buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
            _lib.check(lib.cv_truth_lines_host_form(p(buf), len(text), fmt, ctg, len(ctg or b""), int(lo is not None), lo or 0, hi or 0, n, p(lpos), p(lend) if fmt == tc.BED else None,
                                                    None if fmt == tc.BED else p(llab), p(lrun), p(ltok), p(linfo)))
            assert linfo.tolist() == info.tolist()
            assert np.array_equal(lpos[:rows], pos) and np.array_equal(lrun[:rows], run) and np.array_equal(ltok[:runs], tok)
            assert np.array_equal(lend[:rows], aux) if fmt == tc.BED else np.array_equal(llab[:rows], aux)
            assert (lpos[rows:] == -7).all() and (lrun[rows:] == -7).all() and (ltok[runs:] == -7).all()
            assert (lend[rows if fmt == tc.BED else 0:] == -7).all() and (llab[0 if fmt == tc.BED else rows:] == -7).all()


def test_refusals():
    from clairvoyante_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    assert lib.cv_truth_lines_workspace(-1, 5, ctypes.byref(need)) == 1 and lib.cv_truth_lines_workspace(5, 5, None) == 1
    assert lib.cv_truth_lines_workspace(5, (1 << 27) + 1, ctypes.byref(need)) == 1
    assert lib.cv_bed_table_workspace(-1, ctypes.byref(need)) == 1 and lib.cv_truth_tables_workspace((1 << 30) + 1, ctypes.byref(need)) == 1
    text = np.frombuffer(b"chr1 5 A C 0 1\n", dtype=np.uint8)
    pos = np.zeros(4, np.int64); lab = np.zeros((4, 16), np.float32); run = np.zeros(4, np.int32); tok = np.zeros((4, 2), np.int64)
    info = np.zeros(8, np.int64)
    p = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    call = lambda **kw: lib.cv_truth_lines_host_form(*[kw.get(k, v) for k, v in (
        ("text", p(text)), ("len", len(text)), ("format", tc.VAR), ("ctg", None), ("ctg_len", 0), ("has_bounds", 0), ("lo", 0), ("hi", 0),
        ("max_lines", 4), ("pos", p(pos)), ("end", None), ("label", p(lab)),
        ("run", p(run)), ("tok", p(tok)), ("info", p(info)))])
    assert call() == 0 and info.tolist() == [15, 1, 1, 0, 0, 1, 0, 0] and pos[0] == 5 and lab[0].tolist()[:6] == [0.5, 0.5, 0, 0, 1, 0]
    for bad in (dict(text=None), dict(pos=None), dict(label=None), dict(run=None), dict(tok=None), dict(info=None), dict(format=3), dict(format=tc.VCF), dict(format=tc.VCF, ctg=b"c", ctg_len=257),
                dict(len=-1), dict(max_lines=-1), dict(pos=p(pos, 4)), dict(tok=p(tok, 4)), dict(info=p(info, 4)), dict(run=p(run, 2)),
                dict(format=tc.BED)):
        assert call(**bad) == 1, bad
        assert b"cv_truth_lines_host_form" in lib.cv_last_error()
