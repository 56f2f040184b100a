"""The dataPrepScripts helpers without a GPU: the host loops of clairvoyante_amd/bed_items.py against hand-written
expectations (they are the definitions the device route is held to by test_gpu_bed_items.py), sample_positions_host against
a literal loop over the positions, the library's two host forms (cv_item_lines_host_form, cv_items_keep_host_form) against
the host loop, CombineMultipleDatasetsForTraining's outputs, and the four command lines."""
import ctypes
import gzip
import io
import logging
import os
import sys

import numpy as np
import pytest

import bed_items_cases as bc
import truth_cases as tc

NAMES = ("ChooseItemInBed", "CountNumInBed", "RandomSampling", "CombineMultipleDatasetsForTraining")
BED = b"c 10 20\nd 10 11\n\ne\t100\t200\te1\ne 150 300\ne 120 130\nonlybed 1 5\n"
# contig, position, kept: begin - 1, begin, end - 2, end - 1, end of every interval
ITEMS = (("c", 9, 0), ("c", 10, 1), ("c", 18, 1), ("c", 19, 0), ("c", 20, 0),
         ("d", 9, 0), ("d", 10, 1), ("d", 11, 0),
         ("e", 99, 0), ("e", 100, 1), ("e", 128, 1), ("e", 129, 1), ("e", 130, 1), ("e", 198, 1), ("e", 199, 1), ("e", 200, 1),
         ("e", 298, 1), ("e", 299, 0), ("e", 300, 0), ("onlyitems", 10, 0), ("c", 12, 1))


@pytest.fixture(autouse=True)
def host_route(monkeypatch):
    monkeypatch.setenv("CV_BED_ITEMS", "host")


def _write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def _item_text(items=ITEMS, last_newline=False):
    rows = [("%s %d tail %d" % (c, p, i)).encode() for i, (c, p, _k) in enumerate(items)]
    return b"\n".join(rows) + (b"\n" if last_newline else b""), rows


def test_choose_and_count_against_hand_written_expectations(tmp_path):
    from clairvoyante_amd import bed_items
    bed = _write(tmp_path / "r.bed", BED)
    text, rows = _item_text()
    want = b"".join(r + b"\n" for r, (_c, _p, k) in zip(rows, ITEMS) if k)[:-1]      # the last line has no newline and is kept
    for fn in (_write(tmp_path / "items", text), _write(tmp_path / "items.gz", gzip.compress(text))):
        out = io.BytesIO()
        assert bed_items.choose_items_host(fn, bed, out) == (len(ITEMS), sum(k for _c, _p, k in ITEMS))
        assert out.getvalue() == want and not want.endswith(b"\n")
        assert bed_items.count_items_host(fn, bed) == (len(ITEMS), sum(k for _c, _p, k in ITEMS))
        out = io.BytesIO()
        assert bed_items.choose_items(fn, bed, out) == (len(ITEMS), 12) and out.getvalue() == want
    assert "Blank BED lines follow the project's reader" in bed_items.bed_tree.__doc__


@pytest.mark.parametrize("bad, exc", [(b"c", IndexError), (b"c x", ValueError), (b"", IndexError), (b"c 1.5 z", ValueError)])
def test_an_irregular_line_raises_after_the_lines_before_it(tmp_path, bad, exc):
    from clairvoyante_amd import bed_items
    bed = _write(tmp_path / "r.bed", BED)
    fn = _write(tmp_path / "items", b"c 10 first\nc 9 no\nd 10 second\n" + bad + b"\nc 11 never\n")
    out = io.BytesIO()
    with pytest.raises(exc):
        bed_items.choose_items_host(fn, bed, out)
    assert out.getvalue() == b"c 10 first\nd 10 second\n"
    with pytest.raises(exc):
        bed_items.count_items_host(fn, bed)
    # what int() takes is no error: "+5", "007", "1_0" are positions 5, 7, 10
    fn = _write(tmp_path / "items2", b"c +10 a\nc 0011 b\nc 1_2 c\n\tc\t13\n")
    out = io.BytesIO()
    assert bed_items.choose_items_host(fn, bed, out) == (4, 4) and out.getvalue() == b"c +10 a\nc 0011 b\nc 1_2 c\n\tc\t13\n"


def test_count_num_in_bed_logs_and_divides_by_zero(tmp_path, caplog):
    from clairvoyante_amd import CountNumInBed
    bed = _write(tmp_path / "r.bed", BED)
    fn = _write(tmp_path / "items", _item_text(last_newline=True)[0])
    args = CountNumInBed.build_parser().parse_args(["--input_fn", fn, "--bed_fn", bed])
    with caplog.at_level(logging.INFO):
        CountNumInBed.Run(args)
    assert "Total: 21, Overlapped: 12, Percentage: 57.143" in caplog.text
    args = CountNumInBed.build_parser().parse_args(["--input_fn", _write(tmp_path / "empty", b""), "--bed_fn", bed])
    with pytest.raises(ZeroDivisionError):
        CountNumInBed.Run(args)


def test_route_switch(monkeypatch):
    from clairvoyante_amd import bed_items, utils_v2
    assert bed_items.route() == "host" and bed_items.route("nothing") == "host"
    monkeypatch.delenv("CV_BED_ITEMS")
    assert bed_items.DEVICE_MIN_BYTES is None and bed_items.route(__file__) == "host"     # no floor is set: opt-in
    monkeypatch.setenv("CV_BED_ITEMS", "gpu")
    with pytest.raises(ValueError):
        bed_items.route()
    monkeypatch.setenv("CV_BED_ITEMS", "device")
    assert bed_items.route() == ("device" if utils_v2._gpu_present() else "host")
    c = bed_items.counts(reset=True)
    assert sorted(c) == sorted(("device_lines", "host_lines", "device_calls", "host_calls", "handed_over_calls", "device_positions"))
    assert set(bed_items.counts().values()) == {0}


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def _literal_sample(ctg, start, end, prob, intervals, seed):
    from clairvoyante_amd import draws, utils_v2
    iv = None
    if intervals is not None:
        iv = utils_v2._Intervals()
        for b, e in intervals:
            iv.addi(b, e)
    out = []
    for i in range(start, end):
        if iv is not None and not iv.hit(i):
            continue
        if draws.draws(seed, draws.RANDOM, ctg, [i])[0] <= prob:
            out.append(i)
    return np.array(out, dtype=np.int64)


def test_sample_positions_host_is_the_literal_loop(monkeypatch):
    from clairvoyante_amd import bed_items, draws
    assert draws.RANDOM == 2
    intervals = bc.sample_intervals(end=3000, n=12, seed=4)
    covered = np.array([i for i in range(1, 3000) if any(b <= i < e for b, e in intervals)], dtype=np.int64)
    assert 100 < len(covered) < 2900
    for tile in (1 << 24, 1000):
        monkeypatch.setattr(bed_items, "SAMPLE_TILE", tile)
        for prob in (0.0, 0.3, 1.0):
            for iv in (intervals, None):
                got = bed_items.sample_positions_host("chr7", 1, 3000, prob, iv, 99)
                assert got.dtype == np.int64 and np.array_equal(got, _literal_sample("chr7", 1, 3000, prob, iv, 99)), (tile, prob)
                if prob == 0.3:
                    n = len(covered) if iv is not None else 2999
                    assert 0.2 * n < len(got) < 0.4 * n
        assert np.array_equal(bed_items.sample_positions_host("chr7", 1, 3000, 1.0, intervals, 99), covered)
        assert len(bed_items.sample_positions_host("chr7", 1, 3000, 0.0, intervals, 99)) == 0
        assert len(bed_items.sample_positions_host("chr7", 500, 500, 1.0, None, 99)) == 0
        assert len(bed_items.sample_positions_host("chr7", 500, -1, 1.0, None, 99)) == 0
    # another contig, another seed: other draws
    a = bed_items.sample_positions_host("chr7", 1, 3000, 0.3, None, 99)
    assert not np.array_equal(a, bed_items.sample_positions_host("chr8", 1, 3000, 0.3, None, 99))
    assert not np.array_equal(a, bed_items.sample_positions_host("chr7", 1, 3000, 0.3, None, 98))


def _sampling_files(tmp_path):
    ref = str(tmp_path / "ref.fa")
    _write(ref + ".fai", b"chr1\t500\t6\t60\t61\nchr7\t3000\t600\t60\t61\n")
    bed = _write(tmp_path / "s.bed", b"".join(b"chr7\t%d\t%d\n" % (b, e + 1) for b, e in bc.sample_intervals(end=3000, n=12, seed=4)) + b"chr1 5 50\n")
    return ref, bed


def _main(mod, argv, monkeypatch, capfdbinary):
    monkeypatch.setattr(sys, "argv", [mod.__name__.split(".")[-1] + ".py"] + argv)
    capfdbinary.readouterr()
    mod.main()
    return capfdbinary.readouterr()


def test_random_sampling_command_line(tmp_path, monkeypatch, capfdbinary):
    from clairvoyante_amd import RandomSampling, bed_items
    ref, bed = _sampling_files(tmp_path)
    # candidates * 2 / genomeSize = 0.3; [ctgStart, ctgEnd) inside the contig
    argv = ["--ref_fn", ref, "--ctgName", "chr7", "--candidates", "150", "--genomeSize", "1000", "--bed_fn", bed, "--seed", "7"]
    one = _main(RandomSampling, argv, monkeypatch, capfdbinary).out
    want = bed_items.sample_positions_host("chr7", 1, 3000, 150 * 2. / 1000, bc.sample_intervals(end=3000, n=12, seed=4), 7)
    assert len(want) > 50 and one == b"".join(b"chr7\t%d\n" % p for p in want)
    assert _main(RandomSampling, argv, monkeypatch, capfdbinary).out == one                 # --seed 7 twice
    assert _main(RandomSampling, argv[:-1] + ["8"], monkeypatch, capfdbinary).out != one
    can = str(tmp_path / "can.gz")
    assert _main(RandomSampling, argv + ["--can_fn", can], monkeypatch, capfdbinary).out == b""
    assert open(can, "rb").read(2) == b"\x1f\x8b" and gzip.open(can).read() == one
    cut = _main(RandomSampling, argv + ["--ctgStart", "1000", "--ctgEnd", "2000"], monkeypatch, capfdbinary).out
    assert cut == b"".join(b"chr7\t%d\n" % p for p in want if 1000 <= p < 2000) and cut
    # bounds outside the contig change nothing (:36-39)
    assert _main(RandomSampling, argv + ["--ctgStart", "0", "--ctgEnd", "9000"], monkeypatch, capfdbinary).out == one
    # a contig the .fai lacks: the reference's message, nothing sampled
    got = _main(RandomSampling, ["--ref_fn", ref, "--ctgName", "chrQ", "--seed", "7", "--candidates", "1", "--genomeSize", "1"], monkeypatch, capfdbinary)
    assert got.out == b"" and b"Chromosome chrQ not found in %s.fai" % ref.encode() in got.err
    # a contig the BED lacks: read_bed's exit
    with pytest.raises(SystemExit) as e:
        _main(RandomSampling, ["--ref_fn", ref, "--ctgName", "chrQ", "--bed_fn", bed], monkeypatch, capfdbinary)
    assert e.value.code == 1 and b"ctgName is not in the bed file" in capfdbinary.readouterr().err
    with pytest.raises(SystemExit) as e:
        _main(RandomSampling, ["--ref_fn", str(tmp_path / "none.fa"), "--ctgName", "chr7"], monkeypatch, capfdbinary)
    assert e.value.code == 1


# ---- the library's host forms against the host loop ---------------------------------------------------------------------------
def _forms(lib, text, tables, want_text=1):
    """cv_item_lines_host_form + cv_items_keep_host_form over one piece of text -> (info, rows' (off, ctg, pos), kept text, counts)"""
    from clairvoyante_amd import _lib
    names, bed_off, begin, emax = tables
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = max(len(text), 1)
    buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)
    pos = np.full(n, -7, np.int64); run = np.full(n, -7, np.int32); off = np.full(n, -7, np.int64); ln = np.full(n, -7, np.int64)
    tok = np.full((n, 2), -7, np.int64); info = np.full(8, -7, np.int64)
    _lib.check(lib.cv_item_lines_host_form(p(buf), len(text), n, p(pos), p(run), p(off), p(ln), p(tok), p(info)))
    used, lines, rows, skipped, host, runs = info.tolist()[:6]
    assert skipped == 0 and lines == rows + host and info[6] == 0 and info[7] == 0
    assert (pos[rows:] == -7).all() and (run[rows:] == -7).all() and (off[rows:] == -7).all() and (tok[runs:] == -7).all()
    ctgs = [bytes(text[tok[k, 0]:tok[k, 0] + tok[k, 1]]) for k in range(runs)]
    run_ctg = np.array([names.index(c) if c in names else -1 for c in ctgs] or [0], dtype=np.int32)
    counts = np.full(4, -7, np.int64)
    cap = int(ln[:rows].sum())
    out = np.full(cap + 32, 0xA5, np.uint8)
    _lib.check(lib.cv_items_keep_host_form(p(buf), len(text), rows, p(pos), p(run), p(off), p(ln), p(run_ctg), runs, len(names), p(bed_off),
                                           p(begin) if len(begin) else None, p(emax) if len(emax) else None, want_text, ctypes.c_void_p(out.ctypes.data + 16),
                                           cap, p(counts)))
    assert counts[0] == rows and counts[3] == 0 and (out[:16] == 0xA5).all() and (out[16 + int(counts[2]):] == 0xA5).all()
    found = [(int(off[r]), ctgs[run[r]], int(pos[r]), int(ln[r])) for r in range(rows)]
    return info.tolist(), found, out[16:16 + int(counts[2])].tobytes(), counts.tolist()


def _walk_forms(lib, text, tables, slab):
    """the device route's walk with the host forms in the kernels' place -> (bytes kept, lines, kept, offset of the first
    HOST line's slab or None)"""
    out, total, kept, lo, hi = [], 0, 0, 0, min(slab, len(text))
    while lo < len(text):
        info, _found, got, counts = _forms(lib, text[lo:hi], tables)
        if info[4]:
            return b"".join(out), total, kept, lo
        out.append(got); total += info[1]; kept += counts[1]; lo += info[0]
        if hi >= len(text):
            break
        hi = min(hi + slab, len(text))
    assert lo == len(text)
    return b"".join(out), total, kept, None


def test_the_host_forms_are_the_host_loop(tmp_path):
    from clairvoyante_amd import _lib
    lib = _lib.load()
    bed = tc.write_lines(str(tmp_path / "conf.bed"), tc.bed_lines(), "plain")
    tables = bc.bed_tables(bed)
    assert len(tables[0]) == 5 and len(tables[2]) > 400
    regular = [l for l in tc.truth_lines() if l.strip()] + bc.item_lines(n=60)
    fn = tc.write_lines(str(tmp_path / "items"), regular, "plain")
    want, tally, raised = bc.host_answer(fn, bed)
    assert raised is None and 0.1 * len(regular) < tally[1] < 0.9 * len(regular)
    text = open(fn, "rb").read()
    for slab in (257, 1 << 20):
        assert _walk_forms(lib, text, tables, slab) == (want, tally[0], tally[1], None)
    # the truth list as it is holds blank lines: the host loop raises there, the forms say HOST for that slab, and what
    # they kept before it is the beginning of what the loop wrote
    fn = tc.write_lines(str(tmp_path / "blanks"), tc.truth_lines(), "plain")
    want, _t, raised = bc.host_answer(fn, bed)
    assert isinstance(raised, IndexError)
    got, _lines, _kept, at = _walk_forms(lib, open(fn, "rb").read(), tables, 257)
    assert at is not None and want.startswith(got)
    # without text only the counters
    info, _f, got, counts = _forms(lib, text, tables, want_text=0)
    assert got == b"" and counts == [tally[0], tally[1], 0, 0]


def test_the_host_forms_over_mutated_lines(tmp_path):
    """every line the core calls ROW has the host loop's (ctg, pos), every line the loop raises on is HOST"""
    from clairvoyante_amd import _lib
    lib = _lib.load()
    bed = tc.write_lines(str(tmp_path / "conf.bed"), tc.bed_lines(), "plain")
    tables = bc.bed_tables(bed)
    regular = [l for l in tc.truth_lines() if l.strip()]
    lines = tc.mutated_lines(regular, tc.VAR) + [b"", b" ", b"c", b"c 007", b"c +5", b"c 5\r", b"c 5 \x80", b"c 5 " + b"x" * 8188, b"c 5 " + b"x" * 8189]
    assert len(lines) >= 20000
    text = b"\n".join(lines) + b"\n"
    pieces = text.split(b"\n")[:-1]                         # (a mutated line may hold a newline: these are the lines the file has)
    info, found, kept_text, counts = _forms(lib, text, tables)
    assert info[0] == len(text) and info[1] == len(pieces)
    rows = {o: (c, p, l) for o, c, p, l in found}
    at = n_rows = n_raise = 0
    kept = []
    for piece in pieces:
        want = bc.define_item_line(piece)
        if at in rows:
            c, p, l = rows[at]
            assert bc.check_item_verdict(piece, bc.ROW, c, p) is None and l == len(piece) + 1, piece
            n_rows += 1
            iv = tables[0].index(c) if c in tables[0] else -1
            if iv >= 0:
                b, e = tables[2][tables[1][iv]:tables[1][iv + 1]], tables[3][tables[1][iv]:tables[1][iv + 1]]
                k = int(np.searchsorted(b, p, side="right"))
                if k > 0 and e[k - 1] > p:
                    kept.append(piece + b"\n")
        else:
            n_raise += want[0] == "RAISE"
        assert want[0] != "RAISE" or at not in rows, piece
        at += len(piece) + 1
    assert n_rows > 5000 and n_raise > 1000 and n_rows == info[2]
    assert kept_text == b"".join(kept) and counts[1] == len(kept) > 500
    # the named irregular lines, and the line of exactly CV_TRUTH_LINE_CAP bytes
    verdict = lambda l: _forms(lib, l + b"\n", tables)[0][2]
    assert [verdict(l) for l in lines[-9:]] == [0, 0, 0, 0, 0, 0, 0, 1, 0]
    assert verdict(b"a 1") == 1 and verdict(b"a:b 1") == 1 and verdict(b"a 999999999999") == 1 and verdict(b"a 1000000000000") == 0


def test_host_form_refusals():
    from clairvoyante_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    assert lib.cv_item_lines_workspace(-1, 5, ctypes.byref(need)) == 1 and lib.cv_item_lines_workspace(5, 5, None) == 1
    assert lib.cv_items_keep_workspace(-1, ctypes.byref(need)) == 1 and lib.cv_sample_positions_workspace((1 << 28) + 1, ctypes.byref(need)) == 1
    assert lib.cv_sample_positions_dev(1, 2, -1, 5, 0.5, 0, None, None, None, 0, None, None, 0, None) == 1
    assert b"cv_sample_positions_dev" in lib.cv_last_error()
    info = np.zeros(8, np.int64)
    assert lib.cv_item_lines_host_form(None, 4, 4, None, None, None, None, None, info.ctypes.data_as(ctypes.c_void_p)) == 1
    assert b"cv_item_lines_host_form" in lib.cv_last_error()
    assert lib.cv_items_keep_host_form(None, 0, 0, None, None, None, None, None, 0, 0, None, None, None, 0, None, 0, None) == 1
    assert b"cv_items_keep_host_form" in lib.cv_last_error()


# ---- CombineMultipleDatasetsForTraining -----------------------------------------------------------------------------------------
def test_combine_multiple_datasets(tmp_path, monkeypatch, capfdbinary):
    from clairvoyante_amd import CombineMultipleDatasetsForTraining as combine, utils_v2
    rng = np.random.RandomState(1)
    sets, listing = [], []
    for k in range(3):
        files = []
        for j in range(4):
            rows = [b"chr%d %d %s\n" % (k, int(rng.randint(0, 999)), b"x" * int(rng.randint(0, 90))) for _ in range(int(rng.randint(1, 40)))]
            if k == 1 and j == 2:
                rows[-1] = rows[-1][:-1]                     # a last line without its newline
            if k == 2 and j == 3:
                rows = []                                    # an empty file
            fn = str(tmp_path / ("d%d_%d" % (k, j)))
            _write(fn, gzip.compress(b"".join(rows)) if (k + j) % 2 else b"".join(rows))
            files.append((fn, rows))
        sets.append(files)
        listing.append(" ".join(fn for fn, _r in files))
    lst = _write(tmp_path / "list", ("\n".join(listing) + "\n").encode())
    # prefix + row per row, nothing inserted: behind the line without a newline the next dataset's prefix follows at once
    want = [b"".join(bytes([ord("a") + k]) + r for k in range(3) for r in sets[k][j][1]) for j in range(4)]
    monkeypatch.setattr(combine, "BLOCK", 97)               # many blocks per file: line starts at and across the seams
    for extra in ([], ["--bgzf"]):
        outs = [str(tmp_path / ("out%d%s" % (j, "b" if extra else ""))) for j in range(4)]
        _main(combine, ["--input_list", lst, "--tensor_can_out", outs[0], "--tensor_var_out", outs[1], "--var_out", outs[2],
                        "--bed_out", outs[3]] + extra, monkeypatch, capfdbinary)
        for j in range(4):
            assert gzip.open(outs[j]).read() == want[j], (extra, j)
            assert utils_v2.is_bgzf(outs[j]) == bool(extra)
    seam = sets[1][2][1][-1]
    assert not seam.endswith(b"\n") and (b"b" + seam + b"c" + sets[2][2][1][0]) in want[2]


def test_prefix_lines():
    from clairvoyante_amd import bed_items
    assert bed_items.prefix_lines(b"", 97, True) == (b"", True)
    assert bed_items.prefix_lines(b"x\ny\n", 97, True) == (b"ax\nay\n", True)
    assert bed_items.prefix_lines(b"x\ny", 98, False) == (b"x\nby", False)
    assert bed_items.prefix_lines(b"\n\n", 99, True) == (b"c\nc\n", True)


# ---- the command lines --------------------------------------------------------------------------------------------------------
def test_the_invocator_lists_and_dispatches(tmp_path, monkeypatch, capfdbinary):
    import clairvoyante_amd.__main__ as m
    import importlib
    for n in NAMES:
        assert n in m.SUBMODULES and n not in m.NOT_BUILT
    assert "demoRun" in m.NOT_BUILT
    monkeypatch.setattr(sys, "argv", ["clairvoyante_amd"])
    with pytest.raises(SystemExit) as e:
        m.main()
    listed = capfdbinary.readouterr().out.decode()
    assert e.value.code == 0 and all("  - %s\n" % n in listed for n in NAMES)
    # no arguments: help and exit status 1, through the invocator and on their own
    for n in NAMES:
        mod = importlib.import_module("clairvoyante_amd." + n)
        for argv in (["clairvoyante_amd", n], [n + ".py"]):
            monkeypatch.setattr(sys, "argv", argv)
            with pytest.raises(SystemExit) as e:
                (m if len(argv) == 2 else mod).main()
            assert e.value.code == 1 and b"usage:" in capfdbinary.readouterr().out
        flags = {a.option_strings[0]: a.default for a in mod.build_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
        assert flags == {"ChooseItemInBed": {"--input_fn": None, "--bed_fn": None}, "CountNumInBed": {"--input_fn": None, "--bed_fn": None},
                         "RandomSampling": {"--ref_fn": "ref.fa", "--ctgName": None, "--can_fn": "PIPE", "--candidates": 7000000,
                                            "--genomeSize": 3000000000, "--bed_fn": None, "--ctgStart": None, "--ctgEnd": None, "--seed": None},
                         "CombineMultipleDatasetsForTraining": {"--input_list": None, "--tensor_can_out": None, "--tensor_var_out": None,
                                                                "--var_out": None, "--bed_out": None, "--bgzf": False}}[n]
    bed = _write(tmp_path / "r.bed", BED)
    fn = _write(tmp_path / "items", b"c 10 kept\nc 9 dropped\nq 10 dropped\n")
    monkeypatch.setattr(sys, "argv", ["clairvoyante_amd", "ChooseItemInBed", "--input_fn", fn, "--bed_fn", bed])
    m.main()
    assert capfdbinary.readouterr().out == b"c 10 kept\n"
