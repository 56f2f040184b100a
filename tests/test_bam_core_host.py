"""The per-record core of the device BAM reader (csrc/cv_bam_core.hpp) in its host form, built here with AddressSanitizer
and UBSan (tests/native/bam_core_driver.cpp keeps every stream, record table, segment and SEQ buffer in a heap block of
exactly its size).  The records of the GPU test's inputs must give the take decisions, segments, SEQ bytes and flags that
the Python restatement in bam_device_cases.py gives; the walk from the anchors of the .bai must give the record starts
the BAM writer knows; and a few thousand seeded damaged streams must each be refused or come out exactly as the
restatement takes them -- without a sanitizer report.  The GPU test of damaged inputs rests on this one: the kernels
run the same functions."""
import os
import shutil
import struct
import subprocess

import pytest

import bam_device_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
MUTATIONS = 4000
WHOLE = (0, 2308, 0, 1 << 40)                        # tid, exclude mask, beg0, end0
FILTERS = [(0, 0, 0, 1), (10, 0, 0, 1), (1 << 30, 1, 5, 1), (3, 1, 5, 1), (1 << 30, 1, 5, 0)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed: the GPU test of damaged inputs rests on this sanitized run"
    exe = str(tmp_path_factory.mktemp("bam_core") / "bam_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "bam_core_driver.cpp"), "-o", exe])
    return exe


def run(driver, tmp_path, cases):
    src, dst = str(tmp_path / "cases"), str(tmp_path / "results")
    with open(src, "wb") as fh:
        for c in cases:
            fh.write(c)
    p = subprocess.run([driver, src, dst], stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    out, res, at = open(dst, "rb").read(), [], 0
    for _c in cases:
        r, at = C.unpack_result(out, at)
        res.append(r)
    assert at == len(out)
    return res


def check(d, first, view, filt, got):
    """got: the driver's result for (d, first, view, filt) -> True if it took the stream (then everything must be
    the restatement's), False if it refused it"""
    status, stop, offs = C.py_walk(d, first, view)
    if got["status"] in (C.S_BAD, C.S_MISS):
        return False
    assert (got["status"], got["stop"], got["offs"]) == (status, stop, offs)
    assert len(got["recs"]) == len(offs)
    for k, (off, g) in enumerate(zip(offs, got["recs"])):
        want = C.py_parse(d, off, filt, 1000 + k)
        assert g[0] == want[0], (k, g[0], want[0])
        if want[0] == C.C_BIG:
            assert g == want, (k, g, want)
        if want[0] == C.C_READ:
            assert g[1:5] == want[1:5], (k, g[1:5], want[1:5])
            assert g[5] == want[5], "record %d: segments differ" % k
            assert g[6] == want[6], "record %d: SEQ bytes differ" % k
    return True


def _corner_stream(tmp_path, payload=60000):
    bam = str(tmp_path / "corner.bam")
    recs = C.corner_records()
    where = C.write_bam(bam, recs, C.corner_refs(), block_payload=payload)
    return C.inflated(bam), where, recs


def test_corner_case_records_come_out_as_the_restatement_takes_them(driver, tmp_path):
    d, where, recs = _corner_stream(tmp_path)
    first = where[0][0]
    assert first == C.first_record_offset(C.corner_refs()) and where[-1][0] + where[-1][1] == len(d)
    views = [WHOLE, (0, 2308, 9, 45), (0, 2308 | 1024, 0, 1 << 40), (0, 2308, 250, 1 << 40), (1, 2308, 0, 1 << 40)]
    cases = [(v, f) for v in views for f in FILTERS]
    got = run(driver, tmp_path, [C.pack_case(d, first, v, f) for v, f in cases])
    for (v, f), g in zip(cases, got):
        assert check(d, first, v, f, g), "refused a clean stream"
    # a view that masks duplicates takes every record of ctgA but `g3`, and ends at the read of the second contig
    g = got[len(FILTERS) * 2]
    names = [r.split("\t")[0] for r in recs]
    want = [o + 4 for (o, _n), name in zip(where, names) if name not in ("g3", "z")]
    assert g["offs"] == want and g["status"] == C.S_END and g["stop"] == where[-1][0]
    by_name = dict(zip([n for n in names if n not in ("g3", "z")], g["recs"]))
    assert [s[2] & 0xff for s in by_name["r64"][5]] == [64] and [s[2] & 0xff for s in by_name["r65"][5]] == [64, 1]
    assert [s[2] & 0xff for s in by_name["r128"][5]] == [64, 64, 1, 64, 3] and by_name["c"][6] == b"*" + b"?" * 29
    assert len(by_name["op9"][5]) == 2 and by_name["op9"][5][1][0] == 59 + 5        # code 9 moves nothing
    assert by_name["odd"][6] == C.CORNER_REF[32:39].encode() and by_name["d"][3] == 0


def test_the_walk_from_the_anchors_gives_the_record_starts_the_writer_knows(driver, tmp_path):
    ref, lines = C.random_alignments()
    bam = str(tmp_path / "r.bam")
    where = C.write_bam(bam, lines, [("ctgA", len(ref))], block_payload=60000)
    d = C.inflated(bam)
    first = where[0][0]
    # the linear index as the writer made it: one entry per 16 kbp window -> offsets in the inflated stream
    bai = open(bam + ".bai", "rb").read()
    n_bin = struct.unpack_from("<i", bai, 8)[0]
    at = 12
    for _ in range(n_bin):
        n_chunk = struct.unpack_from("<i", bai, at + 4)[0]
        at += 8 + 16 * n_chunk
    n_intv = struct.unpack_from("<i", bai, at)[0]
    voffs = struct.unpack_from("<%dQ" % n_intv, bai, at + 4)
    coff_to_inflated = {m[0]: m[2] for m in C.members(bam)}
    anchors = sorted(set(coff_to_inflated[v >> 16] + (v & 0xffff) for v in voffs) - {first})
    assert len(anchors) >= 2 and all(a - 0 in {o for o, _n in where} for a in anchors)
    filt = (3, 1, 5, 1)
    regions = [WHOLE, (0, 2308, 8999, 21000)]
    got = run(driver, tmp_path, [C.pack_case(d, first, v, filt, anchors) for v in regions] +
              [C.pack_case(d, first, WHOLE, filt, [anchors[0] + 7] + anchors[1:])])
    assert got[0]["refused"] == 0 and got[0]["walkers"] == len(anchors) + 1
    assert got[0]["offs"] == [o + 4 for o, _n in where] and got[0]["status"] == C.S_LANDED
    assert got[1]["refused"] == 0 and 0 < len(got[1]["offs"]) < len(where)
    assert got[2]["refused"] == 1, "a walker that misses its anchor must refuse the slab"
    for v, g in zip(regions, got):
        assert check(d, first, v, filt, g)


def test_damaged_streams_are_refused_or_right(driver, tmp_path):
    d, where, _recs = _corner_stream(tmp_path)
    first = where[0][0]
    starts = [o for o, _n in where]
    streams = list(C.mutations(d, starts, MUTATIONS, seed=77))
    filt = (3, 1, 5, 1)
    anchors = [starts[5], starts[11]]
    got = run(driver, tmp_path, [C.pack_case(m, first, WHOLE, filt, [a for a in anchors if a < len(m)]) for m in streams])
    taken = sum(check(m, first, WHOLE, filt, g) for m, g in zip(streams, got))
    refused = len(streams) - taken
    anchored_refusals = sum(g["refused"] for g in got)
    print("%d damaged streams: %d refused, %d taken as the restatement takes them; the anchored walk refused %d"
          % (len(streams), refused, taken, anchored_refusals))
    assert refused > 100 and taken > 100 and anchored_refusals >= refused
