"""The arithmetic of the device's VCF merge (csrc/cv_vcfmerge_core.hpp) in its host form.

tests/native/vcf_merge_driver.cpp is built here with AddressSanitizer and UBSan as a stand-alone program (nothing is
loaded into this interpreter under a sanitizer): the per-line function over truncated and mutated lines, each in a heap
block of exactly its length; the record copy at all 16 x 16 phases of source and destination; the merge and the windows
against std::stable_sort and a per-record loop.  Then cv_vcf_merge_host_form / cv_vcf_windows_host_form, loaded the
ordinary way, against the Python definition on every case: fields, verdicts, order, text, chunk and window tables."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vcf_merge_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("vcf_merge_core") / "vcf_merge_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "vcf_merge_driver.cpp"),
                           "-o", exe])
    return exe


def test_the_core_under_the_sanitizers(driver):
    p = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    m = re.match(r"ok (\d+) lines, (\d+) vouched for, (\d+) copies, (\d+) merged records", p.stdout.decode())
    assert m, p.stdout
    lines, vouched, copies, merged = (int(g) for g in m.groups())
    # 16 x 16 phases x 19 lengths; lines of both kinds; every record count of the cases and the long-record set
    assert copies == 16 * 16 * 19 and 1000 < vouched < lines - 1000 and merged >= 4 * (1 + 63 + 64 + 65 + 257 + 2000 + 130)


@pytest.mark.parametrize("total", vc.COUNTS)
def test_the_host_forms_equal_the_definition(total):
    from clairvoyante_amd import vcf_merge
    per = vc.records(total)
    a = vc.line_arrays(per)
    o = vc.host_form(a)
    lines, t = vcf_merge._host_order(vc.HEADER, [b"".join(x) for x in per], None)
    n = a["n"]
    assert n == total == len(lines) and o["info"].tolist()[:3] == [0, len(t.crank), a["n_text"]]
    assert o["text"][:a["n_text"]].tobytes() == b"".join(lines) == b"".join(vc.expected_order(per))
    want = [vc.interval(ln) for ln in lines]
    assert o["sbeg"][:n].tolist() == [b for _c, b, _e in want] and o["send"][:n].tolist() == [e for _c, _b, e in want]
    assert [a["names"][r] for r in o["srank"][:n].tolist()] == [c for c, _b, _e in want]
    assert o["ooff"].tolist() == np.concatenate(([0], np.cumsum([len(x) for x in lines]))).astype(np.int64).tolist()
    got = vcf_merge._Tables()
    got.names = a["names"]
    nc = int(o["info"][1])
    got.crank, got.cbin, got.cubeg, got.cuend = (o["chunks"][k][:nc] for k in range(4))
    got.first, got.last, got.count = o["stats"][0], o["stats"][1], o["stats"][2]
    got.win_off, got.win = o["win_off"], o["win"][:int(o["win_off"][-1])]
    assert t.names == a["names"] or total == 0
    t.names = got.names
    assert got.same(t)


def test_lines_the_device_does_not_vouch_for_are_counted():
    """every hand-over of test_gpu_vcf_merge.py that the per-line function decides (the byte rule and the line cap are the
    item pass's)"""
    per = vc.records(65)
    bad = [vc.rec("chr1", 15000000, "A", "<DEL>", info="SVTYPE=DEL;END=15100000"), vc.rec("chr1", 5, "A", "C", info="END=7"),
           vc.rec("chr1", 1 << 29, "AC", "A"), vc.rec("chr2", 77, "A", "C").replace(b"\t", b" ", 1)]
    for k, ln in enumerate(bad):
        mine = [list(x) for x in per]
        mine[3].insert(k, ln)
        o = vc.host_form(vc.line_arrays(mine))
        assert o["info"][0] == 1, ln
