"""The DEFLATE decode core of the device's BGZF reader (csrc/cv_inflate_core.hpp) in its host form, built here with
AddressSanitizer and UBSan (tests/native/bgzf_core_driver.cpp gives every member heap blocks of exactly its sizes):
the whole corpus of the GPU test must inflate to zlib's bytes, and 20 000 seeded damaged members must each be refused
(HOST) or be exactly what zlib makes of them -- without a sanitizer report.  The GPU test of damaged members rests on
this one: the kernel runs the same functions."""
import os
import shutil
import struct
import subprocess
import zlib

import pytest

import bgzf_cases as B

HERE = os.path.dirname(os.path.abspath(__file__))
MUTATIONS = 20000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("bgzf_core") / "bgzf_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "bgzf_core_driver.cpp"), "-o", exe])
    return exe


def run(driver, tmp_path, members):
    """members: [(data, isize, crc)] -> [bytes or None (HOST)]"""
    src, dst = str(tmp_path / "records"), str(tmp_path / "results")
    with open(src, "wb") as fh:
        for data, isize, crc in members:
            fh.write(struct.pack("<III", len(data), isize, crc) + data)
    p = subprocess.run([driver, src, dst], stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    out, res, at = open(dst, "rb").read(), [], 0
    for _data, isize, _crc in members:
        status = out[at]; at += 1
        assert status in (B.OK, B.HOST)
        if status == B.OK:
            res.append(out[at:at + isize]); at += isize
        else:
            res.append(None)
    assert at == len(out)
    return res


def test_the_corpus_inflates_to_zlibs_bytes(driver, tmp_path):
    corpus = B.corpus() + B.small_corpus()
    got = run(driver, tmp_path, [(data, len(raw), zlib.crc32(raw)) for _n, data, raw in corpus])
    for (name, _data, raw), g in zip(corpus, got):
        assert g is not None, "%s came back HOST" % name
        assert g == raw, name


def test_damaged_members_are_refused_or_right(driver, tmp_path):
    members = list(B.mutations(MUTATIONS, seed=1234))
    assert len(members) >= 20000
    got = run(driver, tmp_path, members)
    accepted = valid = 0
    for k, ((data, isize, crc), g) in enumerate(zip(members, got)):
        want = B.zlib_verdict(data, isize, crc)
        valid += want is not None
        if g is not None:
            accepted += 1
            assert want is not None, "mutation %d: accepted a member zlib refuses" % k
            assert g == want, "mutation %d: bytes differ from zlib's" % k
    print("%d damaged members: %d still valid for zlib, %d accepted by the core" % (len(members), valid, accepted))
    assert accepted <= valid < len(members) // 2
