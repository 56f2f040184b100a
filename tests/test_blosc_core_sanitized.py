"""The decode core of the device's .bin block reader (csrc/cv_lz4_core.hpp) in its host form, built here with
AddressSanitizer and UBSan (tests/native/lz4_core_driver.cpp gives every chunk, stream and plane heap blocks of exactly
their sizes): the whole corpus of the GPU test must decode to cv_blosc_decompress's bytes, and 20 000 seeded damaged
chunks must each be refused (HOST) or be exactly what the host decoder makes of them -- without a sanitizer report.
The GPU test of damaged chunks rests on this one: the kernels run the same functions."""
import os
import shutil
import struct
import subprocess

import pytest

import blosc_cases as B

HERE = os.path.dirname(os.path.abspath(__file__))
MUTATIONS = 20000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("lz4_core") / "lz4_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "lz4_core_driver.cpp"), "-o", exe])
    return exe


def run(driver, tmp_path, chunks):
    """chunks -> [bytes or None (HOST)]"""
    src, dst = str(tmp_path / "records"), str(tmp_path / "results")
    with open(src, "wb") as fh:
        for c in chunks:
            fh.write(struct.pack("<I", len(c)) + c)
    p = subprocess.run([driver, src, dst], stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    out, res, at = open(dst, "rb").read(), [], 0
    for _c in chunks:
        status = out[at]; at += 1
        assert status in (B.OK, B.HOST)
        if status == B.OK:
            n = struct.unpack_from("<I", out, at)[0]; at += 4
            res.append(out[at:at + n]); at += n
        else:
            res.append(None)
    assert at == len(out)
    return res


def test_the_corpus_decodes_to_the_host_decoders_bytes(driver, tmp_path):
    corpus = B.corpus()
    got = run(driver, tmp_path, [c for _n, c in corpus])
    for (name, chunk), g in zip(corpus, got):
        want = B.host_decompress(chunk)
        assert want is not None, name
        if B.unsupported(chunk):
            assert g is None, "%s: typesize %d is not for the device" % (name, chunk[3])
            continue
        assert g is not None, "%s came back HOST" % name
        assert g == want, name


def test_a_last_sequence_without_literals_is_refused(driver, tmp_path):
    assert run(driver, tmp_path, [B.zero_literal_ending()]) == [None]


def test_damaged_chunks_are_refused_or_right(driver, tmp_path):
    # (the last 2 000 are damaged copies of the equal-payload blocks: the GPU test gives the first 300 of them to the device)
    chunks = list(B.mutations(MUTATIONS, seed=1234)) + list(B.mutations(2000, seed=4321, base=B.equal_payload_base()[0]))
    assert len(chunks) >= 20000
    got = run(driver, tmp_path, chunks)
    accepted = valid = 0
    for k, (c, g) in enumerate(zip(chunks, got)):
        want = B.host_decompress(c)
        valid += want is not None
        if g is not None:
            accepted += 1
            assert want is not None, "mutation %d: accepted a chunk the host decoder refuses" % k
            assert g == want, "mutation %d: bytes differ from the host decoder's" % k
    print("%d damaged chunks: %d still valid for the host decoder, %d accepted by the core" % (len(chunks), valid, accepted))
    assert accepted <= valid < len(chunks) // 2
