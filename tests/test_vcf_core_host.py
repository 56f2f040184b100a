"""The arithmetic of the device's VCF formatter (csrc/cv_vcf_core.hpp) in its host form, built here with
AddressSanitizer and UBSan as a stand-alone program (tests/native/vcf_core_driver.cpp, linked with cv_hostio.cpp; nothing
is loaded into this interpreter).  The driver holds the integer of every quality the core vouches for to libm's over a
million random fp32 pairs and over the doubles around exp(-k / 4.343), measures how far the core's own log strays from
libm's (the margin rule is sound only below M/16), and holds every vouched record -- written into a heap block of exactly
its length -- to the bytes cv_format_vcf gives for that candidate alone: 20 000 random candidates and the edges by hand.
The kernels run the same text and are held to it by test_gpu_vcf_format.py."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "clairvoyante_amd", "csrc")
M = 2.0 ** -40


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("vcf_core") / "vcf_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-pthread", "-msse2",
                           os.path.join(HERE, "native", "vcf_core_driver.cpp"), os.path.join(CSRC, "cv_hostio.cpp"),
                           os.path.join(CSRC, "cv_inflate.cpp"), "-lz", "-o", exe])
    p = subprocess.run([exe, "1", "1000000", "20000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, err = p.stdout.decode(), p.stderr.decode("utf-8", "replace")
    print(out)
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    lines = out.splitlines()
    assert lines[-1] == "ok", out
    parts = {}
    for line in lines[:-1]:
        name, rest = line.split(" ", 1)
        parts[name] = {k: float(v) for k, v in re.findall(r"(\w+)=(\S+)", rest)}
    return parts


def test_every_vouched_integer_is_libms(report):
    r = report["integer"]
    assert r["pairs"] >= 1000000 and r["built"] >= 3001 * 17
    assert r["pairs_host"] * 100000 <= r["pairs"]               # hand-overs for the margin: at most 1 in 10^5
    assert r["built_host"] > 0                                  # the built near-integer ratios do reach the margin
    assert r["max_dev"] <= M / 16, r                            # the rule's premise, measured


def test_every_vouched_record_is_the_host_formatters(report):
    r = report["records"]
    assert r["n"] >= 20000 and r["device"] + r["none"] + r["host"] == r["n"]
    assert r["device"] >= 10000 and r["none"] > 0
    for why in ("decision", "quality", "depth", "contig", "position", "sequence", "centre", "af"):
        assert r[why] > 0, why                                  # every reason was met
    assert sum(r[w] for w in ("decision", "quality", "depth", "contig", "position", "sequence", "centre", "af")) == r["host"]
    assert r["eligible"] >= 10000 and r["eligible_device"] * 10 >= r["eligible"] * 9


def test_the_edges(report):
    assert report["edges"]["n"] >= 60
