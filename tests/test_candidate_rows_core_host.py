"""The arithmetic of the device's candidate-row formatter (csrc/cv_candrows_core.hpp) in its host form, built here with
AddressSanitizer and UBSan as a stand-alone program (tests/native/candrows_core_driver.cpp; nothing is loaded into this
interpreter).  The driver holds cv_candidate_rows_host_form's core to an independent rendering -- snprintf for the
numbers, std::stable_sort for the seven pairs -- over its table of edge cases (counts 0 .. 2^31 - 1, a total above 2^31,
ties, positions around every power of ten, reference bytes a / N / 0x7F / 0x80, contig names of 1, 255 and 256 bytes, a
text_cap one byte short of the last row) and a few thousand random entries; every row is assembled into a heap block of
exactly its length.  The kernels run the same text and are held to it by test_gpu_candidate_rows.py."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("candrows_core") / "candrows_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "candrows_core_driver.cpp"),
                           "-o", exe])
    return exe


def test_the_core_prints_what_printf_and_stable_sort_print(driver):
    p = subprocess.run([driver, "1", "5000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    m = re.match(r"ok (\d+) rows, (\d+) on the device side, (\d+) bytes", p.stdout.decode())
    assert m, p.stdout
    rows, vouched, nbytes = (int(g) for g in m.groups())
    # the table alone is 4 name lengths x 11 windows x 200 rows; the 256-byte name and some of every batch are the host's
    assert rows >= 8800 + 5000 and 5000 <= vouched < rows and nbytes > vouched * 30


def test_the_table_it_dumps_is_the_one_the_gpu_tests_plant(driver):
    out = subprocess.check_output([driver, "dump"]).decode().split("\n")
    counts = [[int(v) for v in l.split()[1:]] for l in out if l.startswith("C ")]
    windows = [(int(l.split()[1]), bytes.fromhex(l.split()[2])) for l in out if l.startswith("W ")]
    names = [int(l.split()[1]) for l in out if l.startswith("G ")]
    assert [5, 5, 0, 0, 5, 0, 0] in counts and [2 ** 31 - 1] * 7 in counts and all(len(c) == 7 for c in counts)
    assert any(min(c) < 0 for c in counts)
    assert len(windows) == 11 and all(set(b"aN\x7f\x80") <= set(w) for _, w in windows)
    assert max(f for f, _ in windows) + 8 >= 10 ** 10 - 1 and names == [1, 5, 255, 256]
