"""The arithmetic of the device's text-row formatter (csrc/cv_rowtext_core.hpp) in its host form, built here with
AddressSanitizer and UBSan as a stand-alone program (tests/native/rowtext_core_driver.cpp; nothing is loaded into this
interpreter).  The driver holds every value to snprintf("%0.1f") and to the host formatter's predicate, and every row
the device would vouch for -- assembled lane by lane as the kernel assembles it, into a heap block of exactly its length
-- to the row printf gives; 20 000 of its rows are random bit patterns.  The kernel runs the same text and is held to
cv_format_tensor_row by test_gpu_rowtext.py."""
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
    exe = str(tmp_path_factory.mktemp("rowtext_core") / "rowtext_core_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "rowtext_core_driver.cpp"),
                           "-o", exe])
    return exe


def test_the_core_prints_what_printf_prints(driver):
    p = subprocess.run([driver, "1", "20000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    m = re.match(r"ok (\d+) rows, (\d+) on the device side, (\d+) bytes", p.stdout.decode())
    assert m, p.stdout
    rows, vouched, nbytes = (int(g) for g in m.groups())
    assert rows >= 22000 and vouched >= 2000 and nbytes > 2000 * 1600
