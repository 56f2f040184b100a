"""The device's BGZF compressor (csrc/cv_bgzf_deflate_core.hpp) in its host form.  zlib is the judge of every member, not
its model: no independent encoder writes zlib's bytes.

tests/native/bgzf_deflate_driver.cpp is built here with AddressSanitizer and UBSan as a stand-alone program (nothing is
loaded into this interpreter under a sanitizer): every length 0 .. 300 and the block's limits, runs across the 258
boundary, periods 2 to 4, random bytes (stored), a copy exactly 32 768 and 32 769 bytes back, a text without any match,
the code builder over Fibonacci histograms.  Then cv_bgzf_deflate_host_form, loaded the ordinary way, over three texts of
the project's own formatters at four block sizes, and the two size conditions that keep a silent fall to stored or
literal-only blocks from passing."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bgzf_deflate_cases as bc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("bgzf_deflate_core") / "bgzf_deflate_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", os.path.join(HERE, "native", "bgzf_deflate_driver.cpp"),
                           "-o", exe])
    return exe


def test_the_core_under_the_sanitizers(driver):
    p = subprocess.run([driver], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = p.stderr.decode("utf-8", "replace")
    assert p.returncode == 0 and "runtime error" not in err and "Sanitizer" not in err, err[-4000:]
    m = re.match(r"ok (\d+) members, (\d+) stored, (\d+) fixed, (\d+) dynamic", p.stdout.decode())
    assert m, p.stdout
    members, stored, fixed, dynamic = (int(g) for g in m.groups())
    # 301 lengths, 4 limits, 7 runs, 3 periods, 2 random, 2 windows, 1 without a match; every block type occurs
    assert members == 301 + 4 + 7 + 3 + 2 + 2 + 1 and stored >= 2 and fixed > 0 and dynamic > 100


@pytest.mark.parametrize("block", bc.BLOCKS)
@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_zlib_accepts_every_member(name, block):
    from clairvoyante_amd import utils_v2
    text = bc.fixture(name)
    data, sizes, info = bc.host_form(text, block)
    kinds = bc.judge(data, sizes, text, block)
    members = -(-len(text) // block)
    assert len(sizes) == members and info[0] == len(data) and info[1] == members
    assert [kinds.count(k) for k in (0, 1, 2)] == info[2:5].tolist() and info[2:5].sum() == members
    whole = np.frombuffer(data + utils_v2.BgzfWriter.EOF, dtype=np.uint8)
    table, total = utils_v2.bgzf_scan(whole)                     # the project's own reader takes the file
    assert total == len(text)
    import io
    fh = io.BytesIO()
    with utils_v2.BgzfWriter(fh, block=block, threads=1, deflate="host") as w:
        w.write(text)
    host_table, _ = utils_v2.bgzf_scan(np.frombuffer(fh.getvalue(), dtype=np.uint8))
    assert (table[:, 3] >> 32).tolist() == (host_table[:, 3] >> 32).tolist()     # the ISIZE list is the host writer's
    assert table[:, 2].tolist() == host_table[:, 2].tolist() and len(table) == len(host_table) >= members


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_the_members_are_about_zlib_level_1_in_size(name):
    """at most 1.10 x the members zlib's level 1 (one hash candidate, greedy -- the like-for-like yardstick) makes of the
    same cuts: a fall to fixed codes costs 1.07 - 1.28 x, the loss of the near distances 1.15 x on tensor rows"""
    from clairvoyante_amd import utils_v2
    text = bc.fixture(name)
    block = 65280
    data, sizes, info = bc.host_form(text, block)
    level1 = sum(len(utils_v2.BgzfWriter.member(text[at:at + block], level=1)) for at in range(0, len(text), block))
    level6 = sum(len(utils_v2.BgzfWriter.member(text[at:at + block], level=6)) for at in range(0, len(text), block))
    print("%s: %d bytes, %.3f x level 1, %.3f x level 6" % (name, len(data), len(data) / level1, len(data) / level6))
    assert info[4] == len(sizes)                                 # text like this: every block dynamic
    assert len(data) <= 1.10 * level1


@pytest.mark.parametrize("name,text", bc.special_texts(), ids=[n for n, _t in bc.special_texts()])
def test_the_special_texts(name, text):
    data, sizes, info = bc.host_form(text, 65280)
    kinds = bc.judge(data, sizes, text, 65280)
    if name == "random":
        assert kinds == [0]
    elif name == "window 32768":
        assert len(data) < 700                                   # the second R is two matches, 32 768 back
    elif name == "window 32769":
        assert len(data) > 600                                   # ... and literals when it lies one byte further
    elif name == "no match":
        assert kinds == [2]
    else:
        assert len(data) < 60


def test_small_members_and_the_empty_text():
    for n in list(range(0, 70)) + [255, 256, 257, 258, 259, 260]:
        text = bc.fixture("vcf_records")[:n]
        data, sizes, info = bc.host_form(text, 65280)
        assert len(sizes) == 1                                   # an empty text is one empty member
        bc.judge(data, sizes, text, 65280)


@pytest.mark.parametrize("members,block", bc.TWO_TRIPS)
def test_the_two_trip_text_alternates_its_block_types(members, block):
    """what test_gpu_bgzf_deflate.py's multi-tile case claims: more members than workgroups, every member a whole block of
    16 or 255 tiles, members m and m + 512 of different block types, and in a text member matches that reach further back
    than one tile of 256 positions, by the hundred (the member's own distances, read from its DEFLATE block)"""
    text = bc.two_trip_text(members, block)
    assert members > bc.WORKGROUPS == 512 and len(text) == members * block and block // 256 in (16, 255)
    data, sizes, info = bc.host_form(text, block)
    kinds = bc.member_kinds(data, sizes)
    assert [kinds.count(k) for k in (0, 1, 2)] == info[2:5].tolist() and info[2] > 0 and info[4] > 0
    assert all(kinds[m] != kinds[m + bc.WORKGROUPS] for m in range(members - bc.WORKGROUPS)) and members - bc.WORKGROUPS in (77, 3)
    assert all((kinds[m] == 2) == bc.two_trip_kind(m) and kinds[m] in (0, 2) for m in range(members))
    half = block // 2
    for m in (0, 2, bc.WORKGROUPS + 1):                         # (a first trip's, and a second trip's)
        assert bc.two_trip_kind(m) and text[m * block:m * block + half] == text[m * block + half:(m + 1) * block] and half > 256
        at = int(np.sum(sizes[:m]))
        far = [d for d in bc.match_distances(data[at:at + int(sizes[m])]) if d > 256]
        assert len(far) > block // 40 and max(far) > block // 4, (m, len(far))
    if block == 4096:
        assert bc.judge(data, sizes, text, block) == kinds


def test_an_output_too_small_for_its_members():
    """nothing of a member that does not fit is written, the rest keeps what it held, info[0] names the full need; zlib
    judges the members a cap of whole members holds"""
    text = bc.fixture("vcf_records")[:9 * 1000 + 123]
    full, sizes, info = bc.host_form(text, 1000)
    off = np.concatenate(([0], np.cumsum(sizes)))
    assert len(sizes) == 10 and info[0] == len(full)
    for cap, fit in bc.small_output_caps(sizes):
        out, s, i = bc.host_form(text, 1000, out_cap=cap, fill=0x5A)
        edge = int(off[fit])
        assert s.tolist() == sizes.tolist() and i.tolist() == info.tolist() and edge <= cap
        assert out[:edge] == full[:edge] and out[edge:] == b"\x5a" * (len(out) - edge), cap
        if edge == cap and fit:
            bc.judge(out[:edge], sizes[:fit], text[:fit * 1000], 1000)


def test_arguments_are_checked():
    import ctypes
    from clairvoyante_amd import _lib
    lib = _lib.load()
    a = np.zeros(64, dtype=np.uint8)
    V = lambda x: ctypes.c_void_p(x.ctypes.data)
    sizes, info = np.zeros(4, dtype=np.int32), np.zeros(8, dtype=np.int64)
    assert lib.cv_bgzf_deflate_host_form(V(a), 10, 65281, V(a), 64, V(sizes), V(info)) != 0
    assert lib.cv_bgzf_deflate_host_form(V(a), 10, 0, V(a), 64, V(sizes), V(info)) != 0
    assert lib.cv_bgzf_deflate_host_form(None, 10, 64, V(a), 64, V(sizes), V(info)) != 0
    need = ctypes.c_int64()
    assert lib.cv_bgzf_deflate_workspace(1, 65280, ctypes.byref(need)) == 0 and need.value % 256 == 0
    assert need.value >= 65536 + 4 * 65280
    assert lib.cv_bgzf_deflate_workspace(0, 65280, ctypes.byref(need)) != 0
    # a member that does not fit is not written, the total still says what was needed
    text = bc.fixture("vcf_records")[:3000]
    out = np.full(200, 0xa5, dtype=np.uint8)
    src = np.frombuffer(text, dtype=np.uint8)
    assert lib.cv_bgzf_deflate_host_form(V(src), len(text), 1000, V(out), 100, V(sizes), V(info)) == 0
    assert info[0] == sizes[:3].sum() > 100 and (out == 0xa5).all()
