"""BGZF tensor files without a GPU: the writer, the member scan (cv_bgzf_scan), what counts as "not BGZF", the slab and
tail logic of utils_v2.GetTensorDevice over a stand-in device that inflates with zlib and marks every line HOST, and
callVar's choice of reader.  Batches are compared with GetTensor's bit for bit."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import textparse_cases as T


@pytest.fixture(scope="module")
def text():
    return T.volume_text(2000)


def _write(path, data):
    with open(str(path), "wb") as fh:
        fh.write(data)
    return str(path)


def _rows(fn, num=300):
    from clairvoyante_amd import utils_v2
    return T.collect(utils_v2.GetTensor(fn, num, log=False))


@pytest.mark.parametrize("level,strategy", [(0, 0), (1, 0), (6, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY)])
def test_writer_output_is_gzip_and_gives_the_same_rows(tmp_path, text, level, strategy):
    from clairvoyante_amd import utils_v2
    fn = str(tmp_path / "t.gz")
    with utils_v2.BgzfWriter(fn, level=level, strategy=strategy) as w:
        for at in range(0, len(text), 77777):
            w.write(text[at:at + 77777])
    assert subprocess.check_output(["gzip", "-dc", fn]) == text
    assert gzip.open(fn, "rb").read() == text
    data = open(fn, "rb").read()
    assert data.endswith(utils_v2.BgzfWriter.EOF)
    members = B.walk(data)
    assert [m[2] for m in members[:-1]] == [65280] * (len(text) // 65280) + [len(text) % 65280] and members[-1][2] == 0
    plain = _write(tmp_path / "t.txt", text)
    want, got = _rows(plain), _rows(fn)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and len(got[1]) > 1500
    assert utils_v2.is_bgzf(fn) and not utils_v2.is_bgzf(plain)


def test_writer_takes_bytes_that_do_not_compress(tmp_path):
    from clairvoyante_amd import utils_v2
    noise = np.random.RandomState(1).randint(0, 256, 200000).astype(np.uint8).tobytes()
    fn = str(tmp_path / "noise.gz")
    with utils_v2.BgzfWriter(fn) as w:
        w.write(noise)
    assert gzip.open(fn, "rb").read() == noise and utils_v2.is_bgzf(fn)


def test_reblock_module_and_create_tensor_option(tmp_path, text):
    from clairvoyante_amd import CreateTensor, bgzf, utils_v2
    src = str(tmp_path / "plain.gz")
    with gzip.open(src, "wb", compresslevel=1) as fh:
        fh.write(text)
    assert not utils_v2.is_bgzf(src)
    dst = str(tmp_path / "blocked.gz")
    assert bgzf.reblock(src, dst) == len(text)
    assert utils_v2.is_bgzf(dst) and gzip.open(dst, "rb").read() == text
    again = str(tmp_path / "again.gz")
    bgzf.reblock(_write(tmp_path / "plain.txt", text), again)
    assert open(again, "rb").read() == open(dst, "rb").read()
    p = CreateTensor.build_parser()
    assert p.parse_args(["--ctgName", "chr1"]).bgzf is False and p.parse_args(["--bgzf"]).bgzf is True


def test_scan_table_against_a_python_walk(tmp_path, text):
    from clairvoyante_amd import utils_v2
    for block, eof, pad in ((65280, True, 0), (1000, True, 0), (4096, False, 0), (65280, True, 512)):
        data = B.bgzf_file(text[:300000], block=block, eof=eof) + b"\0" * pad
        if block == 1000:                                    # empty members in mid-file, and other subfields in front of BC
            empty = B.bgzf_member(B.deflate(b""), 0, 0)
            cut = sum(12 + 6 + m[1] + 8 for m in B.walk(data)[:5])
            extra = B.bgzf_member(B.deflate(b"chr1 1 A\n"), 9, zlib.crc32(b"chr1 1 A\n"), extra=b"XY\x03\0abc")
            data = data[:cut] + empty + empty + extra + data[cut:]
        got = utils_v2.bgzf_scan(np.frombuffer(data, dtype=np.uint8))
        assert got is not None
        table, total = got
        want = B.walk(data)
        assert len(want) == table.shape[0] and total == sum(m[2] for m in want)
        assert [tuple(r[:2]) for r in table.tolist()] == [m[:2] for m in want]
        assert [r >> 32 for r in table[:, 3].tolist()] == [m[2] for m in want]
        assert [r & 0xffffffff for r in table[:, 3].tolist()] == [m[3] for m in want]
        assert table[:, 2].tolist() == np.concatenate(([0], np.cumsum([m[2] for m in want])[:-1])).tolist()
        assert gzip.decompress(data) == b"".join(
            zlib.decompress(data[o:o + n], -15) for o, n, _i, _c in want)


def _not_bgzf_files(text):
    """name -> bytes of files that are gzip (or nearly) but not BGZF through and through"""
    good = B.bgzf_file(text, block=20000)
    members = B.walk(good)
    second = members[1][0] - 18                             # start of the second member
    out = {}
    out["plain_gzip"] = gzip.compress(text, 6)
    out["gzip_member_in_the_middle"] = good[:second] + gzip.compress(text[20000:40000]) + good[members[2][0] - 18:]
    out["extra_field_without_bc"] = good[:second] + (
        b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0XY\x02\0zz" + B.deflate(text[20000:40000]) +
        struct.pack("<II", zlib.crc32(text[20000:40000]), 20000)) + good[members[2][0] - 18:]
    out["file_name_flag"] = b"\x1f\x8b\x08\x0c" + good[4:12] + good[12:18] + b"name\0" + good[18:]
    big = text[:70000]
    out["isize_above_65536"] = B.bgzf_member(B.deflate(big), len(big), zlib.crc32(big)) + good
    b = bytearray(good); struct.pack_into("<H", b, len(good) - 28 + 16, 4000)
    out["bsize_past_the_file"] = bytes(b)
    return out, good


def test_not_bgzf_sends_the_whole_file_down_todays_path(tmp_path, text, monkeypatch):
    from clairvoyante_amd import utils_v2
    text = text[:100000]
    files, good = _not_bgzf_files(text)
    want = _rows(_write(tmp_path / "plain.txt", text))
    assert utils_v2.is_bgzf(_write(tmp_path / "good.gz", good))
    monkeypatch.setattr(utils_v2, "_TextSlabDevice", B.ZlibSlabDevice)
    for name, data in sorted(files.items()):
        fn = _write(tmp_path / (name + ".gz"), data)
        assert utils_v2.bgzf_scan(np.frombuffer(data, dtype=np.uint8)) is None, name
        assert not utils_v2.is_bgzf(fn)
        readable = subprocess.run(["gzip", "-dc", fn], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        if readable.returncode == 0 and readable.stdout == text:         # (the others are damaged files, for gzip too)
            got = _rows(fn)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], name
            dev = T.collect(utils_v2.GetTensorDevice(fn, 300, "cpu", log=False))
            assert np.array_equal(dev[0], want[0]) and dev[1] == want[1], name
    # a truncated last member: not BGZF, and the stream reader reports the damage as it does today
    cut = _write(tmp_path / "truncated.gz", good[:-40])
    assert not utils_v2.is_bgzf(cut)
    assert sorted(files) == ["bsize_past_the_file", "extra_field_without_bc", "file_name_flag", "gzip_member_in_the_middle",
                             "isize_above_65536", "plain_gzip"]


def _bad_reported(capsys):
    return sum(int(k) for k in re.findall(r"UnpackATensorRecord Failure \((\d+) malformed", capsys.readouterr().err))


def _same_batches(fn, plain, num, monkeypatch, capsys, slab):
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_TextSlabDevice", B.ZlibSlabDevice)
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    capsys.readouterr()
    want = T.collect(utils_v2.GetTensor(plain, num, log=False))
    bad_want = _bad_reported(capsys)
    assert utils_v2.is_bgzf(fn)
    got = T.collect(utils_v2.GetTensorDevice(fn, num, "cpu", log=False))
    bad_got = _bad_reported(capsys)
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert bad_got == bad_want
    assert got[2][-1] == 1 and not any(got[2][:-1])
    return got


@pytest.mark.parametrize("block", [700, 5000, 65280])
@pytest.mark.parametrize("slab", [4096, 65536, 1 << 20])
def test_slabs_and_tails_through_the_stand_in(tmp_path, monkeypatch, capsys, block, slab):
    """volume_text in members of 700 bytes (every line spans several), 5000 (most lines span two) and 65 280"""
    text = T.volume_text(2000)
    if block == 700:
        text = text[:1500000]
    plain = _write(tmp_path / "v.txt", text)
    fn = _write(tmp_path / "v.gz", B.bgzf_file(text, block=block, level=1))
    got = _same_batches(fn, plain, 300, monkeypatch, capsys, slab)
    assert sum(got[3]) == len(got[1]) > 250


@pytest.mark.parametrize("name", ["nonl", "off_format", "blank_then_rows", "empty", "only_eof", "no_eof_marker", "newline_only"])
def test_edge_files_through_the_stand_in(tmp_path, monkeypatch, capsys, name):
    text = {"nonl": T.volume_text(2000)[:400000].rstrip(b"\n"), "off_format": T.off_format_text()[0],
            "blank_then_rows": T.blank_then_rows_text(), "empty": b"", "only_eof": b"", "no_eof_marker": T.volume_text(2000)[:300000],
            "newline_only": b"\n"}[name]
    if name == "nonl":
        text = text[:text.rfind(b"\n") + 500]               # the last line breaks off in mid-row as well
    plain = _write(tmp_path / "e.txt", text)
    data = B.bgzf_file(text, block=3000, eof=name != "no_eof_marker")
    if name == "empty":
        data = B.bgzf_member(B.deflate(b""), 0, 0) * 3
    fn = _write(tmp_path / "e.gz", data)
    for slab in (4096, None):
        _same_batches(fn, plain, 50, monkeypatch, capsys, slab)


def test_the_member_counters_and_the_host_members(tmp_path, monkeypatch):
    """_BgzfSlab.inflate_member is the host's side of a member the device hands back: right bytes, or CvError"""
    from clairvoyante_amd import _lib, utils_v2
    text = T.volume_text(2000)[:200000]
    data = bytearray(B.bgzf_file(text, block=30000))
    table, total = utils_v2.bgzf_scan(np.frombuffer(bytes(data), dtype=np.uint8))
    slab = utils_v2._BgzfSlab(np.frombuffer(bytes(data), dtype=np.uint8), table, "x.gz")
    assert slab.n == total == len(text)
    assert b"".join(slab.inflate_member(i).tobytes() for i in range(len(table))) == text
    data[int(table[2, 0]) + 100] ^= 0x10
    slab = utils_v2._BgzfSlab(np.frombuffer(bytes(data), dtype=np.uint8), table, "x.gz")
    assert slab.inflate_member(1).tobytes() == text[30000:60000]
    with pytest.raises(_lib.CvError, match="gzip stream broke off after 60000 bytes: x.gz"):
        slab.inflate_member(2)
    assert set(utils_v2.bgzf_member_counts) == {"device", "host"}


def test_parser_choice_with_the_bgzf_constant(tmp_path, monkeypatch, text):
    from clairvoyante_amd import callVar
    monkeypatch.delenv("CV_TEXT_PARSE", raising=False)
    bg = _write(tmp_path / "b.gz", B.bgzf_file(text[:200000]))
    gz = _write(tmp_path / "g.gz", gzip.compress(text[:200000]))
    plain = _write(tmp_path / "p.txt", text[:200000])
    assert isinstance(callVar.TEXT_DEVICE_MIN_BYTES, tuple) and len(callVar.TEXT_DEVICE_MIN_BYTES) == 2
    monkeypatch.setattr(callVar, "TEXT_DEVICE_MIN_BYTES", (None, None))
    monkeypatch.setattr(callVar, "BGZF_DEVICE_MIN_BYTES", None)                # never
    assert not callVar.parses_on_device(bg) and not callVar.parses_on_device(gz) and not callVar.parses_on_device(plain)
    size = os.path.getsize(bg)
    monkeypatch.setattr(callVar, "BGZF_DEVICE_MIN_BYTES", size)                 # a file at the threshold ...
    assert callVar.parses_on_device(bg) and not callVar.parses_on_device(gz) and not callVar.parses_on_device(plain)
    monkeypatch.setattr(callVar, "BGZF_DEVICE_MIN_BYTES", size + 1)             # ... and one byte below it
    assert not callVar.parses_on_device(bg)
    monkeypatch.setattr(callVar, "TEXT_DEVICE_MIN_BYTES", (None, 1))            # an ordinary .gz follows its own floor, BGZF its own
    assert callVar.parses_on_device(gz) and not callVar.parses_on_device(bg)
    monkeypatch.setattr(callVar, "BGZF_DEVICE_MIN_BYTES", None)                 # never means never
    assert callVar.parses_on_device(gz) and not callVar.parses_on_device(bg)
    monkeypatch.setenv("CV_TEXT_PARSE", "host")
    assert not callVar.parses_on_device(bg)
    monkeypatch.setenv("CV_TEXT_PARSE", "device")
    assert callVar.parses_on_device(bg) and callVar.parses_on_device(gz)
