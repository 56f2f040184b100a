"""utils_v2.BgzfWriter's routes without a GPU: the values of CV_BGZF_DEFLATE, deflate="host" byte for byte the file as it
always was, and the slab logic of the device route (whole members leave, the tail waits, write and write_device mixed,
pieces that straddle the cuts) over the core's host form, deflate="host_form"."""
import io
import struct
import zlib

import numpy as np
import pytest

import bgzf_deflate_cases as bc
from clairvoyante_amd import _lib, utils_v2


def reference_file(text, block, level=6):
    """the file as the writer has always made it, restated with zlib alone"""
    out = []
    for at in range(0, len(text), block):
        data = text[at:at + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, 0)
        body = c.compress(data) + c.flush()
        out.append(bc.HEAD + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(data), len(data)))
    return b"".join(out) + utils_v2.BgzfWriter.EOF


def written(text_pieces, block, deflate, device_every=0, **kw):
    fh = io.BytesIO()
    w = utils_v2.BgzfWriter(fh, block=block, deflate=deflate, **kw)
    for k, p in enumerate(text_pieces):
        if device_every and k % device_every == 0:
            w.write_device(np.frombuffer(p, dtype=np.uint8))
        else:
            w.write(p)
    w.close()
    return fh.getvalue(), w


def test_the_values_of_the_switch(monkeypatch):
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    for value, want in ((None, "host"), ("", "host"), ("host", "host"), ("device", "host")):      # no GPU: the host's
        if value is None:
            monkeypatch.delenv("CV_BGZF_DEFLATE", raising=False)
        else:
            monkeypatch.setenv("CV_BGZF_DEFLATE", value)
        assert utils_v2.bgzf_deflate_route() == want
        assert utils_v2.BgzfWriter(io.BytesIO()).deflate == want
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: True)
    assert utils_v2.bgzf_deflate_route() == "device" and utils_v2.bgzf_deflate_route("host") == "host"
    for bad in ("gpu", "Device", "1"):
        monkeypatch.setenv("CV_BGZF_DEFLATE", bad)
        with pytest.raises(_lib.CvError):
            utils_v2.bgzf_deflate_route()
        with pytest.raises(_lib.CvError):
            utils_v2.BgzfWriter(io.BytesIO())
        assert utils_v2.bgzf_deflate_route("host") == "host"         # an argument is not the environment's business
    with pytest.raises(_lib.CvError):
        utils_v2.bgzf_deflate_route("zlib")


@pytest.mark.parametrize("block", (1000, None))
def test_the_host_route_is_the_file_as_it_was(block, monkeypatch):
    text = bc.fixture("vcf_records")
    want = reference_file(text, block or 65280)
    for env in (None, "host"):
        if env is None:
            monkeypatch.delenv("CV_BGZF_DEFLATE", raising=False)
        else:
            monkeypatch.setenv("CV_BGZF_DEFLATE", env)
        for threads in (1, 4):
            got, w = written([text[:777], text[777:]], block, None, threads=threads)
            assert got == want and sum(w.member_sizes) == len(got) - 28
    got, w = written([text], block, "host", threads=2)
    assert got == want
    got, _w = written([text[:5000]], block, "host", device_every=1, threads=1)   # write_device on the host route is write
    assert got == reference_file(text[:5000], block or 65280)


@pytest.mark.parametrize("block", (64, 1000))
@pytest.mark.parametrize("piece", ("1", "block-1", "block+1", "3*block+7"))
def test_pieces_and_one_write_give_the_same_members(block, piece):
    text = bc.fixture("candidate_list")[:20 * block + 13]
    step = {"1": 1, "block-1": block - 1, "block+1": block + 1, "3*block+7": 3 * block + 7}[piece]
    if step == 1:
        text = text[:3 * block + 5]
    one, w1 = written([text], block, "host_form")
    pieces = [text[at:at + step] for at in range(0, len(text), step)]
    before = utils_v2.bgzf_deflate_counts()
    for every in (0, 1, 2):                                           # write alone, write_device alone, the two mixed
        got, w = written(pieces, block, "host_form", device_every=every)
        assert got == one and w.member_sizes == w1.member_sizes
    after = utils_v2.bgzf_deflate_counts()
    members = -(-len(text) // block)
    assert after["host_form"] - before["host_form"] == 3 * members and after["host"] == before["host"]
    assert sum(after[k] - before[k] for k in ("stored", "fixed", "dynamic")) == 3 * members
    assert len(w1.member_sizes) == members and sum(w1.member_sizes) == len(one) - len(utils_v2.BgzfWriter.EOF)
    data, sizes, _info = bc.host_form(text, block)                    # the writer's members are the entry point's
    assert one == data + utils_v2.BgzfWriter.EOF and w1.member_sizes == sizes.tolist()
    bc.judge(data, sizes, text, block)


def test_slabs_leave_whole_members_and_the_tail_waits(monkeypatch):
    monkeypatch.setattr(utils_v2.BgzfWriter, "SLAB_MEMBERS", 4)
    block = 100
    text = bc.fixture("tensor_rows")[:2345]
    fh = io.BytesIO()
    w = utils_v2.BgzfWriter(fh, block=block, deflate="host_form")
    w.write(text[:399])
    assert w.member_sizes == [] and w.pending == 399               # less than a slab: nothing leaves
    w.write(text[399:450])
    assert len(w.member_sizes) == 4 and w.pending == 50            # a slab of whole members, the tail waits
    w.write_device(np.frombuffer(text[450:1999], dtype=np.uint8))
    assert len(w.member_sizes) == 16 and w.pending == 399          # three more slabs; less than a slab waits
    w.write(text[1999:])
    w.close()
    assert len(w.member_sizes) == 24 and w.pending == 0
    data, sizes, _info = bc.host_form(text, block)
    assert fh.getvalue() == data + utils_v2.BgzfWriter.EOF and w.member_sizes == sizes.tolist()
    empty = io.BytesIO()
    utils_v2.BgzfWriter(empty, deflate="host_form").close()
    assert empty.getvalue() == utils_v2.BgzfWriter.EOF               # nothing written: the marker alone, as on the host
