"""The host plan of the device BAM reader (cv_bam_view_plan in csrc/cv_bam.cpp), no GPU: slabs of whole BGZF members that
tile the view's file range, member tables in cv_bgzf_scan's row format, anchors that are true record starts, the first
record's offset, and the host inflate of a member."""
import ctypes
import os
import struct
import zlib

import numpy as np
import pytest

import bam_device_cases as C


def plan(bam, ctg, start, end, slab_bytes):
    """-> (usable, [dict per slab])"""
    from clairvoyante_amd import _lib
    from clairvoyante_amd.bam import BamFile
    bf = BamFile(bam, threads=2)
    lib = bf.lib
    usable = ctypes.c_int(-1)
    _lib.check(lib.cv_bam_view_plan_begin(bf.h, ctg.encode(), int(start or 0), int(end or 0), 2308, ctypes.byref(usable)))
    slabs = []
    blob = open(bam, "rb").read()
    while usable.value:
        info = (ctypes.c_int64 * 8)()
        comp = ctypes.c_void_p(); table = ctypes.c_void_p(); anchors = ctypes.c_void_p()
        _lib.check(lib.cv_bam_view_plan(bf.h, slab_bytes, info, ctypes.byref(comp), ctypes.byref(table), ctypes.byref(anchors)))
        if info[0] == 0:
            break
        t = np.ctypeslib.as_array(ctypes.cast(table, ctypes.POINTER(ctypes.c_int64)), shape=(info[0], 4)).copy()
        a = np.ctypeslib.as_array(ctypes.cast(anchors, ctypes.POINTER(ctypes.c_int64)), shape=(info[4],)).copy() if info[4] else np.zeros(0, np.int64)
        assert ctypes.string_at(comp.value, info[1]) == blob[t[0, 0]:t[0, 0] + info[1]]
        buf = ctypes.create_string_buffer(65536)
        _lib.check(lib.cv_bam_plan_inflate_host(bf.h, 0, buf))
        slabs.append(dict(table=t, anchors=a, inflated=info[2], first=info[3], eof=info[5], coff=info[6], is_first=info[7],
                          member0=buf.raw[:int(t[0, 3]) >> 32]))
        if info[5]:
            break
    bf.close()
    return usable.value, slabs


@pytest.fixture(scope="module")
def noisy_bam(tmp_path_factory):
    ref, lines = C.random_alignments()
    bam = str(tmp_path_factory.mktemp("plan") / "r.bam")
    where = C.write_bam(bam, lines, [("ctgA", len(ref)), ("zzz", 50)], block_payload=4093)
    return bam, where, lines


@pytest.mark.parametrize("slab_bytes", [1 << 26, 200000, 1])
def test_slabs_tile_the_view_with_whole_members_and_true_anchors(noisy_bam, slab_bytes):
    bam, where, lines = noisy_bam
    mem = C.members(bam)
    stream = C.inflated(bam)
    starts = {o for o, _n in where}
    usable, slabs = plan(bam, "ctgA", None, None, slab_bytes)
    assert usable == 1 and slabs[0]["is_first"] == 1 and slabs[-1]["eof"] == 1
    m0 = max(i for i, m in enumerate(mem) if m[2] <= where[0][0])
    at, seen = m0, []
    for s in slabs:
        t = s["table"]
        assert s["coff"] == mem[at][0]
        base = mem[at][2]
        for row in t:                                      # cv_bgzf_scan's rows, over the file
            off, size, inflated_at, isize = mem[at]
            assert (row[0], row[1], row[2], row[3] >> 32) == (off + 18, size - 26, inflated_at - base, isize)
            assert row[3] & 0xffffffff == zlib.crc32(stream[inflated_at:inflated_at + isize])
            at += 1
        assert s["inflated"] == sum(int(r[3]) >> 32 for r in t) and s["member0"] == stream[base:base + (int(t[0, 3]) >> 32)]
        assert sum(mem[k][1] for k in range(at - len(t), at)) >= slab_bytes or s is slabs[-1]
        assert (s["first"] == where[0][0] - base) if s is slabs[0] else s["first"] == 0
        a = s["anchors"]
        assert np.all(np.diff(a) > 0) and all(int(x) + base in starts for x in a)
        if s is slabs[0]:
            assert np.all(a > s["first"])
        seen += [int(x) + base for x in a]
    assert at == len(mem)
    # three 16 kbp windows: the first entry is the start of the view, the other two are anchors
    pos = np.asarray([int(l.split("\t")[3]) - 1 for l in lines])
    want = [where[int(np.argmax(pos >= w << 14))][0] for w in (1, 2)]
    assert len(seen) == 2 and all(x <= w for x, w in zip(seen, want)) and seen == sorted(seen)
    if slab_bytes == 1:
        assert len(slabs) == len(mem) - m0 and all(len(s["table"]) == 1 for s in slabs)


def test_a_region_starts_at_its_window_and_views_without_a_start_are_not_planned(noisy_bam, tmp_path):
    bam, where, _lines = noisy_bam
    usable, slabs = plan(bam, "ctgA", 20000, 21000, 1 << 26)
    whole = plan(bam, "ctgA", None, None, 1 << 26)[1]
    base = whole[0]["anchors"]
    assert usable == 1 and slabs[0]["coff"] > whole[0]["coff"] and len(slabs[0]["anchors"]) == 1 and len(base) == 2
    for ctg in ("zzz", "nope"):                            # no alignments / unknown: an empty view, nothing to plan
        usable, slabs = plan(bam, ctg, None, None, 1 << 26)
        assert usable == 1 and slabs == []
    nobai = str(tmp_path / "n.bam")
    C.write_bam(nobai, C.corner_records(), C.corner_refs(), index=False)
    assert plan(nobai, "ctgA", None, None, 1 << 26) == (0, [])


def test_damaged_index_entries_are_dropped(noisy_bam, tmp_path):
    """duplicates, zeros, an entry out of order, one outside every member: fewer anchors, never other ones"""
    import shutil
    bam, where, _lines = noisy_bam
    bad = str(tmp_path / "b.bam")
    shutil.copy(bam, bad)
    bai = bytearray(open(bam + ".bai", "rb").read())
    # ctgA's linear index: 3 entries, followed by zzz's n_bin = 0 and n_intv = 0
    at = len(bai) - 8 - 24
    assert struct.unpack_from("<i", bai, at - 4)[0] == 3
    v = list(struct.unpack_from("<3Q", bai, at))
    for entries, n_anchors in (([v[0], v[1], v[1]], 1), ([v[0], 0, v[2]], 1), ([v[0], v[2], v[1]], 1), ([v[0], v[1] + (5 << 16), v[2]], 1),
                               ([v[0], v[1], v[2]], 2)):
        bai[at:at + 24] = struct.pack("<3Q", *entries)
        open(bad + ".bai", "wb").write(bytes(bai))
        usable, slabs = plan(bad, "ctgA", None, None, 1 << 26)
        assert usable == 1 and len(slabs[0]["anchors"]) == n_anchors, entries


def test_null_arguments_are_errors():
    from clairvoyante_amd import _lib
    lib = _lib.load()
    i8 = (ctypes.c_int64 * 8)()
    for rc in (lib.cv_bam_view_plan_begin(None, b"c", 0, 0, 0, None), lib.cv_bam_view_plan(None, 1, i8, None, None, None),
               lib.cv_bam_plan_inflate_host(None, 0, None), lib.cv_bam_view_params(None, i8)):
        assert rc == 1 and lib.cv_last_error()
