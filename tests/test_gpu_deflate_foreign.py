"""The device's DEFLATE decoders (csrc/cv_inflate_dev.hip, csrc/cv_gzip_dev.hip, and the BAM route on top of the first)
over streams zlib does not write: the members of tests/foreign_cases.py, made bit by bit, and what libdeflate wrote.  The
checker is zlib, byte for byte.  NO valid member may come back HOST and none of the BAM's members may be refused: the host
fallback must not hide a decoder that only takes zlib's streams (tests/test_deflate_foreign_host.py shows the same core
takes them all in its host form, and refuses the invalid ones, under sanitizers)."""
import os
import types
import zlib

import numpy as np
import pytest

import bam_writer
import bgzf_cases as B
import common
import deflate_writer as W
import foreign_cases as F
import textparse_cases as T
from test_gpu_bam_device import clean, feed
from test_gpu_bgzf import device_inflate as bgzf_inflate
from test_gpu_gzip import device_inflate as gzip_inflate
from test_gpu_pileup import _same

pytestmark = pytest.mark.gpu


def _write(path, data):
    with open(str(path), "wb") as fh:
        fh.write(data)
    return str(path)


# ---- BGZF members ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 5])
def test_every_valid_member_inflates_on_the_device(offset):
    members = F.valid() + F.libdeflate_members()
    status, outs, intact = bgzf_inflate([(m.data, len(m.raw), zlib.crc32(m.raw)) for m in members], offset)
    assert intact
    for m, s, o in zip(members, status, outs):
        assert s == B.OK, "%s came back %d" % (m.name, s)
        assert o == m.raw, m.name


def test_every_invalid_member_goes_back_to_the_host():
    """with the size the tokens would give, and with room to spare: the refusal is not the output range's"""
    bad = F.invalid()
    members = [(data, isize, 0) for _n, data, isize in bad] + [(data, isize + 300, 0) for _n, data, isize in bad]
    status, _outs, intact = bgzf_inflate(members)
    assert intact
    assert list(status) == [B.HOST] * len(members), [n for (n, _d, _i), s in zip(bad + bad, status) if s != B.HOST]


# ---- ordinary gzip files ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing,slab", [(4096, None), (1024, 4096)])
@pytest.mark.parametrize("name", ["volume300_level6.gz", "volume300_level12.gz", "writer"])
def test_gzip_files_of_other_writers(tmp_path, monkeypatch, name, spacing, slab):
    """libdeflate's blocks are few and long, and cv_gzip_header_at finds every one of their starts but the final block's
    (test_deflate_foreign_host.py asserts that): nothing may go to the host.  The writer's file mixes headers the finder
    does not take (a single distance code, none) among complete ones: their blocks stay with the chunk in front."""
    if name == "writer":
        data, text, _blocks = F.writer_gzip()
    else:
        data, text = F.fixture(name), T.volume_text(300)
    got, device, host, _slabs = gzip_inflate(_write(tmp_path / "f.gz", data), monkeypatch, spacing=spacing, slab=slab)
    print("%s: %d device chunks, %d hand-overs" % (name, device, host))
    assert got == text
    assert host == 0 and device >= 3


# ---- BAM -------------------------------------------------------------------------------------------------------------------
def _noisy_ref():
    return "".join(l.strip() for l in open(os.path.join(F.PILEUP, "noisy.fa")) if not l.startswith(">"))


def test_bam_files_of_other_writers(tmp_path):
    """the committed libdeflate BAM and one whose members the bit writer made (code depths 7, 9, 12, 15 in turn, matches up
    to 32 768 back) against the zlib-written BAM of the same records, through both routes"""
    ref, recs, refs = _noisy_ref(), F.noisy_records(), F.noisy_refs()
    plain = str(tmp_path / "zlib.bam")
    bam_writer.write_bam(plain, recs, refs, block_payload=9001)
    turn = [0]

    def by_the_writer(data):
        turn[0] += 1
        return W.compress(data, F.DEPTHS[turn[0] % 4], per_block=1500, joint=bool(turn[0] % 2))
    written = str(tmp_path / "writer.bam")
    bam_writer.write_bam(written, recs, refs, block_payload=40000, compress=by_the_writer)
    assert turn[0] >= 2
    centers = np.arange(20, len(ref) - 20, 7, dtype=np.int64)
    for kw in (dict(evc=True, retain=True, dcov=3, minMQ=3, evc_minMQ=5), dict(centers=centers, dcov=250)):
        want, want_stats, _c = feed(plain, "host", ref=ref, **kw)
        assert want[4] > 0
        for bam in (os.path.join(F.FIXTURES, "noisy_libdeflate.bam"), written):
            h, hs, hc = feed(bam, "host", ref=ref, **kw)
            d, ds, dc = feed(bam, "device", ref=ref, **kw)
            assert hc["host_views"] == 1 and hc["device_views"] == 0
            _same(want, h)
            _same(want, d)
            assert hs == want_stats and ds == want_stats
            clean(dc)                                         # no member refused: all of them inflated on the device


# ---- callVar ---------------------------------------------------------------------------------------------------------------
def test_callvar_over_a_libdeflate_bgzf_tensor_file(tmp_path, oracle, monkeypatch):
    from clairvoyante_amd import callVar, clairvoyante_v3, utils_v2
    data, text = F.libdeflate_bgzf_tensor_file()
    files = {"plain": _write(tmp_path / "t.txt", text), "bgzf": _write(tmp_path / "t.bgzf.gz", data)}
    assert utils_v2.is_bgzf(files["bgzf"])
    m = clairvoyante_v3.Clairvoyante(); m.setParameters(common.bench_params(oracle, "full"))
    chk = str(tmp_path / "full" / "model"); m.saveParameters(chk); m.close()
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    vcf = {}
    for form, side in (("plain", "host"), ("bgzf", "host"), ("bgzf", "device")):
        monkeypatch.setenv("CV_TEXT_PARSE", side)
        before = dict(utils_v2.bgzf_member_counts)
        out = str(tmp_path / ("%s_%s.vcf" % (form, side)))
        callVar.Run(types.SimpleNamespace(tensor_fn=files[form], chkpnt_fn=chk, call_fn=out, qual=0, sampleName="S", ref_fn=None, threads=None,
                                          showRef=True, v3=True, v2=False, slim=False))
        vcf[form, side] = open(out, "rb").read()
        grew = {k: utils_v2.bgzf_member_counts[k] - before[k] for k in before}
        if (form, side) == ("bgzf", "device"):
            assert grew["host"] == 0 and grew["device"] >= 4, grew       # libdeflate's four members, on the device
    assert len([l for l in vcf["plain", "host"].splitlines() if not l.startswith(b"#")]) >= 30
    assert vcf["bgzf", "host"] == vcf["plain", "host"] and vcf["bgzf", "device"] == vcf["plain", "host"]
