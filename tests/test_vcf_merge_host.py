"""vcf_merge.py as a machine without a GPU sees it: the merged order against an independent sort, the written .tbi held to
what it is for -- every region answered through it equals a brute-force overlap filter over the merged text, with fewer
BGZF members inflated than the file has --, the reader over coarsened indexes, the index's own invariants, the file
formats, the errors, and the three places users meet the merge (MergeVcf, callVarBamParallel --merged_fn, GetTruth)."""
import gzip
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest

import vcf_merge_cases as vc


@pytest.fixture(autouse=True)
def _host_route(monkeypatch):
    monkeypatch.delenv("CV_VCF_MERGE", raising=False)


@pytest.fixture(scope="module")
def merged(tmp_path_factory):
    """the 2 000-record set merged once with block=4096 -> (out_fn, records in expected order, per-file records)"""
    from clairvoyante_amd import vcf_merge
    d = tmp_path_factory.mktemp("merged")
    files, fai, per = vc.build(d, 2000)
    out = str(d / "all.vcf.gz")
    got = vcf_merge.merge(files, out, fai_fn=fai, block=4096)
    assert got["records"] == 2000 and got["route"] == "host"
    return out, vc.expected_order(per), per


def _brute(lines, ctg, beg, end):
    out = []
    for ln in lines:
        c, b, e = vc.interval(ln)
        if c == ctg and beg < end and b < end and e > beg:         # (an empty region overlaps nothing)
            out.append(ln)
    return out


def _regions(lines):
    """a few hundred regions: single positions, window and bin edges on both sides, empty regions, whole contigs, a contig
    without records, a contig the file lacks, and random ones"""
    rs = np.random.RandomState(7)
    out = []
    edges = [16382, 16383, 16384, 16385, 16386, 16387, 131070, 131071, 131072, 131073, 131074, 1048574, 1048576, 1048579, 1048580,
             9999999, 10000000, 99999999, 100000000, (1 << 29) - 12, (1 << 29) - 11, (1 << 29) - 10, (1 << 29) - 9]
    for e in edges:
        for w in (1, 2, 16384):
            out.append((b"chr1", e, e + w))
            out.append((b"chr1", max(e - w, 0), e))
        out.append((b"chr1", e, e))                         # empty
    for ctg in (b"chr1", b"chr2", b"chr10", b"chrUn_7", b"chr3", b"chrNone"):
        out.append((ctg, 0, 1 << 29))
        out.append((ctg, 0, 1))
        out.append((ctg, 5, 2))
    recs = [vc.interval(ln) for ln in lines]
    for k in rs.randint(0, len(recs), 120).tolist():
        c, b, e = recs[k]
        w = int(rs.choice([1, 3, 100, 20000, 3000000]))
        out.append((c, b, b + 1)); out.append((c, e - 1, e)); out.append((c, e, e + w)); out.append((c, max(b - w, 0), b + 1))
        out.append((c, max(b - w, 0), b))
    for _ in range(60):
        c = [b"chr1", b"chr2", b"chr10"][rs.randint(0, 3)]
        b = int(rs.randint(0, 120000000))
        out.append((c, b, b + int(rs.choice([1, 1000, 16384, 131072, 5000000]))))
    return out


@pytest.mark.parametrize("total", vc.COUNTS)
@pytest.mark.parametrize("block", vc.BLOCKS)
def test_the_merged_text_is_the_header_and_the_records_sorted_by_rank_pos_and_input_order(total, block, tmp_path):
    from clairvoyante_amd import vcf_merge
    files, fai, per = vc.build(tmp_path, total)
    out = str(tmp_path / "all.vcf.gz")
    vcf_merge.counts(reset=True)
    vcf_merge.merge(files, out, fai_fn=fai, block=block, threads=1 if total % 2 else 4)
    want = vc.HEADER + b"".join(vc.expected_order(per))
    assert gzip.open(out, "rb").read() == want
    c = vcf_merge.counts()
    assert c["host_calls"] == 1 and c["host_records"] == total and c["device_calls"] == 0 and c["handed_over_calls"] == 0
    # both files are what Python's gzip reads, and the data file ends with the BGZF EOF member
    raw = open(out, "rb").read()
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    assert gzip.open(out + ".tbi", "rb").read()[:4] == b"TBI\1"
    # every region of a small list through the index
    lines = vc.expected_order(per)
    for ctg, b, e in [(b"chr1", 16383, 16384), (b"chr1", 0, 1 << 29), (b"chr2", 0, 1 << 29), (b"chrUn_7", 0, 100), (b"chr3", 0, 9)]:
        assert list(vcf_merge.fetch(out, ctg, b, e)) == _brute(lines, ctg, b, e)


def test_without_a_fai_the_header_contig_lines_give_the_ranks(tmp_path):
    from clairvoyante_amd import vcf_merge
    files, _fai, per = vc.build(tmp_path, 257)
    out = str(tmp_path / "all.vcf")
    vcf_merge.merge(files, out)
    assert open(out, "rb").read() == vc.HEADER + b"".join(vc.expected_order(per)) and not os.path.exists(out + ".tbi")
    # another order of the names, another order of the file
    fai2 = str(tmp_path / "other.fai")
    open(fai2, "w").write("chr2\t9\nchr10\t9\n")
    vcf_merge.merge(files, out, fai_fn=fai2)
    assert open(out, "rb").read() == vc.HEADER + b"".join(vc.expected_order(per, [b"chr2", b"chr10"]))


def test_every_region_through_the_index_equals_a_brute_force_filter_and_seeks(merged):
    from clairvoyante_amd import vcf_merge
    out, lines, _per = merged
    idx = vcf_merge.TabixIndex.read(out + ".tbi")
    regions = _regions(lines)
    assert len(regions) > 300
    hits = 0
    for ctg, b, e in regions:
        got = list(vcf_merge.fetch(out, ctg, b, e, index=idx))
        assert got == _brute(lines, ctg, b, e), (ctg, b, e)
        hits += len(got)
    assert hits > 1000
    # the index has to actually seek: a one-window query inflates fewer members than the file holds
    members = len(vcf_merge.utils_v2.bgzf_scan(np.fromfile(out, dtype=np.uint8))[0])
    vcf_merge.counts(reset=True)
    got = list(vcf_merge.fetch(out, b"chr1", 10000000, 10000000 + 16384))
    c = vcf_merge.counts()
    assert got and c["fetch_calls"] == 1 and 0 < c["members_inflated"] < members / 4, (c, members)


def _rewrite(idx, out_fn, move):
    """the index with every chunk moved to bin move(bin), chunks per bin sorted by their begin"""
    from clairvoyante_amd import vcf_merge
    contigs = []
    for r in range(len(idx.names)):
        bins = {}
        for b, chunks in idx.bins[r].items():
            bins.setdefault(move(b), []).extend(chunks)
        meta = idx.pseudo[r]
        contigs.append((sorted((b, sorted(c)) for b, c in bins.items()), (int(meta[0][0]), int(meta[0][1]), int(meta[1][0])), idx.ioff[r]))
    vcf_merge.write_tbi(out_fn, idx.names, contigs)


def _parent(b):
    return (b - 1) >> 3 if b else 0


@pytest.mark.parametrize("variant", ["bin0", "parent"])
def test_the_reader_answers_a_coarsened_index_identically(merged, variant, tmp_path):
    """a valid index may hold its chunks in coarser bins than reg2bin chooses (htslib folds small bins into parents)"""
    from clairvoyante_amd import vcf_merge
    out, lines, _per = merged
    idx = vcf_merge.TabixIndex.read(out + ".tbi")
    coarse_fn = str(tmp_path / "coarse.tbi")
    _rewrite(idx, coarse_fn, (lambda b: 0) if variant == "bin0" else _parent)
    coarse = vcf_merge.TabixIndex.read(coarse_fn)
    assert any(set(c.keys()) != set(f.keys()) for c, f in zip(coarse.bins, idx.bins))
    for ctg, b, e in _regions(lines)[::2]:
        assert list(vcf_merge.fetch(out, ctg, b, e, index=coarse)) == _brute(lines, ctg, b, e), (ctg, b, e)


def _uncompressed_at(out):
    """virtual offset -> uncompressed offset of a BGZF file"""
    from clairvoyante_amd import utils_v2
    table, _total = utils_v2.bgzf_scan(np.fromfile(out, dtype=np.uint8))
    start = {}
    for off, _clen, at, _packed in table.tolist():
        start[off - 18] = at                                # (the members of BgzfWriter carry an 18-byte header)
    size = os.path.getsize(out)
    start[size - 28] = int(table[-1, 2] + (table[-1, 3] >> 32)) if len(table) else 0
    return lambda v: start[v >> 16] + (v & 0xffff)


def test_the_index_holds_what_the_format_says(merged):
    from clairvoyante_amd import vcf_merge
    out, lines, _per = merged
    idx = vcf_merge.TabixIndex.read(out + ".tbi")
    assert (idx.format, idx.col_seq, idx.col_beg, idx.col_end, idx.meta, idx.skip) == (2, 1, 2, 0, 35, 0)
    assert idx.names == [b"chr1", b"chr2", b"chr10", b"chrUn_7"]          # contigs with records, in output order
    at = _uncompressed_at(out)
    text = vc.HEADER + b"".join(lines)
    levels = set()
    for r, name in enumerate(idx.names):
        mine = [ln for ln in lines if ln.startswith(name + b"\t")]
        seen = 0
        for b, chunks in idx.bins[r].items():
            levels.add(sum(b >= first for first in (1, 9, 73, 585, 4681)))
            last_end = 0
            for cb, ce in chunks:
                assert cb < ce and cb >= last_end            # ascending, no overlap
                last_end = ce
                piece = text[at(cb):at(ce)]
                assert piece.endswith(b"\n") and text[at(cb) - 1:at(cb)] == b"\n"
                for ln in piece.splitlines(True):
                    c, beg, end = vc.interval(ln)
                    assert c == name and vcf_merge.reg2bin(beg, end) == b
                    seen += 1
        assert seen == len(mine)                             # every record in exactly one chunk
        meta = idx.pseudo[r]
        assert int(meta[1][0]) == len(mine) and int(meta[1][1]) == 0
        assert text[at(int(meta[0][0])):at(int(meta[0][1]))] == b"".join(mine)
        ioff = idx.ioff[r].astype(np.uint64)
        assert len(ioff) == ((max(vc.interval(ln)[2] for ln in mine) - 1) >> 14) + 1
        assert (ioff[1:] >= ioff[:-1]).all()
        # the window of the contig's first record names that record
        w = vc.interval(mine[0])[1] >> 14
        assert at(int(ioff[w])) == text.index(mine[0])
    assert len(levels) >= 3                                  # leaves, 2^17 and 2^20 bins occur (the issue's three levels)


def test_reg2bin_and_reg2bins():
    from clairvoyante_amd import vcf_merge as vm
    assert vm.reg2bin(0, 1) == 4681 and vm.reg2bin(16383, 16384) == 4681 and vm.reg2bin(16384, 16385) == 4682
    assert vm.reg2bin(16382, 16387) == 585 and vm.reg2bin(131070, 131074) == 73 and vm.reg2bin(1048574, 1048580) == 9
    assert vm.reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767 and vm.reg2bin(0, 1 << 29) == 0 and vm.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0
    rs = np.random.RandomState(3)
    for _ in range(300):
        b = int(rs.randint(0, (1 << 29) - 70000))
        e = b + int(rs.choice([1, 2, 5, 20000, 70000]))
        assert vm.reg2bin(b, e) in vm.reg2bins(b, e) and vm.reg2bin(b, e) == int(vm._reg2bin_np(np.array([b]), np.array([e]))[0])
        assert vm.reg2bin(b, e) in vm.reg2bins(max(b - 5, 0), b + 1) and vm.reg2bin(b, e) in vm.reg2bins(e - 1, e + 9)


def test_member_sizes_is_additive_and_says_what_was_written(tmp_path):
    from clairvoyante_amd import utils_v2
    data = bytes(bytearray(np.random.RandomState(1).randint(65, 70, 200000).astype(np.uint8)))
    files = []
    for threads in (1, 4):
        fn = str(tmp_path / ("t%d.gz" % threads))
        w = utils_v2.BgzfWriter(fn, block=4096, threads=threads)
        with w:
            for at in range(0, len(data), 1777):
                w.write(data[at:at + 1777])
        raw = open(fn, "rb").read()
        assert len(w.member_sizes) == -(-len(data) // 4096) and sum(w.member_sizes) + 28 == len(raw)
        at = 0
        for s in w.member_sizes:
            assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and struct.unpack_from("<H", raw, at + 16)[0] + 1 == s
            at += s
        files.append(raw)
    assert files[0] == files[1] and gzip.decompress(files[0]) == data


def test_errors_and_END(tmp_path):
    from clairvoyante_amd import vcf_merge
    files, fai, per = vc.build(tmp_path, 65)
    out = str(tmp_path / "o.vcf.gz")
    # a header that differs byte for byte
    vc.write_file(files[3], vc.HEADER.replace(b"SAMPLE", b"OTHER") + b"".join(per[3]), "plain")
    with pytest.raises(ValueError, match="chr1_10000000_20000000"):
        vcf_merge.merge(files, out, fai_fn=fai)
    # a position past 2^29
    vc.write_file(files[3], vc.HEADER + b"".join(per[3]) + vc.rec("chr1", (1 << 29), "AC", "A"), "plain")
    with pytest.raises(ValueError, match="2\\^29"):
        vcf_merge.merge(files, out, fai_fn=fai)
    # fewer than 8 columns
    vc.write_file(files[3], vc.HEADER + b"chr1\t5\t.\tA\tC\t3\t.\n", "plain")
    with pytest.raises(ValueError, match="8 columns"):
        vcf_merge.merge(files, out, fai_fn=fai)
    # END= widens the record: a query that overlaps only its tail finds it
    wide = vc.rec("chr1", 15000000, "A", "<DEL>", info="SVTYPE=DEL;END=15100000")
    short = vc.rec("chr1", 15000500, "A", "C", info="END=7")          # (an END in front of the record does not count)
    vc.write_file(files[3], vc.HEADER + b"".join(per[3]) + wide + short, "plain")
    vcf_merge.merge(files, out, fai_fn=fai, block=512)
    assert list(vcf_merge.fetch(out, "chr1", 15099990, 15099999)) == [wide]
    assert list(vcf_merge.fetch(out, "chr1", 15100000, 15100001)) == []
    assert list(vcf_merge.fetch(out, "chr1", 15000400, 15000500)) == [wide, short]
    # a last line without newline gets one
    vc.write_file(files[3], vc.HEADER + b"".join(per[3])[:-1], "plain")
    vcf_merge.merge(files, out, fai_fn=fai)
    assert gzip.open(out, "rb").read() == vc.HEADER + b"".join(vc.expected_order(per))


def test_the_switch_takes_host_or_device_and_nothing_else(monkeypatch):
    import torch
    from clairvoyante_amd import vcf_merge
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for v in ("", "host", "device"):                         # no GPU: the host loop whatever the switch says
        monkeypatch.setenv("CV_VCF_MERGE", v)
        assert vcf_merge.route() == "host"
    for v in ("gpu", "Device", "1"):
        monkeypatch.setenv("CV_VCF_MERGE", v)
        with pytest.raises(ValueError):
            vcf_merge.route()


def test_MergeVcf_over_a_glob_and_in_the_submodule_list(tmp_path):
    from clairvoyante_amd import __main__ as entry
    assert "MergeVcf" in entry.SUBMODULES
    files, fai, per = vc.build(tmp_path, 257, form="bgzf")
    out = str(tmp_path / "hg.vcf.gz")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    env.pop("CV_VCF_MERGE", None)
    subprocess.check_call([sys.executable, "-m", "clairvoyante_amd", "MergeVcf", "--vcf_glob", str(tmp_path / "p.chr*.vcf.gz"),
                           "--ref_fn", fai[:-4], "--out_fn", out, "--block", "4096", "--threads", "2"], env=env)
    assert gzip.open(out, "rb").read() == vc.HEADER + b"".join(vc.expected_order(per)) and os.path.isfile(out + ".tbi")


def test_callVarBamParallel_merges_the_chunk_files_that_exist(tmp_path):
    """--run itself needs a GPU (test_gpu_pileup.py); here the step behind it, over the chunk naming of chunks()"""
    from clairvoyante_amd import callVarBamParallel as par
    assert par.build_parser().parse_args([]).merged_fn is None
    _files, fai, per = vc.build(tmp_path, 0)
    prefix = str(tmp_path / "run")
    todo = [("chr10", 0, 10000000), ("chr1", 0, 10000000), ("chr1", 100000000, 110000000), ("chr1", 10000000, 20000000),
            ("chr2", 0, 10000000), ("chr2", 10000000, 20000000)]
    todo = [(c, s, e, "%s.%s_%d_%d.vcf" % (prefix, c, s, e)) for c, s, e in todo]
    per = vc.records(257)
    for k, (t, lines) in enumerate(zip(todo, per)):
        if k != vc.EMPTY_FILE:                               # a chunk without candidates wrote no file
            vc.write_file(t[3], vc.HEADER + b"".join(lines), "plain")
    args = types.SimpleNamespace(merged_fn=str(tmp_path / "run.vcf.gz"), ref_fn=fai[:-4])
    got = par.merge_chunks(args, todo, 0, 1)
    assert got["records"] == 257 and got["files"] == 5
    assert gzip.open(args.merged_fn, "rb").read() == vc.HEADER + b"".join(vc.expected_order(per))
    assert par.merge_chunks(args, todo, 1, 1) is None       # only rank 0 merges


def test_GetTruth_reads_a_region_through_the_tbi_when_tabix_is_absent(tmp_path, monkeypatch, capfdbinary):
    from clairvoyante_amd import GetTruth, vcf_merge
    files, fai, per = vc.build(tmp_path, 2000)
    out = str(tmp_path / "truth.vcf.gz")
    vcf_merge.merge(files, out, fai_fn=fai, block=4096)
    empty = tmp_path / "bin"
    empty.mkdir()
    for tool in ("gzip", "which", "sh"):                     # a PATH with the tools GetTruth pipes through, and no tabix
        import shutil
        os.symlink(shutil.which(tool), str(empty / tool))
    monkeypatch.setenv("PATH", str(empty))
    rows = {}
    for with_index in (True, False):
        if not with_index:
            os.remove(out + ".tbi")
        vcf_merge.counts(reset=True)
        var = str(tmp_path / ("rows_%d" % with_index))
        GetTruth.OutputVariant(types.SimpleNamespace(vcf_fn=out, var_fn=var, ctgName="chr1", ctgStart=10000000, ctgEnd=10030000))
        rows[with_index] = gzip.open(var, "rb").read()
        c = vcf_merge.counts()
        assert c["fetch_calls"] == (1 if with_index else 0)
        if with_index:
            assert 0 < c["members_inflated"] < 20
    assert rows[True] == rows[False] and rows[True].count(b"\n") > 50
