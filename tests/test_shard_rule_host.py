"""One tensor file under several ranks, without a GPU: the ownership rule (utils_v2.shard_span: which rank owns which
line), the ranged readers GetTensor / GetTensorDevice with part=(rank, ws) over plain text and BGZF -- the device side
replaced by the stand-ins of tests/test_text_parse_device_host.py and tests/test_bgzf_host.py --, callVar.shard_route,
and two ranks over gloo.  The ranks' batches one behind the other must be GetTensor's over the whole file."""
import itertools
import os
import sys

import numpy as np
import pytest

import bgzf_cases as B
import shard_cases as S
import textparse_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ---------------------------------------------------------------------------------------------------------
def _rule_text(final_newline):
    """~300 bytes: lines of 0, 1, 2 and 50 bytes, a run of blank lines, blank lines at both ends"""
    lines = [b"", b"a", b"bc", b"d" * 50, b"", b"", b"", b"", b"e", b"f" * 50, b"gh", b"", b"i" * 50, b"j", b"k" * 50,
             b"lm", b"n" * 50, b"", b"o", b"pq"]
    text = b"\n".join(lines) + (b"\n" if final_newline else b"")
    assert 280 <= len(text) <= 320 and text.endswith(b"\n") == final_newline
    return text


def _owned_lines(text):
    """the lines of a piece of text as (bytes with their newline) -- a piece that ends without newline ends the text"""
    return text.splitlines(True)


def _check_vector(utils_v2, text, want, cuts):
    got = []
    for r in range(len(cuts) - 1):
        got += _owned_lines(utils_v2.shard_text(text, cuts, r))
    assert got == want, cuts


@pytest.mark.parametrize("final_newline", [True, False])
def test_every_line_has_exactly_one_owner(final_newline):
    """For every ws in 1..8 and every vector of cuts among a dense set, the lines of ranks 0..ws-1 one behind the other
    are the text's lines, each once.  What rank r owns depends on B[r] and B[r+1] alone, so every offset 0..n is tried
    in every position for ws <= 3 (all pairs of neighbours); for ws 4..8 the vectors run over eleven offsets that hold
    every kind of place a cut can fall on: 0, the first line's newline, a line start, the bytes around it, the middle of
    a long line, inside the run of blank lines, n - 1 and n."""
    from clairvoyante_amd import utils_v2
    text = _rule_text(final_newline)
    n = len(text)
    want = _owned_lines(text)
    assert len(want) == 20 and b"".join(want) == text
    for ws in (1, 2, 3):
        for inner in itertools.combinations_with_replacement(range(n + 1), ws - 1):
            _check_vector(utils_v2, text, want, [0] + list(inner) + [n])
    start = text.index(b"f" * 50)                       # a line start in the middle
    blank = text.index(b"\n\n\n\n")
    dense = sorted({0, 1, start - 1, start, start + 1, start + 25, blank + 1, blank + 2, n - 2, n - 1, n})
    assert len(dense) == 11
    for ws in range(4, 9):
        for inner in itertools.combinations_with_replacement(dense, ws - 1):
            _check_vector(utils_v2, text, want, [0] + list(inner) + [n])


def test_the_rule_in_words():
    from clairvoyante_amd import utils_v2
    text = b"ab\ncd\nef"
    own = lambda cuts: [utils_v2.shard_text(text, cuts, r) for r in range(len(cuts) - 1)]
    assert own([0, 3, 8]) == [b"ab\n", b"cd\nef"]                   # a line that starts exactly at B[r] belongs to rank r
    assert own([0, 4, 8]) == [b"ab\ncd\n", b"ef"]                   # one byte later it belongs to the rank before
    assert own([0, 4, 5, 8]) == [b"ab\ncd\n", b"", b"ef"]           # a range without a line start owns nothing
    assert own([0, 7, 8]) == [b"ab\ncd\nef", b""]                   # the last line, without newline: who holds its first byte
    assert own([0, 6, 8]) == [b"ab\ncd\n", b"ef"]
    assert own([0, 0, 8]) == [b"ab\n", b"cd\nef"] and own([0, 8, 8]) == [text, b""]
    assert utils_v2.shard_text(b"", [0, 0, 0], 1) == b"" and utils_v2.shard_cuts(10, 4) == [0, 2, 5, 7, 10]


def test_bgzf_cuts_come_from_the_member_table():
    from clairvoyante_amd import utils_v2
    data = B.bgzf_file(T.volume_text(2000)[:30000], block=5000)
    table, total = utils_v2.bgzf_scan(np.frombuffer(data, dtype=np.uint8))
    assert total == 30000 and len(table) == 7
    for ws in (1, 2, 3, 5):
        cuts = utils_v2.bgzf_shard_cuts(table, total, len(data), ws)
        assert cuts[0] == 0 and cuts[-1] == total and cuts == sorted(cuts)
        for r in range(1, ws):
            first = min(i for i in range(len(table)) if table[i, 0] >= len(data) * r // ws)
            assert cuts[r] == table[first, 2] and cuts[r] % 5000 == 0


# ---- the ranged readers -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("shard")
    text = T.volume_text(2000)
    few = b"".join(text.splitlines(True)[:3])
    out = {"text": text, "few": few}

    def put(name, data):
        out[name] = str(d / name)
        open(out[name], "wb").write(data)
    put("volume.txt", text)
    put("volume_nonl.txt", text[:-1])
    put("few.txt", few)
    for block in (65280, 5000, 700):
        put("volume_%d.gz" % block, B.bgzf_file(text, block=block))
    put("volume_nonl_5000.gz", B.bgzf_file(text[:-1], block=5000))
    put("empties_5000.gz", S.bgzf_with_empty_members(text, 5000))
    put("empties_700.gz", S.bgzf_with_empty_members(text[:400000], 700))
    put("few_700.gz", B.bgzf_file(few, block=700))
    put("only_eof.gz", B.bgzf_file(b""))
    return out


@pytest.fixture(scope="module")
def whole(files):
    """GetTensor over the whole file, once per file: what the ranks' batches must add up to (read only)"""
    from clairvoyante_amd import utils_v2
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = T.collect(utils_v2.GetTensor(files[name], 300, log=False))
        return memo[name]
    return get


def _same_as_whole(files, whole, name, ws, reader):
    want = whole(name)
    x, pos, flags, sizes = S.parts_concatenated(reader, ws)
    assert np.array_equal(x, want[0])
    assert pos == want[1]
    for f in flags:
        assert f[-1] == 1 and not any(f[:-1])
    return sizes, flags


WAYS = [1, 2, 3, 4, 7]
PLAIN = ["volume.txt", "volume_nonl.txt", "few.txt"]
BGZF = ["volume_65280.gz", "volume_5000.gz", "volume_700.gz", "volume_nonl_5000.gz", "empties_5000.gz", "empties_700.gz",
        "few_700.gz", "only_eof.gz"]


@pytest.mark.parametrize("ws", WAYS)
@pytest.mark.parametrize("name", PLAIN + BGZF)
def test_ranged_host_reader(files, whole, name, ws):
    from clairvoyante_amd import utils_v2
    sizes, flags = _same_as_whole(files, whole, name, ws,
                                  lambda r: utils_v2.GetTensor(files[name], 300, log=False, part=(r, ws)))
    if name.startswith("few") and ws == 7:
        assert sum(1 for c in sizes if c == 0) >= 4 and sum(sizes) == 3        # three lines: four ranks own nothing


@pytest.mark.parametrize("slab", [None, 4096])
@pytest.mark.parametrize("ws", WAYS)
@pytest.mark.parametrize("name", PLAIN)
def test_ranged_device_reader_plain_text(files, whole, name, ws, slab, monkeypatch):
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_TextSlabDevice", T.AllHostDevice)
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    _same_as_whole(files, whole, name, ws, lambda r: utils_v2.GetTensorDevice(files[name], 300, "cpu", log=False, part=(r, ws)))


@pytest.mark.parametrize("slab", [None, 4096])
@pytest.mark.parametrize("ws", WAYS)
@pytest.mark.parametrize("name", BGZF)
def test_ranged_device_reader_bgzf(files, whole, name, ws, slab, monkeypatch):
    """block = 700 is a third of a line: a line spans three or more members, the cuts fall inside lines, and of the
    three-line file most of seven ranks own nothing; the files with empty members have one at every cut"""
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_TextSlabDevice", S.RangedZlibDevice)
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    sizes, flags = _same_as_whole(files, whole, name, ws,
                                  lambda r: utils_v2.GetTensorDevice(files[name], 300, "cpu", log=False, part=(r, ws)))
    if name == "few_700.gz" and ws == 7:
        assert sum(1 for c in sizes if c == 0) >= 4 and sum(sizes) == 3


def test_the_member_a_cut_names_is_an_empty_one(files):
    """what the files with empty members are for: at every inner cut of 2, 3 and 4 ranks the first member at or above
    the cut's file offset is empty"""
    from clairvoyante_amd import utils_v2
    for name in ("empties_5000.gz", "empties_700.gz"):
        data = np.fromfile(files[name], dtype=np.uint8)
        table, _total = utils_v2.bgzf_scan(data)
        hits = 0
        for ws in (2, 3, 4):
            for r in range(1, ws):
                i = int(np.searchsorted(table[:, 0], len(data) * r // ws, side="left"))
                hits += int(table[i, 3] >> 32 == 0)
        assert hits >= 5, name


def test_a_range_of_what_is_no_plain_or_bgzf_file_is_an_error(files, tmp_path, monkeypatch):
    import gzip
    from clairvoyante_amd import utils_v2
    fn = str(tmp_path / "t.gz")
    with gzip.open(fn, "wb") as fh:
        fh.write(files["few"])
    with pytest.raises(ValueError, match="plain-text or BGZF"):
        list(utils_v2.GetTensor(fn, 10, log=False, part=(0, 2)))
    with pytest.raises(ValueError, match="plain-text or BGZF"):
        list(utils_v2.GetTensor("PIPE", 10, log=False, part=(0, 2)))
    monkeypatch.setenv("CV_TEXT", "stream")
    with pytest.raises(ValueError, match="plain-text or BGZF"):
        list(utils_v2.GetTensor(files["few.txt"], 10, log=False, part=(0, 2)))


# ---- the route ------------------------------------------------------------------------------------------------------------
def test_shard_route_follows_the_input(files, tmp_path, monkeypatch):
    import gzip
    from clairvoyante_amd import callVar
    gz = str(tmp_path / "t.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(files["few"])
    plain, bgzf = files["volume.txt"], files["volume_5000.gz"]
    monkeypatch.delenv("CV_SHARD", raising=False)
    monkeypatch.delenv("CV_TEXT", raising=False)
    # unset: a form takes the range route only where the measurement made it the default, and from a SHARE of its floor upwards
    for form, fn, floor_name in (("text", plain, "TEXT_DEVICE_MIN_BYTES"), ("bgzf", bgzf, "BGZF_DEVICE_MIN_BYTES")):
        size = os.path.getsize(fn)
        monkeypatch.setattr(callVar, "SHARD_RANGE_DEFAULT", {"text": False, "bgzf": False})
        monkeypatch.setattr(callVar, floor_name, (1, None) if form == "text" else 1)
        assert callVar.shard_route(fn, 2) == "lines"
        monkeypatch.setattr(callVar, "SHARD_RANGE_DEFAULT", {"text": form == "text", "bgzf": form == "bgzf"})
        assert callVar.shard_route(fn, 2) == "range"
        share = size // 4
        monkeypatch.setattr(callVar, floor_name, (share, None) if form == "text" else share)
        assert callVar.shard_route(fn, 4) == "range" and callVar.shard_route(fn, 5) == "lines"
        monkeypatch.setattr(callVar, floor_name, (None, None) if form == "text" else None)
        assert callVar.shard_route(fn, 2) == "lines"
    monkeypatch.setattr(callVar, "SHARD_RANGE_DEFAULT", {"text": True, "bgzf": True})
    monkeypatch.setattr(callVar, "TEXT_DEVICE_MIN_BYTES", (1, 1))
    monkeypatch.setattr(callVar, "BGZF_DEVICE_MIN_BYTES", 1)
    assert callVar.shard_route(plain, 2) == callVar.shard_route(bgzf, 2) == "range"
    for other in (gz, "PIPE", plain + "," + bgzf, str(tmp_path / "missing.txt")):
        assert callVar.shard_route(other, 2) == "lines"
    monkeypatch.setenv("CV_SHARD", "lines")
    assert callVar.shard_route(plain, 2) == "lines"
    monkeypatch.setenv("CV_SHARD", "range")
    monkeypatch.setattr(callVar, "SHARD_RANGE_DEFAULT", {"text": False, "bgzf": False})
    assert callVar.shard_route(plain, 2) == callVar.shard_route(bgzf, 2) == "range"
    for other in (gz, "PIPE", plain + "," + bgzf):
        with pytest.raises(ValueError, match="CV_SHARD=range needs"):
            callVar.shard_route(other, 2)
    monkeypatch.setenv("CV_SHARD", "bogus")
    with pytest.raises(ValueError, match="CV_SHARD must be"):
        callVar.shard_route(plain, 2)
    assert set(callVar.shard_counts()) == {"lines", "range"}


def test_the_shipped_defaults_keep_small_inputs_on_the_lines_route(files, monkeypatch):
    """nothing an existing test reads changes its route: with CV_SHARD unset a file below the floors splits by lines"""
    from clairvoyante_amd import callVar
    monkeypatch.delenv("CV_SHARD", raising=False)
    for name in ("volume.txt", "volume_65280.gz", "few.txt"):
        assert callVar.shard_route(files[name], 2) == "lines"


# ---- two ranks over gloo: the range route of callVar.TestSharded with the oracle in the model's place ------------------------
def _range_worker(rank, ws, port, tmp, tfn):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws),
                      LOCAL_RANK=str(rank), OMP_NUM_THREADS="1", CV_SHARD="range", CV_TEXT_PARSE="host")
    torch.set_num_threads(1)
    import io
    import types
    from clairvoyante_amd import callVar, parallel, utils_v2
    utils_v2._pinned.enabled = False           # (pageable row buffers: the page-locked ones would open the GPU of a GPU box)
    from oracle import cv_oracle as O
    import common
    parallel.init_from_env(backend="gloo")
    P = common.bench_params(O, "slim")
    args = types.SimpleNamespace(v2=False, v3=True, showRef=False, qual=30, ref_fn=None, sampleName="S")
    call_fn = os.path.join(tmp, "calls.vcf")
    assert callVar.shard_route(tfn, ws) == "range"
    nbytes = 0
    with open("%s.rank%d" % (call_fn, rank), "w") as frag:
        for _end, c, X, pos in callVar.range_batches(utils_v2, tfn, rank, ws, "cpu", batch=37):
            buf = io.StringIO()
            if c:
                o = O.predict("slim", P, np.asarray(X))
                callVar.Output(args, buf, c, X, pos, o[:, 0:4], o[:, 4:6], o[:, 6:10], o[:, 10:16])
            frag.write(buf.getvalue())
            nbytes += len(buf.getvalue().encode("ascii"))
    with open("%s.rank%d.idx" % (call_fn, rank), "w") as f:          # ONE entry per rank, also for a rank that owns nothing
        f.write("%d %d\n" % (rank, nbytes))
    dist.all_reduce(torch.zeros(1))
    if rank == 0:
        with open(call_fn, "w") as fh:
            callVar.PrintVCFHeader(args, fh)
            callVar.merge_fragments(call_fn, ws, fh)
    dist.all_reduce(torch.zeros(1))
    dist.destroy_process_group()


@pytest.mark.parametrize("ws,n,form", [(2, 130, "text"), (2, 130, "bgzf"), (3, 2, "bgzf")])
def test_range_route_over_gloo_equals_one_process(oracle, tmp_path, ws, n, form):
    """every rank reads its range of the one file with the ranged host reader and writes ONE index entry; rank 0 joins the
    fragments with merge_fragments as it is: the VCF of one process, byte for byte ((3, 2): a rank that owns nothing)"""
    import io
    import types
    import torch.multiprocessing as mp
    import common
    from clairvoyante_amd import callVar, utils_v2
    text = S.tensor_text(common.inputs(n, seed=23))
    tfn = str(tmp_path / ("t.txt" if form == "text" else "t.gz"))
    open(tfn, "wb").write(text if form == "text" else B.bgzf_file(text, block=3000))
    port = 29950 + (os.getpid() + n + 17 * ws + len(form)) % 40
    mp.spawn(_range_worker, args=(ws, port, str(tmp_path), tfn), nprocs=ws, join=True)
    got = open(str(tmp_path / "calls.vcf")).read()
    args = types.SimpleNamespace(v2=False, v3=True, showRef=False, qual=30, ref_fn=None, sampleName="S")
    P = common.bench_params(oracle, "slim")
    fh = io.StringIO()
    callVar.PrintVCFHeader(args, fh)
    for _end, c, X, pos in utils_v2.GetTensor(tfn, 100, log=False):
        if c:
            o = oracle.predict("slim", P, X)
            callVar.Output(args, fh, c, X, pos, o[:, 0:4], o[:, 4:6], o[:, 6:10], o[:, 10:16])
    assert got == fh.getvalue()
    assert got.count("\n") > 10 or n < 20
    assert not [f for f in os.listdir(str(tmp_path)) if ".rank" in f]
