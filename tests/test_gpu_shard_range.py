"""One tensor file read by several ranks, each its own byte range, on the GPU: cv_text_find_newline_dev against
bytes.find, utils_v2.GetTensorDevice(part=(rank, ws)) against GetTensor over the whole file (bit for bit), how many BGZF
members the ranks inflate between them, a member the device hands to the host at a cut, and callVar's `range` route from
the command line against the single-process VCF (byte for byte)."""
import ctypes
import os
import subprocess
import sys
import time
import types
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import common
import shard_cases as S
import textparse_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = -0x0123456789ABCDEF
FRONT = 48                              # bytes in front of the text: newlines, which a kernel that masks wrongly would find


# ---- cv_text_find_newline_dev ---------------------------------------------------------------------------------------------
def _find(text, offset, queries):
    """`text` at `offset` bytes behind a 16-byte boundary, newlines in front of and behind it; -> (answers, the buffer
    around the answers intact, the buffer around the text intact)"""
    import torch
    from clairvoyante_amd import _lib
    n, k = len(text), len(queries)
    buf = np.full(FRONT + offset + n + 64, 10, dtype=np.uint8)
    buf[FRONT + offset:FRONT + offset + n] = np.frombuffer(text, dtype=np.uint8)
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    out = torch.full((8 + 64 + 8,), CANARY, dtype=torch.int64, device="cuda")
    q = (ctypes.c_int64 * max(k, 1))(*queries)
    torch.cuda.synchronize()
    _lib.check(_lib.load().cv_text_find_newline_dev(ctypes.c_void_p(dev.data_ptr() + FRONT + offset), n, q, k,
                                                    ctypes.c_void_p(out.data_ptr() + 64),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[8:8 + k], bool(np.all(o[:8] == CANARY) and np.all(o[8 + k:] == CANARY)), np.array_equal(dev.cpu().numpy(), buf)


def _want(text, queries):
    out = []
    for f in queries:
        j = text.find(b"\n", max(f, 0)) if f < len(text) else -1
        out.append(len(text) if j < 0 else j)
    return out


def _texts(n):
    """texts of n bytes: a newline at the first byte, at the last byte, at both, nowhere, and (when there is room) some
    in the middle"""
    base = bytes(97 + i % 23 for i in range(n))
    out = [b"\n" + base[1:], base[:-1] + b"\n", b"\n" + base[1:-1] + b"\n" if n > 1 else b"\n", base]
    if n > 40:
        b = bytearray(base)
        for at in (7, 15, 16, 17, n // 2, n // 2 + 1, n - 9):
            b[at] = 10
        out.append(bytes(b))
    return [t for t in out if len(t) == n]


@pytest.mark.parametrize("offset", [0, 5, 15])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
def test_find_newline_against_bytes_find(n, offset):
    for text in _texts(n):
        queries = [0, n - 1, n, n + 3] + [j + 1 for j in range(n) if text[j] == 10]
        queries += [(7 * i) % (n + 2) for i in range(64 - len(queries))]          # 64 queries at once
        queries = queries[:64]
        got, out_intact, text_intact = _find(text, offset, queries)
        assert list(got) == _want(text, queries), (n, offset, text[:20])
        assert out_intact and text_intact
    got, out_intact, _t = _find(_texts(n)[0], offset, [0])                        # one query: the 63 slots behind it stay
    assert list(got) == [0] and out_intact


def test_find_newline_over_more_text_than_the_grid_covers_in_one_step():
    """5 MiB + 5 bytes (the grid steps over 4 MiB at a time), sparse newlines, queries in every part of it -- some behind
    the last newline, some far behind an answer that other waves have long found"""
    rng = np.random.RandomState(3)
    n = (5 << 20) + 5
    a = rng.randint(32, 127, n).astype(np.uint8)
    nl = np.sort(rng.choice(n - 70000, 40, replace=False))
    a[nl] = 10
    text = a.tobytes()
    queries = [0, int(nl[0]), int(nl[0]) + 1, int(nl[-1]), int(nl[-1]) + 1, n - 1, n, n + 3, -4, 4 << 20, (4 << 20) + 4096]
    queries += [int(v) for v in rng.randint(0, n, 64 - len(queries))]
    got, out_intact, text_intact = _find(text, 5, queries)
    assert list(got) == _want(text, queries) and out_intact and text_intact
    assert sum(1 for g in got if g == n) >= 3


def test_find_newline_checks_its_arguments():
    import torch
    from clairvoyante_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, q = ctypes.c_void_p(buf.data_ptr()), (ctypes.c_int64 * 65)()
    assert lib.cv_text_find_newline_dev(p, 10, q, 65, p, None) != 0 and "queries" in lib.cv_last_error().decode()
    assert lib.cv_text_find_newline_dev(p, -1, q, 1, p, None) != 0
    assert lib.cv_text_find_newline_dev(None, 10, q, 1, p, None) != 0 and "null" in lib.cv_last_error().decode()
    assert lib.cv_text_find_newline_dev(p, 10, q, 1, ctypes.c_void_p(buf.data_ptr() + 4), None) != 0
    assert lib.cv_text_find_newline_dev(None, 0, None, 0, None, None) == 0           # no query: nothing to do
    assert lib.cv_text_find_newline_dev(None, 0, q, 2, p, None) == 0                 # no text: every answer is len = 0
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0


# ---- the ranged reader -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("shard_gpu")
    text = T.volume_text(2000)
    short = text[:400000]                                   # for the runs with 4 KiB slabs
    short = short[:short.rindex(b"\n") + 1]
    off = T.off_format_text()[0]
    out = {}

    def put(name, data):
        out[name] = str(d / name)
        open(out[name], "wb").write(data)
    for tag, body in (("volume", text), ("short", short)):
        put(tag + ".txt", body)
        put(tag + "_nonl.txt", body[:-1])
        for block in (65280, 5000, 700):
            put("%s_%d.gz" % (tag, block), B.bgzf_file(body, block=block, level=1))
        put(tag + "_nonl_5000.gz", B.bgzf_file(body[:-1], block=5000, level=1))
    put("short_empties_5000.gz", S.bgzf_with_empty_members(short, 5000))
    put("volume_empties_5000.gz", S.bgzf_with_empty_members(text, 5000))
    put("off_format.txt", off)
    put("off_format_3000.gz", B.bgzf_file(off, block=3000))
    return out


@pytest.fixture(scope="module")
def whole(files):
    """GetTensor over the whole file, once per file (read only)"""
    from clairvoyante_amd import utils_v2
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = T.collect(utils_v2.GetTensor(files[name], 300, log=False))
        return memo[name]
    return get


def _parts_equal_whole(files, whole, name, ws):
    from clairvoyante_amd import utils_v2
    want = whole(name)
    x, pos, flags, sizes = S.parts_concatenated(
        lambda r: utils_v2.GetTensorDevice(files[name], 300, "cuda", log=False, part=(r, ws)), ws)
    assert np.array_equal(x, want[0]), (name, ws)
    assert pos == want[1], (name, ws)
    for f in flags:
        assert f[-1] == 1 and not any(f[:-1])
    return sizes


FORMS = [".txt", "_nonl.txt", "_65280.gz", "_5000.gz", "_700.gz", "_nonl_5000.gz", "_empties_5000.gz"]


@pytest.mark.parametrize("form", FORMS + ["off_format.txt", "off_format_3000.gz"])
@pytest.mark.parametrize("slab", [None, 4096])
def test_ranged_device_reader_gives_the_whole_file(files, whole, form, slab, monkeypatch):
    """all parts of 1, 2, 3 and 4 ranks, one after the other in this process; with 4 KiB slabs over the first 400 KB"""
    if slab is None:
        monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    else:
        monkeypatch.setenv("CV_TEXT_SLAB_BYTES", str(slab))
    name = form if form.startswith("off_format") else ("volume" if slab is None else "short") + form
    for ws in (1, 2, 3, 4):
        sizes = _parts_equal_whole(files, whole, name, ws)
        assert sum(sizes) > 50 and (form.startswith("off_format") or min(sizes) > 0)


def test_ranks_inflate_the_file_once_and_two_members_per_cut(files, whole, monkeypatch):
    """65 280-byte members, lines shorter than a member, no empty member but the EOF marker: rank r inflates the members
    of its range, the one in front (which holds byte B[r] - 1) and at most one behind (which holds the end of its last
    line) -- M + 2 (ws - 1) between them at the most, by the rule; none goes to the host"""
    from clairvoyante_amd import utils_v2
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    M = sum(1 for m in B.walk(open(files["volume_65280.gz"], "rb").read()) if m[2])
    assert M > 60
    for ws in (1, 2, 3, 4):
        before = dict(utils_v2.bgzf_member_counts)
        _parts_equal_whole(files, whole, "volume_65280.gz", ws)
        grew = {k: utils_v2.bgzf_member_counts[k] - before[k] for k in before}
        print("ws %d: %d members inflated on the device, %d on the host (the file has %d)" % (ws, grew["device"], grew["host"], M))
        assert grew["host"] == 0 and M <= grew["device"] <= M + 2 * (ws - 1)


def test_a_member_the_device_hands_to_the_host_at_a_cut(files, whole, tmp_path, monkeypatch):
    """the member in front of the cut of two ranks, the one at it and the one behind it carry a byte behind their DEFLATE
    data: the device does not vouch for such a member (its stream must end where the data ends), the host takes it.  The
    rows are the file's, and only those three members go to the host"""
    from clairvoyante_amd import utils_v2
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    text = T.volume_text(2000)
    data = open(files["volume_65280.gz"], "rb").read()
    table, _total = utils_v2.bgzf_scan(np.frombuffer(data, dtype=np.uint8))
    at = int(np.searchsorted(table[:, 0], len(data) // 2, side="left"))
    damaged = (at - 1, at, at + 1)
    members = []
    for i, start in enumerate(range(0, len(text), 65280)):
        piece = text[start:start + 65280]
        members.append(B.bgzf_member(B.deflate(piece, 1) + (b"\0" if i in damaged else b""), len(piece), zlib.crc32(piece)))
    fn = str(tmp_path / "damaged.gz")
    open(fn, "wb").write(b"".join(members) + B.bgzf_member(B.deflate(b""), 0, 0))
    table2, _total = utils_v2.bgzf_scan(np.fromfile(fn, dtype=np.uint8))
    assert int(np.searchsorted(table2[:, 0], os.path.getsize(fn) // 2, side="left")) == at        # the cut did not move
    marks = {int(table2[i, 3]) for i in damaged}
    taken = []
    inflate = utils_v2._BgzfSlab.inflate_member
    monkeypatch.setattr(utils_v2._BgzfSlab, "inflate_member", lambda self, i: (taken.append(int(self.table[i, 3])), inflate(self, i))[1])
    files = dict(files, damaged=fn)
    # two ranks: rank 1 also reads the member in front of its range, rank 0 the one behind unless its last line ends with its range
    for ws, count in ((1, 3), (2, 4 + (text[at * 65280 - 1:at * 65280] != b"\n"))):
        del taken[:]
        before = dict(utils_v2.bgzf_member_counts)
        x, pos, _flags, _sizes = S.parts_concatenated(
            lambda r: utils_v2.GetTensorDevice(fn, 300, "cuda", log=False, part=(r, ws)), ws)
        want = whole("volume_65280.gz")
        assert np.array_equal(x, want[0]) and pos == want[1]
        assert set(taken) == marks and len(taken) == count
        assert utils_v2.bgzf_member_counts["host"] - before["host"] == count


# ---- the command line ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(oracle, tmp_path_factory):
    from clairvoyante_amd import clairvoyante_v3, utils_v2
    d = tmp_path_factory.mktemp("shard_cli")
    m = clairvoyante_v3.Clairvoyante(); m.setParameters(common.bench_params(oracle, "full"))
    out = {"dir": str(d), "model": str(d / "model"), "plain": str(d / "t.txt"), "bgzf": str(d / "t.bgzf.gz")}
    m.saveParameters(out["model"]); m.close()
    text = S.tensor_text(common.inputs(3000, seed=17))
    open(out["plain"], "wb").write(text)
    with utils_v2.BgzfWriter(out["bgzf"]) as w:
        w.write(text)
    return out


def _single(cli, form, show_ref, monkeypatch):
    """the VCF of one process, in this process"""
    from clairvoyante_amd import callVar
    monkeypatch.delenv("CV_SHARD", raising=False)
    monkeypatch.delenv("CV_VCF_FORMAT", raising=False)
    monkeypatch.delenv("CV_TEXT_SLAB_BYTES", raising=False)
    monkeypatch.setenv("CV_TEXT_PARSE", "host")
    out = os.path.join(cli["dir"], "one_%s_%d.vcf" % (form, show_ref))
    a = types.SimpleNamespace(tensor_fn=cli[form], chkpnt_fn=cli["model"], call_fn=out, qual=30, sampleName="S", ref_fn=None,
                              threads=None, showRef=show_ref, v3=True, v2=False, slim=False)
    callVar.Run(a)
    return open(out, "rb").read()


def _ranks(cli, form, ws, call_fn, extra_args=(), limit=120, **env_more):
    """`ws` callVar processes on the one GPU (gloo); every child has `limit` seconds; when one exits non-zero the others
    are terminated; -> exit codes"""
    base = [sys.executable, "-m", "clairvoyante_amd.callVar", "--chkpnt_fn", cli["model"], "--tensor_fn", cli[form],
            "--sampleName", "S", "--qual", "30", "--call_fn", call_fn] + list(extra_args)
    port = 29100 + (os.getpid() + 7 * ws + len(call_fn)) % 150
    env = dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE=str(ws), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
               CV_DIST_BACKEND="gloo", CV_TEXT_PARSE="device")
    env.update(env_more)
    procs = [subprocess.Popen(base, env=dict(env, RANK=str(r)), cwd=ROOT) for r in range(ws)]
    deadline = time.time() + limit
    codes = [None] * ws
    try:
        while any(c is None for c in codes):
            for i, p in enumerate(procs):
                if codes[i] is None:
                    try:
                        codes[i] = p.wait(timeout=0.05)
                    except subprocess.TimeoutExpired:
                        pass
            if any(c not in (None, 0) for c in codes) or time.time() > deadline:
                break
    finally:
        for i, p in enumerate(procs):
            if codes[i] is None:
                p.terminate()
        for i, p in enumerate(procs):
            if codes[i] is None:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill(); p.wait()
                codes[i] = "ended"
    return codes


@pytest.mark.parametrize("form,ws,show_ref", [("bgzf", 2, False), ("plain", 3, True)])
def test_range_route_from_the_command_line_writes_the_single_process_vcf(cli, form, ws, show_ref, monkeypatch):
    """3000 rows, CV_SHARD=range, the device reader; the run with --showRef also writes its records on the device"""
    want = _single(cli, form, show_ref, monkeypatch)
    call_fn = os.path.join(cli["dir"], "ranks_%s_%d.vcf" % (form, ws))
    more = {"CV_SHARD": "range"}
    if show_ref:
        more["CV_VCF_FORMAT"] = "device"
    codes = _ranks(cli, form, ws, call_fn, ["--showRef"] if show_ref else [], **more)
    assert codes == [0] * ws
    got = open(call_fn, "rb").read()
    assert got == want and got.count(b"\n") > (2500 if show_ref else 200)
    assert not [f for f in os.listdir(cli["dir"]) if ".rank" in f]


def test_a_mistyped_route_ends_every_rank(cli):
    call_fn = os.path.join(cli["dir"], "bogus.vcf")
    codes = _ranks(cli, "plain", 2, call_fn, CV_SHARD="bogus")
    assert all(c not in (0, None) for c in codes) and not os.path.exists(call_fn)
    assert not [f for f in os.listdir(cli["dir"]) if ".rank" in f]
