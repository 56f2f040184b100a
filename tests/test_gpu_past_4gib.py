"""The device entry points on buffers past 2^32 bytes, 2^31 elements and 2^32 elements ("Sizes past 32
bits"): a single narrow product in an address, a narrow grid size or a narrow item count passes every other test of the
suite and corrupts the first real workload.  Each case sits just past the line it is about and is compared, without a
tolerance, with numpy / the host form of the same operation over the CHECKED rows: the first 64, the last 64, the 64 around
each line and 256 seeded others (large_cases.checked_rows).  The shared [8 134 416, 528] fp32 array holds (r * 528 + c) mod
4093 at (r, c): every sum cv_call_postproc forms is exact, and a read from an address wrapped at any of the three lines
gives another value than the right one (test_the_shared_array_tells_a_wrapped_address_apart).

What one inference pass with chunk = n puts where (test_one_pass_whose_largest_map_crosses_2_31_elements), maps in the
workspace's tile-major layout, default variant:
  full, n = 466 048 (19.2 GB of workspace): pool2 3 328 floats per candidate = 6.20 GB and pool3 4 608 = 8.59 GB lie past
    2^32 bytes, pool3 also past 2^31 elements, and both are written and read; pool1 (3.46 GB), fc4 (0.63 GB) and fc5
    (0.33 GB) stay below 2^32 bytes -- pool1, fc4 and fc5 are allocated but not written on this path (fused front, fused tail);
  slim, n = 508 416 (17.3 GB): conv1 and conv2 2 112 floats per candidate = 4.295 GB each, just past 2^32 bytes, conv3
    4 224 = 8.59 GB past 2^31 elements; of these the default path writes conv2 only (the first layer rides in conv2's
    kernel, conv3 stays in the registers of the conv3 + fc4 kernel), so the slim pass crosses the 2^32-byte line in
    a map it uses and the 2^31-element line only in memory it owns; fc4 (98 MB) and fc5 (65 MB) stay below.
No map reaches 2^32 elements: chunk is capped at 2^22 candidates and the workspace would take 38 GB.

cv_parse_tensor_text_dev documents CV_TEXT_SLAB_MAX = 2^31 bytes: the 300 planted rows are parsed as the LAST lines of a
slab of exactly that size, and a slab one byte longer must be refused.  A run of newlines cannot fill the front of such a
slab -- every line, empty or not, owns a slot of the outputs, 2^31 slots of 2 112 bytes --, so the front is ONE line of
zero bytes, which the parser must leave to the host (longer than CV_TEXT_LINE_CAP) before it reaches the rows.

What this file found: dense_tm and dense_rag added a 32-bit byte offset, taken from the start of fc4's input, to a scalar
base.  Past 2^32 bytes (233 024 candidates of the full topology in one pass) a wave read another group's activations:
test_one_pass_whose_largest_map_crosses_2_31_elements[full] got other bits than chunks of 2 048 from the first candidate
behind the line on, without a fault.  The offset now starts at the workgroup's first group.

Seconds per test on one MI355X (pytest --durations; the whole file 5.4 s, 17 passed, none skipped): the shared array
and its wrapped addresses 2.31 (the fill of 17.18 GB and ~1 100 row-sized copies), cv_eval_counts 0.77, one pass full
0.55 (the pass itself 0.029) / slim 0.09 (0.014), cv_forward over 4 067 220 rows 0.48, cv_tensor_rows_text_dev 0.20,
cv_text_gather_rows into the large output 0.13, cv_trainset_gather into the large output 0.09, cv_call_postproc 0.07,
cv_trainset_gather from the large source 0.05, cv_vcf_records_dev 0.04, the other six 0.01 or less.

cv_vcf_merge_dev (test_vcf_merge_gathers_from_and_into_text_past_2_32_bytes, 0.31 s): a source text of 2^32 + 2^20 bytes
whose records all lie in its last MiB (every off past 2^32), 524 352 records of 8 192 bytes -- 4 295 491 584 bytes, so
ooff passes 2^32 at record 524 288, inside vm_gather's wave-per-record path -- and 200 records of 40 to 90 bytes behind
them, whose tiles take the LDS path wholly past the line; source and output 4.30 GB each.
"""
import ctypes
import time

import numpy as np
import pytest

import common
import large_cases as L
from large_cases import NV, ROWS

pytestmark = pytest.mark.gpu


def _abi():
    from clairvoyante_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _room(nbytes, what):
    """a case may skip only where the device has not the memory it needs"""
    import torch
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip("%s needs %.2f GB of device memory, %.2f GB are free" % (what, nbytes / L.GB, free / L.GB))


def _model(arch):
    from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim
    return clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()


@pytest.fixture(scope="module")
def shared():
    s = L.Shared()
    yield s
    s.release()


@pytest.fixture(scope="module")
def rows():
    return L.checked_rows(ROWS)


def _shared_array(shared):
    if shared.buf is None:
        _room((ROWS * NV + L.CANARY_FLOATS) * 4 + (3 << 30), "the shared [%d, %d] fp32 array (17.18 GB)" % (ROWS, NV))
    return shared.array()


# ---- 1. the shared input ---------------------------------------------------------------------------------------------------
def test_the_shared_array_tells_a_wrapped_address_apart(shared, rows):
    x = _shared_array(shared)
    assert x.numel() * 4 > 1 << 32 and x.numel() > 1 << 32
    assert [r * NV < line < (r + 1) * NV for r, (_n, line) in zip(L.LINE_ROWS, L.LINES)] == [True] * 3
    assert all(r in rows and r - 32 in rows and r + 31 in rows for r in L.LINE_ROWS[:2]) and L.LINE_ROWS[2] in rows and ROWS - 1 in rows
    want = L.expected_rows(rows)
    assert np.array_equal(L.read_rows(x, rows), want)
    assert want.max() == L.P - 1 and want.min() == 0
    # a read at the row's offset taken mod 2^32 bytes, mod 2^31 elements or mod 2^32 elements gives 528 other values
    flat = shared.buf
    wrapped = 0
    for k, r in enumerate(rows):
        for _name, line in L.LINES:
            e = int(r) * NV
            if e < line:
                continue                                 # (the row begins in front of the line: its offset does not wrap)
            w = e % line
            got = flat[w:w + NV].cpu().numpy()
            assert not (got == want[k]).any(), (int(r), _name)
            wrapped += 1
    assert wrapped > 3 * 64


# ---- 2. row-indexed entry points over the shared array -------------------------------------------------------------------------
def test_gather_rows_from_the_large_source(shared, rows):
    import torch
    A, lib = _abi()
    x = _shared_array(shared)
    order = np.random.RandomState(5).permutation(rows)
    idx = torch.from_numpy(order).cuda()
    out = torch.full((len(order) + 1, NV), -1.0, device="cuda")
    A.check(lib.cv_text_gather_rows(_p(x), _p(idx), len(order), _p(out), _stream()))
    got = out.cpu().numpy()
    assert np.array_equal(got[:-1], L.expected_rows(order)) and (got[-1] == -1.0).all()


def _small_source(seed):
    """1 000 rows of integers no element of the shared array holds, and ROWS seeded indices into them (on the device)"""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    src = torch.randint(5000, 9000, (1000, NV), generator=g, device="cuda").to(torch.float32)
    idx = torch.randint(0, 1000, (ROWS,), generator=g, device="cuda")
    return src, idx


def test_gather_rows_into_the_large_output(shared, rows):
    A, lib = _abi()
    x = _shared_array(shared)
    src, idx = _small_source(21)
    shared.dirty = True
    A.check(lib.cv_text_gather_rows(_p(src), _p(idx), ROWS, _p(x), _stream()))
    want = src.cpu().numpy()[L.read_rows(idx, rows)]
    assert np.array_equal(L.read_rows(x, rows), want)
    assert shared.canary_intact()


def test_trainset_gather_from_the_large_source(shared, rows):
    import torch
    A, lib = _abi()
    x = _shared_array(shared)
    rng = np.random.RandomState(6)
    k = len(rows)
    src_h = rng.permutation(rows)
    perm_h = rng.permutation(k).astype(np.int64)
    y_h = rng.randint(0, 3, (k, 16)).astype(np.float32) * np.float32(0.5)
    src, perm, y = (torch.from_numpy(a).cuda() for a in (src_h, perm_h, y_h))
    x_out = torch.full((k + 1, NV), -1.0, device="cuda"); y_out = torch.full((k + 1, 16), -1.0, device="cuda")
    A.check(lib.cv_trainset_gather(_p(x), _p(y), _p(src), _p(perm), k, _p(x_out), _p(y_out), _stream()))
    gx, gy = x_out.cpu().numpy(), y_out.cpu().numpy()
    assert np.array_equal(gx[:-1], L.expected_rows(src_h[perm_h])) and (gx[-1] == -1.0).all()
    assert np.array_equal(gy[:-1], y_h[perm_h]) and (gy[-1] == -1.0).all()


def test_trainset_gather_into_the_large_output(shared, rows):
    import torch
    A, lib = _abi()
    x = _shared_array(shared)
    small, perm = _small_source(22)
    g = torch.Generator(device="cuda"); g.manual_seed(23)
    src = torch.randperm(1000, generator=g, device="cuda")
    y = torch.randint(0, 3, (1000, 16), generator=g, device="cuda").to(torch.float32) * 0.5
    y_out = torch.full((ROWS + 1, 16), -1.0, device="cuda")
    shared.dirty = True
    A.check(lib.cv_trainset_gather(_p(small), _p(y), _p(src), _p(perm), ROWS, _p(x), _p(y_out), _stream()))
    p = L.read_rows(perm, rows)
    assert np.array_equal(L.read_rows(x, rows), small.cpu().numpy()[src.cpu().numpy()[p]])
    assert np.array_equal(L.read_rows(y_out, rows), y.cpu().numpy()[p])
    assert shared.canary_intact() and bool((y_out[ROWS] == -1.0).all())


def test_call_postproc_over_the_shared_array(shared, rows):
    import torch
    A, lib = _abi()
    x = _shared_array(shared)
    g = torch.Generator(device="cuda"); g.manual_seed(31)
    out16 = torch.rand((ROWS, 16), generator=g, device="cuda")
    call = torch.full((ROWS + 1, 8), -7, dtype=torch.int32, device="cuda")
    qual = torch.full((ROWS + 1, 4), -7.0, device="cuda")
    m = _model("full")
    try:
        A.check(lib.cv_call_postproc(m._h, _p(x), _p(out16), ROWS, _p(call), _p(qual), _stream()))
        torch.cuda.synchronize()
    finally:
        m.close()
    o, xs = L.read_rows(out16, rows), L.expected_rows(rows).reshape(-1, 33, 4, 4)
    gc, gq = L.read_rows(call, rows), L.read_rows(qual, rows)
    wc, wq = common.decide_all(o, xs)
    assert np.array_equal(gc[:, :5], wc) and not gc[:, 5:].any()
    assert np.array_equal(gq[:, :3].view(np.uint32), wq.view(np.uint32)) and not gq[:, 3].any()
    # the documented order ((s0 + s1) + s2) + s3, restated: every partial sum is an integer below 2^24
    f = np.float32
    s = [xs[:, 16, :, 0], xs[:, 17, :, 1], xs[:, 17, :, 2], xs[:, 16, :, 3]]
    s = [((f(0) + a[:, 0]) + a[:, 1] + a[:, 2]) + a[:, 3] for a in s]
    assert np.array_equal(gq[:, 2], ((s[0] + s[1]) + s[2]) + s[3])
    assert bool((call[ROWS] == -7).all()) and bool((qual[ROWS] == -7.0).all())


def test_vcf_records_whose_rows_lie_past_the_lines(shared, rows):
    import torch
    import test_gpu_vcf_format as V
    A, lib = _abi()
    x = _shared_array(shared)
    n = 300
    pick = np.random.RandomState(8).permutation(np.concatenate([rows[:20], rows[-20:], L.LINE_ROWS, rows[64:-64]]))[:n - 3]
    xrow = np.concatenate([pick, L.LINE_ROWS]).astype(np.int64)
    assert len(xrow) == n and (xrow > L.LINE_ROWS[0]).sum() > 100 and (xrow > L.LINE_ROWS[1]).sum() > 50
    b = V.random_batch(n, 77)
    b.x = L.expected_rows(xrow).reshape(n, 33, 4, 4)           # the same rows gathered small, for the host
    want_text, want_off, want_status, want_info = V.host_form(b, show_ref=True, qual=3)
    up = lambda a: torch.from_numpy(a).cuda()
    call, qual, buf, meta, xr = (up(a) for a in (b.call, b.qual, b.buf, b.meta, xrow))
    off = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda"); status = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    need = ctypes.c_int64(0)
    A.check(lib.cv_vcf_records_workspace(n, ctypes.byref(need)))
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
    cap = len(want_text)
    text = torch.full((cap + V.CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    A.check(lib.cv_vcf_records_dev(_p(call), _p(qual), n, _p(x), _p(xr), _p(buf), _p(meta), None, 1, 1, 3, _p(off), _p(status), _p(info),
                                   _p(text), cap, _p(ws), ws.numel(), _stream()))
    got = text.cpu().numpy().tobytes()
    st = status.cpu().numpy()
    assert np.array_equal(st, want_status) and np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(info.cpu().numpy(), want_info)
    assert got[:cap] == want_text and got[cap:] == b"\xa5" * V.CANARY
    assert (st == V.DEVICE).sum() > n // 2
    o = want_off
    for i in range(n):
        if st[i] != V.HOST:
            assert got[o[i]:o[i + 1]] == V.host_one(b, i, True, 3), i
    if not (st == V.HOST).any():
        assert (want_text, int(want_info[1])) == V.host_batch(b, True, 3)


def test_forward_over_the_first_4_067_220_rows(shared):
    """one cv_forward call over x rows that end behind 2^31 elements, in default chunks, against per-batch calls (what
    tools/gpu_big_call_check.py looked at, at a size that crosses two lines of the input)"""
    import torch
    x = _shared_array(shared)
    n = 4067220
    assert n * NV > 1 << 31
    m = _model("full")
    try:
        m.setParameters(common.bench_params(None, "full"))
        xs = x[:n].view(n, 33, 4, 4)
        one = m.predict_device(xs)
        per = torch.cat([m.predict_device(xs[s:s + 65536]) for s in range(0, n, 65536)])
        torch.cuda.synchronize()
    finally:
        m.close()
    r = L.checked_rows(n, lines=L.LINE_ROWS[:2])
    a, b = L.read_rows(one, r), L.read_rows(per, r)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert a.view(np.uint32).any()
    assert torch.equal(one.view(torch.int32), per.view(torch.int32))


def test_eval_counts_over_4_gib_of_float64_labels(shared):
    import torch
    A, lib = _abi()
    shared.release()
    n = 33554448
    assert n * 16 * 8 > 1 << 32 and n * 16 * 4 > 1 << 31
    _room(n * 16 * 12 + (4 << 30), "cv_eval_counts at n = %d (labels 4.29 GB, outputs 2.15 GB)" % n)
    g = torch.Generator(device="cuda"); g.manual_seed(41)
    y = torch.zeros((n, 16), dtype=torch.float64, device="cuda")
    out = torch.full((n, 16), 0.125, dtype=torch.float32, device="cuda")
    host = {}
    for name, lo, k in (("base", 0, 4), ("zyg", 4, 2), ("type", 6, 4), ("len", 10, 6)):
        t = torch.randint(0, k, (n,), generator=g, device="cuda")
        p = torch.randint(0, k, (n,), generator=g, device="cuda")
        y.scatter_(1, (t + lo)[:, None], 1.0)
        out.scatter_(1, (p + lo)[:, None], 0.875)
        host[name] = (t.to(torch.int16).cpu().numpy().astype(np.int64), p.to(torch.int16).cpu().numpy().astype(np.int64))
        if name == "base":                       # a clear second: another base than the first
            p2 = (p + 1 + torch.randint(0, 3, (n,), generator=g, device="cuda")) % 4
            out.scatter_(1, p2[:, None], 0.5)
            host["base2"] = p2.to(torch.int16).cpu().numpy().astype(np.int64)
            del p2
        del t, p
    counts = torch.zeros(64, dtype=torch.int64, device="cuda")
    A.check(lib.cv_eval_counts(_p(out), _p(y), 1, n, _p(counts), _stream()))
    got = counts.cpu().numpy()
    del y, out
    want = np.zeros(64, dtype=np.int64)
    tb, pb = host["base"]
    want[0] = n; want[1] = int((tb == pb).sum()); want[2] = int(((tb == pb) | (tb == host["base2"])).sum())
    for name, at, k in (("zyg", 4, 2), ("type", 8, 4), ("len", 24, 6)):
        t, p = host[name]
        want[at:at + k * k] = np.bincount(t * k + p, minlength=k * k)
    assert np.array_equal(got, want)
    assert want[4:8].sum() == want[8:24].sum() == want[24:60].sum() == n and 0 < want[1] < want[2] < n


# ---- 3. byte-indexed entry points --------------------------------------------------------------------------------------------
TEXT_LEN = (1 << 32) + (1 << 20)
TAIL0 = (1 << 32) - (1 << 20)                    # the planted part of the text buffer: its last 2 MiB
NEWLINES = ((1 << 32) - 1, 1 << 32, (1 << 32) + 77)
TOKENS = [((1 << 32) + 1000 + 100 * i, b"chr%d" % (i + 1), b"%d" % (123456 + 1000 * i), (b"ACGTTGCA" * 5)[i:i + 33]) for i in range(5)]


@pytest.fixture(scope="module")
def text(shared):
    """zeros, the newlines and the tokens planted; -> (device buffer, the last 2 MiB as bytes)"""
    import torch
    shared.release()
    _room(TEXT_LEN + (1 << 30), "the text buffer of 2^32 + 2^20 bytes")
    buf = torch.zeros(TEXT_LEN + 64, dtype=torch.uint8, device="cuda")
    for at in NEWLINES:
        buf[at] = 10
    for at, ctg, pos, seq in TOKENS:
        line = ctg + b" " + pos + b" " + seq
        buf[at:at + len(line)] = torch.frombuffer(bytearray(line), dtype=torch.uint8).cuda()
    tail = buf[TAIL0:TEXT_LEN].cpu().numpy().tobytes()
    yield buf, tail
    del buf
    torch.cuda.empty_cache()


def test_find_newline_either_side_of_2_32_bytes(text):
    import torch
    A, lib = _abi()
    buf, tail = text
    a, b, c = NEWLINES
    queries = [0, TAIL0 - 5, a - 1, a, b, b + 1, c - 1, c, c + 1, TEXT_LEN - 1, TEXT_LEN, TEXT_LEN + 9, -3]
    from_ = (ctypes.c_int64 * len(queries))(*queries)
    out = torch.full((len(queries) + 1,), -7, dtype=torch.int64, device="cuda")
    A.check(lib.cv_text_find_newline_dev(_p(buf), TEXT_LEN, from_, len(queries), _p(out), _stream()))
    got = out.cpu().numpy()
    want = []
    for q in queries:                            # (everything in front of the planted tail is zero)
        at = tail.find(b"\n", max(q - TAIL0, 0)) if q < TEXT_LEN else -1
        want.append(TAIL0 + at if at >= 0 else TEXT_LEN)
    assert want[:9] == [a, a, a, a, b, c, c, c, TEXT_LEN] and want[9:] == [TEXT_LEN] * 3 + [a]
    assert got[:-1].tolist() == want and got[-1] == -7


def test_gather_tokens_planted_past_2_32_bytes(text):
    import torch
    A, lib = _abi()
    buf, tail = text
    meta = np.zeros((len(TOKENS) + 1, 6), dtype=np.int64)
    for i, (at, ctg, pos, seq) in enumerate(TOKENS):
        meta[i] = [at, len(ctg), at + len(ctg) + 1, len(pos), at + len(ctg) + len(pos) + 2, len(seq)]
    meta[-1] = [(1 << 32) - 3, 6, (1 << 32) + 70, 10, TEXT_LEN - 33, 33]     # tokens that straddle the line, and the last bytes
    index = np.array([5, 3, 0, 4, 1, 2, 5], dtype=np.int64)
    want_bytes, want_meta = b"", []
    for k in index:
        row = []
        for t in range(3):
            s = tail[meta[k, 2 * t] - TAIL0:meta[k, 2 * t] - TAIL0 + meta[k, 2 * t + 1]]
            row += [len(want_bytes), len(s)]
            want_bytes += s
        want_meta.append(row)
    assert b"\n" in want_bytes and b"chr4" in want_bytes
    meta_d, index_d = torch.from_numpy(meta).cuda(), torch.from_numpy(index).cuda()
    out = torch.full((len(want_bytes) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    meta_out = torch.full((len(index) + 1, 6), -7, dtype=torch.int64, device="cuda")
    A.check(lib.cv_text_gather_tokens(_p(buf), _p(meta_d), _p(index_d), len(index), _p(out), len(want_bytes), _p(meta_out), _stream()))
    got = out.cpu().numpy().tobytes()
    assert got[:len(want_bytes)] == want_bytes and got[len(want_bytes):] == b"\xa5" * 64
    assert meta_out.cpu().numpy().tolist() == want_meta + [[-7] * 6]


def test_vcf_merge_gathers_from_and_into_text_past_2_32_bytes():
    """cv_vcf_merge_dev: every record lies in the last MiB of a source text of 2^32 + 2^20 bytes, and 524 352 records of
    8 192 bytes (64 lines, 8 193 copies each, a tie run per line) make an output whose offsets pass 2^32 inside vm_gather's
    wave-per-record path; 200 short records follow in a higher rank, their tiles on the LDS path wholly behind the line.
    The order is numpy's lexsort by (rank, POS, input index)"""
    import torch
    import vcf_merge_big_cases as B
    A, lib = _abi()
    mib, a, line = B.big_case()
    n, n_long = a["n"], B.BIG_LINES * B.BIG_COPIES
    order = B.expected_order(a)
    ooff = np.concatenate(([0], np.cumsum(a["len"][order])))
    total = int(ooff[-1])
    assert a["n_text"] == TEXT_LEN and a["off"].min() >= 1 << 32 and ooff[n_long] == (1 << 32) + 524288 and ooff[524288] == 1 << 32
    need = ctypes.c_int64(-1)
    A.check(lib.cv_vcf_merge_workspace(n, ctypes.byref(need)))
    _room(TEXT_LEN + total + need.value + (2 << 30), "cv_vcf_merge_dev over a source and an output text of 4.3 GB each")
    src = torch.zeros(TEXT_LEN + 64, dtype=torch.uint8, device="cuda")
    src[B.BIG_BASE:TEXT_LEN] = torch.from_numpy(mib).cuda()
    assert src.data_ptr() % 16 == 0
    out = torch.full((total + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    d = [torch.from_numpy(a[k]).cuda() for k in ("pos", "run", "off", "len", "run_rank")]
    srank, sbeg, send, d_ooff = (torch.full((n + 2,), -7, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int64, torch.int64))
    chunks, stats, info = (torch.full((k,), -7, dtype=torch.int64, device="cuda") for k in (4 * n, 4 * 2, 8))
    ws = torch.full((need.value,), 0xAB, dtype=torch.uint8, device="cuda")
    A.check(lib.cv_vcf_merge_dev(_p(src), TEXT_LEN, n, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), a["nruns"], 2, _p(srank), _p(sbeg),
                                 _p(send), _p(d_ooff), _p(out), total, _p(chunks), _p(stats), _p(info), _p(ws), need.value, _stream()))
    assert info.cpu().numpy().tolist()[:3:2] == [0, total]
    got_off = d_ooff.cpu().numpy()
    assert np.array_equal(got_off[:n + 1], ooff) and got_off[n + 1] == -7
    assert np.array_equal(srank.cpu().numpy()[:n], a["rank"][order]) and np.array_equal(sbeg.cpu().numpy()[:n], a["pos"][order] - 1)
    st = stats.cpu().numpy().reshape(4, 2)
    assert st[0].tolist() == [0, ooff[n_long]] and st[1].tolist() == [ooff[n_long], total] and st[2].tolist() == [n_long, 200]
    # the text, on the device: the long records slice by slice from the 64 lines, then the short ones
    lines = src[B.BIG_BASE:B.BIG_BASE + B.BIG_LINES * B.LINE_CAP].view(B.BIG_LINES, B.LINE_CAP)
    which = torch.from_numpy(line[order[:n_long] - B.BIG_SHORT]).cuda()
    per = (256 << 20) // B.LINE_CAP
    for r0 in range(0, n_long, per):
        r1 = min(r0 + per, n_long)
        assert torch.equal(out[r0 * B.LINE_CAP:r1 * B.LINE_CAP], lines[which[r0:r1]].view(-1)), r0
    short = b"".join(mib[int(a["off"][j]) - B.BIG_BASE:int(a["off"][j]) - B.BIG_BASE + int(a["len"][j])].tobytes() for j in order[n_long:])
    tail = out[n_long * B.LINE_CAP:].cpu().numpy().tobytes()
    assert tail == short + b"\xa5" * 256 and len(short) == total - n_long * B.LINE_CAP
    del src, out, lines, which
    torch.cuda.empty_cache()


def _planted_rows():
    import textparse_cases as T
    rng = np.random.RandomState(9)
    vocab = T._vocabulary()
    return ("\n".join(T.good_row(rng, vocab, i) for i in range(300)) + "\n").encode()


def test_parse_rows_at_the_end_of_a_slab_of_the_cap(shared):
    import torch
    import textparse_cases as T
    A, lib = _abi()
    shared.release()
    cap = 1 << 31
    need = ctypes.c_int64()
    A.check(lib.cv_parse_tensor_text_dev_workspace(cap, 310, ctypes.byref(need)))
    _room(cap + need.value + (1 << 30), "a text slab of 2^31 bytes")
    rows_text = _planted_rows()
    first = cap - len(rows_text)                         # the slab: zeros, one newline, the rows as its last lines
    buf = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    buf[first - 1] = 10
    buf[first:cap] = torch.frombuffer(bytearray(rows_text), dtype=torch.uint8).cuda()
    buf[cap:] = 10                                       # (behind the slab: newlines the parser must not count)
    lines = 310
    x = torch.full((lines, NV), float("nan"), device="cuda"); meta = torch.full((lines, 6), -1, dtype=torch.int64, device="cuda")
    status = torch.full((lines,), 255, dtype=torch.uint8, device="cuda"); info = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
    A.check(lib.cv_parse_tensor_text_dev(_p(buf), cap, lines, _p(x), _p(meta), _p(status), _p(info), _p(ws), ws.numel(), _stream()))
    hc, bad, hx, hmeta = T.host_parse(rows_text)
    st = status.cpu().numpy()
    assert bad == 0 and hc == len(rows_text) and hx.shape[0] == 300
    assert info.cpu().numpy().tolist() == [cap, 301, 300, 1]
    assert st[0] == T.HOST and (st[1:301] == T.ROW).all() and (st[301:] == 255).all()
    assert np.array_equal(x[1:301].cpu().numpy().view(np.uint32), hx.view(np.uint32))
    hmeta[:, 0::2] += first
    assert np.array_equal(meta[1:301].cpu().numpy(), hmeta)
    assert bool(torch.isnan(x[301:]).all()) and bool((meta[301:] == -1).all())


def test_parse_refuses_a_slab_past_the_cap():
    import torch
    A, lib = _abi()
    from clairvoyante_amd import _lib
    past = (1 << 31) + 1
    need = ctypes.c_int64(-5)
    assert lib.cv_parse_tensor_text_dev_workspace(past, 4, ctypes.byref(need)) != 0 and need.value == -5
    assert b"range" in lib.cv_last_error()
    A.check(lib.cv_parse_tensor_text_dev_workspace(1 << 31, 4, ctypes.byref(need)))
    room = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = ctypes.c_void_p(room.data_ptr() + (1 << 15))            # every output points into the middle of the canaries
    for length in (past, 1 << 32, (1 << 32) + 5, 1 << 40):
        assert lib.cv_parse_tensor_text_dev(mid, length, 4, mid, mid, mid, mid, mid, 1 << 40, _stream()) != 0
        assert b"range" in lib.cv_last_error()
    with pytest.raises(_lib.CvError, match="range"):
        A.check(lib.cv_parse_tensor_text_dev(mid, past, 4, mid, mid, mid, mid, mid, 1 << 40, _stream()))
    torch.cuda.synchronize()
    assert bool((room == 0xA5).all())


def test_tensor_rows_text_past_2_32_bytes(shared):
    import torch
    import test_gpu_rowtext as R
    A, lib = _abi()
    shared.release()
    rows, ctg = 1999000, "ctgA"
    centres = 100 + 5 * np.arange(rows, dtype=np.int64)
    digits = 1 + sum((centres >= 10 ** k).astype(np.int64) for k in range(1, 13))
    lens = len(ctg) + 1 + digits + 1 + 33 + NV * 4 + 1             # "<ctg> <centre> <33 bases>" + 528 x " 0.0" + newline
    want_off = np.concatenate(([0], np.cumsum(lens)))
    total = int(want_off[rows])
    assert total > (1 << 32) + (1 << 20) and set(digits.tolist()) == {3, 4, 5, 6, 7}
    _room(rows * NV * 4 + total + (2 << 30), "cv_tensor_rows_text_dev over %d rows (counts 4.22 GB, text %.2f GB)" % (rows, total / L.GB))
    ref = R.make_ref(int(centres[-1]) + 40)
    cen, rf = torch.from_numpy(centres).cuda(), torch.from_numpy(np.frombuffer(ref, dtype=np.uint8).copy()).cuda()
    counts = torch.zeros((rows, NV), device="cuda")
    off = torch.full((rows + 2,), -7, dtype=torch.int64, device="cuda"); status = torch.full((rows + 1,), 9, dtype=torch.uint8, device="cuda")
    need = ctypes.c_int64(0)
    A.check(lib.cv_tensor_rows_text_workspace(rows, ctypes.byref(need)))
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device="cuda")
    room = torch.full((3 + total + R.CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    cb = ctg.encode()
    A.check(lib.cv_tensor_rows_text_dev(cb, len(cb), _p(cen), rows, _p(rf), 0, len(ref), _p(counts), _p(off), _p(status),
                                        ctypes.c_void_p(room.data_ptr() + 3), total, _p(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    got_off = off.cpu().numpy()
    assert np.array_equal(got_off[:rows + 1], want_off) and got_off[rows + 1] == -7
    assert not status[:rows].any() and int(status[rows]) == 9
    assert room[:3].cpu().numpy().tobytes() == b"\xa5" * 3 and room[3 + total:].cpu().numpy().tobytes() == b"\xa5" * R.CANARY
    line = int(np.searchsorted(want_off, 1 << 32, side="right")) - 1        # the row whose text straddles 2^32 bytes
    assert want_off[line] < 1 << 32 < want_off[line + 1] and line < rows - 64
    check = L.checked_rows(rows, lines=(line,))
    want = R.host_rows(ctg, centres[check], ref, 0, np.zeros((len(check), NV), dtype=np.float32))
    for r, w in zip(check, want):
        a = 3 + int(want_off[r])
        assert room[a:a + len(w)].cpu().numpy().tobytes() == w, int(r)
    # behind the line every row starts where off[] says: with the contig name, and with a newline in front of it
    behind = torch.from_numpy(want_off[line + 1:rows]).cuda() + 3
    assert len(behind) > 5000
    for k, ch in enumerate(b"\n" + cb + b" "):
        assert bool((room[behind + (k - 1)] == ch).all()), k


# ---- 4. one inference pass whose maps cross the lines ----------------------------------------------------------------------------
def _map_floats(m):
    """floats per candidate of the maps a pass keeps in the workspace (tile-major: channels in fragments of 16), from the
    model's own shapes"""
    sh = m.paramShapes()
    pools = [1 if p is None else p[0] for p in (m.pollSize1, m.pollSize2, m.pollSize3)]
    up16 = lambda v: (v + 15) // 16 * 16
    h, per = 33, {}
    for l in range(3):
        h -= pools[l] - 1
        per["map%d" % (l + 1)] = h * 4 * up16(sh["conv%d/kernel" % (l + 1)][3])
    assert sh["fc4/kernel"][0] == h * 4 * sh["conv3/kernel"][3]
    per["fc4"] = up16(sh["fc4/kernel"][1]); per["fc5"] = up16(sh["fc5/kernel"][1])
    return per


@pytest.mark.parametrize("arch", ["full", "slim"])
def test_one_pass_whose_largest_map_crosses_2_31_elements(arch, oracle, shared):
    import torch
    from clairvoyante_amd import synth
    shared.release()
    m = _model(arch)
    try:
        per = _map_floats(m)
        largest = max(per.values())
        n = ((1 << 31) // largest // 16 + 1) * 16
        assert (n - 16) * largest <= 1 << 31 < n * largest and n <= 1 << 22
        assert (arch, largest, n) in (("full", 4608, 466048), ("slim", 4224, 508416))
        ws = sum(per.values()) * 4 * n
        _room(ws + n * (NV + 32) * 4 + (3 << 30), "one %s pass of %d candidates (workspace %.1f GB)" % (arch, n, ws / L.GB))
        P = common.bench_params(oracle, arch)
        m.setParameters(P)
        xd = synth.make_candidates(n, seed=83, device="cuda")
        m.setOption("chunk", 2048)
        want = m.predict_device(xd)
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        m.setOption("chunk", n)
        t0 = time.perf_counter()
        got = m.predict_device(xd)
        torch.cuda.synchronize()
        print("%s: one pass of %d candidates %.3f s (first call: the workspace is allocated)" % (arch, n, time.perf_counter() - t0))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        again = m.predict_device(xd)
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        if arch == "full":
            # fc4's other two large-pass kernels read the same map through the same kind of offset: the three slabs on
            # ragged waves (dense_rag) and on whole groups (dense_tm<7, 8>), fc5 and the heads behind them from the fc4 map
            for forced in ({"infer_slab_groups": 65536}, {"dense_rag": -1, "infer_slab_groups": 65536}):
                try:
                    for k, v in forced.items():
                        m.setOption(k, v)
                    slabs = m.predict_device(xd)
                    assert torch.equal(slabs.view(torch.int32), want.view(torch.int32)), forced
                finally:
                    for k in forced:
                        m.setOption(k, common.FORCED_LAUNCH_DEFAULTS[k])
                del slabs
        # the candidates either side of the place where each map crosses a line, held to the oracle directly
        lines = sorted(set(line // f for f in per.values() for _name, line in L.LINES if line // f < n))
        assert len(lines) >= 2 and (1 << 31) // largest in lines
        r = L.checked_rows(n, lines=lines)
        ref = oracle.forward_all(arch, P, L.read_rows(xd, r))
        assert np.array_equal(L.read_rows(got, r).view(np.uint32), ref["out"].view(np.uint32))
    finally:
        m.setOption("chunk", 65536)
        m.close()
        torch.cuda.empty_cache()


# ---- 5. documented limits are refusals, not wraps ---------------------------------------------------------------------------------
def test_documented_limits_refuse():
    import torch
    A, lib = _abi()
    from clairvoyante_amd import _lib
    room = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = ctypes.c_void_p(room.data_ptr() + (1 << 15))
    st = _stream()
    m = _model("slim")
    try:
        v = ctypes.c_int64()
        for bad in ((1 << 22) + 1, 1 << 31, (1 << 32) + 16, 15, 0, -16):
            with pytest.raises(_lib.CvError, match="chunk"):
                m.setOption("chunk", bad)
            A.check(lib.cv_get_option(m._h, b"chunk", ctypes.byref(v)))
            assert v.value == 65536
        m.setOption("chunk", 1 << 22)
        A.check(lib.cv_get_option(m._h, b"chunk", ctypes.byref(v)))
        assert v.value == 1 << 22
    finally:
        m.close()
    # the int32 tables of cv_trainset_finish, the scans of the record and row writers: 2^30 items and no more
    need = ctypes.c_int64(-5)
    for past in ((1 << 30) + 1, 1 << 31, (1 << 32) + 7):
        for ws_fn in (lib.cv_trainset_finish_workspace, lib.cv_trainset_tokens_workspace, lib.cv_vcf_records_workspace,
                      lib.cv_tensor_rows_text_workspace):
            assert ws_fn(past, ctypes.byref(need)) != 0 and need.value == -5 and b"range" in lib.cv_last_error()
        assert lib.cv_trainset_finish(past, mid, mid, mid, mid, mid, mid, mid, 1, mid, 0, mid, mid, mid, mid, 1 << 40, st) != 0
        assert b"range" in lib.cv_last_error()
        assert lib.cv_trainset_gather(mid, mid, mid, None, past, mid, mid, st) != 0 and b"range" in lib.cv_last_error()
        assert lib.cv_trainset_tokens(mid, mid, None, past, mid, mid, mid, mid, mid, mid, 1 << 40, st) != 0 and b"range" in lib.cv_last_error()
        assert lib.cv_trainset_join(past, mid, mid, 1, mid, 0, 0, None, None, None, None, None, mid, mid, mid, st) != 0
        assert b"range" in lib.cv_last_error()
        assert lib.cv_vcf_records_dev(mid, mid, past, mid, None, mid, mid, None, 1, 0, 0, mid, mid, mid, mid, 1 << 40, mid, 1 << 40, st) != 0
        assert b"range" in lib.cv_last_error()
        assert lib.cv_tensor_rows_text_dev(b"c", 1, mid, past, mid, 0, 100, mid, mid, mid, mid, 1 << 40, mid, 1 << 40, st) != 0
        assert b"range" in lib.cv_last_error()
    torch.cuda.synchronize()
    assert bool((room == 0xA5).all())
