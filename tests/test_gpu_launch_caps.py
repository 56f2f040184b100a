"""The data-plane kernels past their launch caps (tests/launch_cap_cases.py is the inventory): a capped launch stops
growing at a constant and a loop inside the kernel walks the items beyond it.  Each test here is the smallest shape at
which a thread, wave or block of its kernels makes a SECOND trip -- items = line + R, R ragged --, and 2 * line + R as
well where a wave reduction follows the loop, so that lanes of one wave make two and three trips.  Results are integers,
bytes or copied floats and are compared exactly, with the header's *_host_form where there is one, cv_draws_host for the
draws, the host parser for the text rows, and otherwise a vectorised numpy restatement of the header's contract.

Every output starts as a sentinel the result cannot hold (torch.full, never torch.empty: the caching allocator hands
back the last test's right answer) with a canary stretch behind it, and every workspace has exactly the size its query
names.  Inputs are built once per module with numpy; no test body loops over rows in Python.  Behind every line lie
R = 77 rows, so what a kernel has to tell apart (contigs, run starts, verdicts, flags) is planted among those 77.

That the tests bite: with CV_GRID_STRIDE cut to one trip, every test here whose kernels sit behind cv_grid_for fails; the
others hold kernels with loops of their own (ik_copy, tp_parse_rows and the index kernels, the decoders, the packer,
bam_gather) or, test_three_rows_over_65535_contigs, a loop that never strides.

The VCF merge (section 10; inputs from tests/vcf_merge_big_cases.py, held to their claims on the CPU by
test_vcf_merge_big_cases_host.py): vm_fields, vm_sorted, vm_heads, vm_chunks, vm_chunk_out and vw_min cross GRID_FOR at
1 048 653 records, vw_fill at 1 162 900 windows, vw_backfill its 1 024 blocks at 1 100 contig ranks, vm_gather its
65 536 blocks x 64 records at 4 194 381 records (its workspace is 340 281 088 bytes by the query: under the 512 MB a
buffer of a test here may take, which _merge_call asserts).
That they bite, each with a library built from a scratch copy for one run: with vm_gather's tile loop cut to one trip
test_vcf_gather_past_the_tile_line fails (the text of tiles 65 536 and 65 537 keeps its sentinel); with CV_GRID_STRIDE
cut to one trip test_vcf_merge_past_the_grid_stride_line fails at info (83 407 chunks for 83 430).  That second run had
the workspace filled with zeros: vm_fields' unwritten line numbers are indices, and 0xAB bytes would have been wild ones.
Seconds on one MI355X (pytest --durations): the merge past the grid-stride line 2.8 (two builds, two host forms, two
device calls), the gather past the tile line 1.5, the rank widths 0.05.

The lines, as arithmetic on the sources' own constants:"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID_FOR = 4096 * 256              # csrc/cv_dev_common.hpp, cv_grid_for: max_grid 4096 blocks x 256 threads, CV_GRID_STRIDE
GATHER_PIECES = 528 // 4 + 4       # csrc/cv_trainset.hip, ts_gather: 16-byte pieces of one item (its row and its label)
GATHER_LINE = -(-GRID_FOR // GATHER_PIECES)      # 7 711 rows: the first count whose pieces exceed GRID_FOR
LABEL_LINE = GRID_FOR // 16 + 1    # csrc/cv_trainset.hip, ts_labels walks entries * 16: 65 537 entries
COPY_LINE = 65536 * (256 // 64)    # csrc/cv_beditems_dev.hip, ik_copy: 65 536 blocks x 4 waves, one wave per row
PARSE_LINE = 2048 * 4              # csrc/cv_textparse.hip, tp_parse_rows: PARSE_GRID x PARSE_WAVES, one wave per line
TILE_LINE = 2048 * 4096            # csrc/cv_textparse.hip, tp_count_newlines / tp_line_ends: INDEX_GRID tiles of TILE bytes
TOKEN_LINE = 4096 * 256            # csrc/cv_textparse.hip, tp_token_copy: 4 096 blocks x 256 rows
GZIP_LINE = 4096 * 4               # csrc/cv_gzip_dev.hip, gzip_find / gzip_decode: GRID blocks x WAVES, one wave per guess / chunk
GZIP_REST_LINE = 4096 * 256 * 8    # csrc/cv_gzip_dev.hip, gzip_rest: GRID blocks of 256 threads sized for 8 symbols each
BLOSC_LINE = 8192 * 4              # csrc/cv_blosc_dev.hip, blosc_decode: DECODE_GRID x DECODE_WAVES, one wave per stream
PACK_LINE = 1 << 20                # csrc/cv_blosc_pack_dev.hip, pack_encode / pack_assemble: MAX_GRID blocks, one per stream
WALK_LINE = 4096                   # csrc/cv_bam_dev.hip, bam_gather: 4 096 blocks, one per walker
MERGE_TILE_LINE = 65536 * 64       # csrc/cv_vcfmerge_dev.hip, vm_gather: 65 536 one-wave blocks, a tile of 64 output records each
BACKFILL_LINE = 1024               # csrc/cv_vcfmerge_dev.hip, vw_backfill: 1 024 blocks, one contig rank each
TEST_BYTES = 512 << 20             # the largest single buffer a test here allocates
WSIZE, MARK = 32768, 0x8000        # csrc/cv_gzip_core.hpp: the window, the marker bit of a symbol
R = 77                             # ragged: no multiple of 16, 64 or 256
CANARY = 96                        # elements of sentinel behind every output
WS_FILL = 0xAB                     # what a workspace holds before its call
MAX_CONTIGS = 65535                # CV_TRAINSET_MAX_CONTIGS
P10 = 10 ** np.arange(13, dtype=np.int64)

assert R % 16 and R % 64 and R % 256 and (GATHER_LINE - 1) * GATHER_PIECES <= GRID_FOR < GATHER_LINE * GATHER_PIECES


# ---- plumbing -------------------------------------------------------------------------------------------------------------
def _abi():
    from clairvoyante_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _hp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


SENTINEL = {"int64": -7, "int32": -7, "int16": -7, "uint8": 0xAB, "float32": float("nan"), "float64": float("nan")}


class Out(object):
    """an output of k rows filled with its sentinel, CANARY more rows behind it"""

    def __init__(self, k, dtype, width=None):
        import torch
        self.k = int(k)
        shape = (self.k + CANARY,) if width is None else (self.k + CANARY, width)
        self.t = torch.full(shape, SENTINEL[dtype], dtype=getattr(torch, dtype), device="cuda")
        self.dtype = dtype

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def untouched(self, a):
        s = SENTINEL[self.dtype]
        return bool(np.isnan(a).all()) if s != s else bool((a == s).all())

    def get(self, used=None):
        """the first `used` rows (default: all k); asserts that everything behind them still holds the sentinel"""
        a = self.t.cpu().numpy()
        used = self.k if used is None else int(used)
        assert self.untouched(a[used:]), "written behind row %d" % used
        return a[:used]


def _workspace(query, *args):
    """a workspace of exactly the bytes the query names"""
    import torch
    A, _lib = _abi()
    need = ctypes.c_int64(-1)
    A.check(query(*(args + (ctypes.byref(need),))))
    assert need.value > 0
    return torch.full((need.value,), WS_FILL, dtype=torch.uint8, device="cuda"), need.value


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _decimal(values, lead_zero=None):
    """canonical decimal of non-negative int64 values -> (bytes [n, 15], lengths); rows of lead_zero get a '0' in front"""
    d = 1 + sum((values >= P10[k]).astype(np.int64) for k in range(1, 13))
    mat = np.full((len(values), 15), 32, dtype=np.uint8)
    for j in range(13):
        e = d - 1 - j
        m = e >= 0
        mat[m, j] = (values[m] // P10[e[m]]) % 10 + 48
    lens = d.copy()
    if lead_zero is not None and lead_zero.any():
        mat[lead_zero, 1:14] = mat[lead_zero, 0:13]
        mat[lead_zero, 0] = 48
        lens[lead_zero] += 1
    return mat, lens


def _names_column(names, ids):
    w = max(len(s) for s in names)
    table = np.full((len(names), w), 32, dtype=np.uint8)
    for k, s in enumerate(names):
        table[k, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return table[ids], np.array([len(s) for s in names], dtype=np.int64)[ids]


def _join_columns(cols):
    """rows of blank-separated tokens, a newline behind each; cols = [(bytes [n, w], lengths [n])] -> (text uint8,
    offset of every row, per column its offsets)"""
    n = len(cols[0][1])
    row_len = sum(l for _m, l in cols) + len(cols)
    row_off = np.concatenate(([0], np.cumsum(row_len)))
    buf = np.full(int(row_off[-1]), 32, dtype=np.uint8)
    buf[row_off[1:] - 1] = 10
    at, col_off = row_off[:-1].copy(), []
    for mat, lens in cols:
        col_off.append(at.copy())
        for k in range(mat.shape[1]):
            m = lens > k
            if not m.any():
                break
            buf[at[m] + k] = mat[m, k]
        at = at + lens + 1
    assert n == len(row_len)
    return buf, row_off, col_off


def _runs(rng, n, nctg, mean, tail=R, short=5):
    """contig id per row, in runs of about `mean` rows, the last `tail` rows in runs of `short` rows that cycle through
    every contig (the stretch behind a line is R rows); consecutive runs differ -> (ids, run index per row, id per run)"""
    body = n - tail
    nruns = max(body // mean, 2 * nctg)
    cut = np.sort(rng.choice(np.arange(1, body), nruns - 1, replace=False))
    run_ctg = rng.randint(0, nctg, nruns)
    same = np.flatnonzero(run_ctg[1:] == run_ctg[:-1]) + 1
    while len(same):
        run_ctg[same] = (run_ctg[same] + 1 + rng.randint(0, nctg - 1, len(same))) % nctg
        same = np.flatnonzero(run_ctg[1:] == run_ctg[:-1]) + 1
    ntail = -(-tail // short)
    run_ctg = np.concatenate((run_ctg, (run_ctg[-1] + 1 + np.arange(ntail)) % nctg))
    run = np.zeros(n, dtype=np.int64)
    run[cut] = 1
    run[body + short * np.arange(ntail)] = 1
    run = np.cumsum(run)
    return run_ctg[run].astype(np.int32), run.astype(np.int32), run_ctg.astype(np.int32)


def _pool(rng, k):
    """k distinct positions of 1 .. 12 digits, sorted: more than 32 bits of position"""
    d = rng.randint(1, 13, 2 * k)
    p = np.unique((rng.random_sample(2 * k) * (P10[d] - P10[d - 1])).astype(np.int64) + P10[d - 1])
    p = rng.permutation(p)[:k]
    assert len(p) == k
    return np.sort(p)


def _per_contig_tables(rng, pool, nctg, share, with_ends):
    """per contig a sorted sample of the pool; -> (off [nctg + 1], values) and, with_ends, the running maximum of ends that
    reach 0 .. 3 positions past each begin (the tables cv_bed_table_dev writes)"""
    parts = [np.sort(rng.choice(pool, int(len(pool) * share), replace=False)) for _c in range(nctg)]
    off = np.concatenate(([0], np.cumsum([len(q) for q in parts]))).astype(np.int64)
    vals = np.concatenate(parts)
    if not with_ends:
        return off, vals
    emax = np.concatenate([np.maximum.accumulate(q + rng.randint(0, 4, len(q))) for q in parts])
    return off, vals, emax


def _stab(off, begin, emax, ctg, pos, ntab):
    """the header's BED test per row: upper_bound(begin, pos) = k > 0 and emax[k - 1] > pos, inside the contig's stretch"""
    keep = np.zeros(len(pos), dtype=bool)
    for c in np.unique(ctg):
        if c < 0 or c >= ntab:
            continue
        m = np.flatnonzero(ctg == c)
        b, e = begin[off[c]:off[c + 1]], emax[off[c]:off[c + 1]]
        k = np.searchsorted(b, pos[m], side="right")
        keep[m] = (k > 0) & (e[np.maximum(k - 1, 0)] > pos[m])
    return keep


def _everything_behind(line, *arrays):
    """every value an array takes appears behind the line too, not only in front"""
    return all(set(np.unique(a[line:]).tolist()) == set(np.unique(a).tolist()) for a in arrays)


NAMES = (b"chr1", b"chr10", b"chr2", b"c", b"chrUn_KI270742v1")     # the last one has no table rows (ntab = 4)
NTAB = 4


class Rows(object):
    """GRID_FOR + R rows "contig position sequence" as the parser leaves them (text in HBM, meta [n, 6]) and everything
    the three trainset calls must make of them, from the arrays the text was written from"""

    def __init__(self):
        rng = np.random.RandomState(101)
        n = self.n = GRID_FOR + R
        self.ctg, self.run, self.run_ctg = _runs(rng, n, len(NAMES), 3000)
        self.pool = _pool(rng, n // 8)
        self.pos = self.pool[rng.randint(0, len(self.pool), n)]
        r = np.arange(n)
        t = np.where(r >= GRID_FOR, r - GRID_FOR, -1)               # (behind the line every kind is planted among the R rows)
        self.bad_coord = (r % 1009 == 5) | (t % 13 == 2)            # "0" + digits: no canonical decimal
        seq_len = 17 + r % 4
        seq_len[(r % 1013 == 7) | (t % 17 == 3)] = 16               # no centre base
        seq = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.randint(0, 8, (n, 20))].copy()
        seq[(r % 499 == 3) | (t % 19 == 4), 16] = ord("N")
        colon = (r % 1021 == 9) | (t % 23 == 5)
        seq[colon, 3] = ord(":")
        high = (r % 1031 == 11) | (t % 29 == 6)
        seq_len[high] = 19 + r[high] % 2
        seq[high, 18] = 0xC3
        pm, pl = _decimal(self.pos, self.bad_coord)
        nm, nl = _names_column(NAMES, self.ctg)
        self.text, self.row_off, (co, po, so) = _join_columns([(nm, nl), (pm, pl), (seq, seq_len)])
        self.meta = np.stack([co, nl, po, pl, so, seq_len], axis=1).astype(np.int64)
        # what cv_trainset_tokens must say
        self.want_pos = np.where(self.bad_coord, 0, self.pos)
        self.want_digits = np.where(self.bad_coord, 0, pl).astype(np.uint8)
        c = seq[:, 16].copy()
        c[(c >= 97) & (c <= 122)] -= 32
        base = np.full(n, 255, dtype=np.uint8)
        for k, ch in enumerate(b"ACGT"):
            base[c == ch] = k
        base[seq_len <= 16] = 255
        self.want_centre = base
        start = np.concatenate(([True], self.run[1:] != self.run[:-1]))
        bad_seq = (base == 255) | colon | high
        self.item_host = self.bad_coord | high                      # as an item line: a byte outside 0x21 .. 0x7E
        self.want_flags = (start * 1 + self.bad_coord * 2 + bad_seq * 4).astype(np.uint8)
        # the tables cv_trainset_join reads, and what it must say
        self.bed_off, self.bed_begin, self.bed_emax = _per_contig_tables(rng, self.pool, NTAB, 0.5, True)
        self.truth_off, self.truth_pos = _per_contig_tables(rng, self.pool, NTAB, 0.3, False)
        self.labels = (rng.randint(0, 3, (len(self.truth_pos), 16)) * 0.5).astype(np.float32)
        self.want_keep = _stab(self.bed_off, self.bed_begin, self.bed_emax, self.ctg, self.want_pos, NTAB)
        t = np.full(n, -1, dtype=np.int32)
        for k in range(NTAB):
            m = np.flatnonzero(self.ctg == k)
            q = self.truth_pos[self.truth_off[k]:self.truth_off[k + 1]]
            u = np.searchsorted(q, self.want_pos[m], side="right")
            hit = (u > 0) & (q[np.maximum(u - 1, 0)] == self.want_pos[m])
            t[m[hit]] = (self.truth_off[k] + u[hit] - 1).astype(np.int32)
        self.want_truth = t
        f = self.want_flags
        assert _everything_behind(GRID_FOR, self.ctg, f & 1, f & 2, f & 4, self.want_centre, self.want_keep, self.want_truth >= 0)
        assert self.pos.max() > 1 << 32 and len(self.run_ctg) > 300 and len(np.unique(pl[GRID_FOR:])) > 6


@pytest.fixture(scope="module")
def rows():
    return Rows()


@pytest.fixture(scope="module")
def rows_dev(rows):
    """the text and the meta rows on the device, the meta rows in REVERSE so that an index list has something to say"""
    import torch
    text = _up(rows.text)
    meta = _up(rows.meta[::-1])
    idx = _up(np.arange(rows.n - 1, -1, -1, dtype=np.int64))
    yield text, meta, idx
    del text, meta, idx
    torch.cuda.empty_cache()


# ---- 1. the trainset calls (ts_tokens, ts_run_index, ts_join, ts_keys, ts_heads, ts_entries, ts_labels, ts_gather) ------------
@pytest.fixture(scope="module")
def tokens(rows, rows_dev):
    """cv_trainset_tokens over the GRID_FOR + R rows -> its five outputs as Out"""
    A, lib = _abi()
    text, meta, idx = rows_dev
    n = rows.n
    o = {"pos": Out(n, "int64"), "digits": Out(n, "uint8"), "centre": Out(n, "uint8"), "flags": Out(n, "uint8"), "run": Out(n, "int32")}
    ws, need = _workspace(lib.cv_trainset_tokens_workspace, n)
    A.check(lib.cv_trainset_tokens(_p(text), _p(meta), _p(idx), n, o["pos"].p, o["digits"].p, o["centre"].p, o["flags"].p, o["run"].p,
                                   _p(ws), need, _stream()))
    return o


def test_trainset_tokens_past_the_grid_stride_line(rows, tokens):
    assert np.array_equal(tokens["pos"].get(), rows.want_pos)
    assert np.array_equal(tokens["digits"].get(), rows.want_digits)
    assert np.array_equal(tokens["centre"].get(), rows.want_centre)
    assert np.array_equal(tokens["flags"].get(), rows.want_flags)
    assert np.array_equal(tokens["run"].get(), rows.run)              # hipcub InclusiveSum past its single tile, then ts_run_index


@pytest.fixture(scope="module")
def joined(rows):
    """cv_trainset_join over the rows, fed with the columns the tokens call must have written"""
    A, lib = _abi()
    n = rows.n
    o = {"ctg": Out(n, "int32"), "keep": Out(n, "uint8"), "truth": Out(n, "int32")}
    d = [_up(a) for a in (rows.run, rows.run_ctg, rows.want_pos, rows.bed_off, rows.bed_begin, rows.bed_emax, rows.truth_off, rows.truth_pos)]
    A.check(lib.cv_trainset_join(n, _p(d[0]), _p(d[1]), len(rows.run_ctg), _p(d[2]), NTAB, 1, _p(d[3]), _p(d[4]), _p(d[5]), _p(d[6]),
                                 _p(d[7]), o["ctg"].p, o["keep"].p, o["truth"].p, _stream()))
    return o


def test_trainset_join_past_the_grid_stride_line(rows, joined):
    assert np.array_equal(joined["ctg"].get(), rows.ctg)
    assert np.array_equal(joined["keep"].get().astype(bool), rows.want_keep)
    assert np.array_equal(joined["truth"].get(), rows.want_truth)
    assert 0.2 < rows.want_keep.mean() < 0.8 and (rows.want_truth >= 0).sum() > rows.n // 10


def _finish_definition(ctg, pos, digits, centre, keep, truth, rank, labels):
    """cv_trainset_finish restated: the kept rows sorted (stable) by (rank of the contig, pos * 10^(12 - digits), digits),
    one entry per distinct key, src = its LAST arrival, the centre base of its FIRST arrival -> (src, y)"""
    valid = np.flatnonzero(keep & (digits >= 1) & (digits <= 12))
    d = digits[valid].astype(np.int64)
    scaled = pos[valid] * P10[12 - d]
    rk = rank[ctg[valid]].astype(np.int64)
    order = np.lexsort((valid, d, scaled, rk))
    v, d, scaled, rk = valid[order], d[order], scaled[order], rk[order]
    head = np.concatenate(([True], (rk[1:] != rk[:-1]) | (scaled[1:] != scaled[:-1]) | (d[1:] != d[:-1])))
    first = v[head]
    src = v[np.concatenate((head[1:], [True]))]
    t = truth[src]
    y = np.zeros((len(src), 16), dtype=np.float32)
    y[:, [5, 6, 10]] = 1.0
    cb = centre[first]
    ok = cb < 16
    y[np.flatnonzero(ok), cb[ok]] = 1.0
    y[t >= 0] = labels[t[t >= 0]]
    return src, y


def test_trainset_finish_past_the_grid_stride_line(rows):
    """ts_keys / ts_heads / ts_entries over GRID_FOR + R rows, ts_labels over more than LABEL_LINE entries, the radix sort
    and the scan past their single-tile paths; more than a quarter of the kept rows repeat an earlier key"""
    A, lib = _abi()
    n = rows.n
    rank = np.array([2, 0, 3, 1, 4], dtype=np.int32)
    src_w, y_w = _finish_definition(rows.ctg, rows.want_pos, rows.want_digits, rows.want_centre, rows.want_keep, rows.want_truth, rank,
                                    rows.labels)
    total_w = len(src_w)
    kept = int((rows.want_keep & (rows.want_digits > 0)).sum())
    assert total_w > LABEL_LINE + R and kept - total_w > kept // 4 and (src_w > GRID_FOR).any()
    d = [_up(a) for a in (rows.ctg, rows.want_pos, rows.want_digits, rows.want_centre, rows.want_keep.astype(np.uint8), rows.want_truth,
                          rank, rows.labels)]
    src, y, total = Out(n, "int64"), Out(n, "float32", 16), Out(1, "int64")
    ws, need = _workspace(lib.cv_trainset_finish_workspace, n)
    A.check(lib.cv_trainset_finish(n, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), _p(d[5]), _p(d[6]), len(rank), _p(d[7]),
                                   len(rows.labels), src.p, y.p, total.p, _p(ws), need, _stream()))
    assert int(total.get()[0]) == total_w
    assert np.array_equal(src.get(total_w), src_w)
    assert np.array_equal(y.get(total_w).view(np.uint32), y_w.view(np.uint32))
    assert (y_w.sum(axis=1) != 4).any() and (rows.want_truth[src_w] < 0).any()


def test_trainset_gather_past_the_grid_stride_line():
    """ts_gather walks total * 136 pieces: GATHER_LINE + R rows are the first few past GRID_FOR pieces"""
    import torch
    A, lib = _abi()
    rng = np.random.RandomState(102)
    total, m = GATHER_LINE + R, 1000
    x_all = rng.randint(-500, 500, (m, 528)).astype(np.float32)
    y = (rng.randint(0, 3, (total, 16)) * 0.5).astype(np.float32)
    src = rng.randint(0, m, total).astype(np.int64)
    perm = rng.permutation(total).astype(np.int64)
    d = [_up(a) for a in (x_all, y, src, perm)]
    for pm, want_from in ((d[3], perm), (None, np.arange(total))):
        x_out, y_out = Out(total, "float32", 528), Out(total, "float32", 16)
        A.check(lib.cv_trainset_gather(_p(d[0]), _p(d[1]), _p(d[2]), _p(pm), total, x_out.p, y_out.p, _stream()))
        assert np.array_equal(x_out.get(), x_all[src[want_from]]) and np.array_equal(y_out.get(), y[want_from])
    torch.cuda.synchronize()


def test_gather_tokens_past_the_token_copy_line(rows, rows_dev):
    """tp_token_copy over TOKEN_LINE + R rows, tp_token_offsets' carry over 1 025 steps of its one workgroup; in list order
    the tokens back to back are the text without its blanks and newlines"""
    A, lib = _abi()
    text, meta, idx = rows_dev
    n = rows.n
    assert n == TOKEN_LINE + R
    want = rows.text[(rows.text != 32) & (rows.text != 10)]
    lens = rows.meta[:, 1::2]
    start = np.concatenate(([0], np.cumsum(lens.reshape(-1))))[:-1].reshape(n, 3)
    want_meta = np.stack([start[:, 0], lens[:, 0], start[:, 1], lens[:, 1], start[:, 2], lens[:, 2]], axis=1)
    out, meta_out = Out(len(want), "uint8"), Out(n, "int64", 6)
    A.check(lib.cv_text_gather_tokens(_p(text), _p(meta), _p(idx), n, out.p, len(want), meta_out.p, _stream()))
    assert np.array_equal(meta_out.get(), want_meta)
    assert np.array_equal(out.get(), want)


# ---- 2. the line passes (il_verdicts, il_rows, tl_verdicts, tl_rows, tp_run_flags, the index kernels) ---------------------------
def _item_lines(lib, A, text_h, text_d, max_lines):
    """cv_item_lines_dev against cv_item_lines_host_form -> the host form's (pos, run, off, len, tok, info)"""
    o = {"pos": Out(max_lines, "int64"), "run": Out(max_lines, "int32"), "off": Out(max_lines, "int64"), "len": Out(max_lines, "int64"),
         "tok": Out(max_lines, "int64", 2), "info": Out(8, "int64")}
    ws, need = _workspace(lib.cv_item_lines_workspace, len(text_h), max_lines)
    A.check(lib.cv_item_lines_dev(_p(text_d), len(text_h), max_lines, o["pos"].p, o["run"].p, o["off"].p, o["len"].p, o["tok"].p,
                                  o["info"].p, _p(ws), need, _stream()))
    h = {"pos": np.zeros(max_lines, np.int64), "run": np.zeros(max_lines, np.int32), "off": np.zeros(max_lines, np.int64),
         "len": np.zeros(max_lines, np.int64), "tok": np.zeros((max_lines, 2), np.int64), "info": np.zeros(8, np.int64)}
    A.check(lib.cv_item_lines_host_form(_hp(text_h), len(text_h), max_lines, _hp(h["pos"]), _hp(h["run"]), _hp(h["off"]), _hp(h["len"]),
                                        _hp(h["tok"]), _hp(h["info"])))
    nrows, nruns = int(h["info"][2]), int(h["info"][5])
    assert np.array_equal(o["info"].get(), h["info"])
    for k in ("pos", "run", "off", "len"):
        assert np.array_equal(o[k].get(nrows), h[k][:nrows]), k
    assert np.array_equal(o["tok"].get(nruns), h["tok"][:nruns])
    return h


def test_item_lines_past_the_grid_stride_line(rows, rows_dev):
    """the rows' text as an item file: GRID_FOR + R lines in one slab of more than TILE_LINE bytes; the "0123" coordinates
    and the bytes past 0x7E are the HOST lines"""
    A, lib = _abi()
    assert len(rows.text) > TILE_LINE + 4096
    h = _item_lines(lib, A, rows.text, rows_dev[0], rows.n)
    info = h["info"].tolist()
    nhost = int(rows.item_host.sum())
    assert info[:3] == [len(rows.text), rows.n, rows.n - nhost] and info[4] == nhost
    ok = ~rows.item_host
    assert np.array_equal(h["pos"][:info[2]], rows.pos[ok]) and np.array_equal(h["off"][:info[2]], rows.row_off[:-1][ok])
    assert info[5] > len(rows.run_ctg) and rows.item_host[GRID_FOR:].any() and ok[GRID_FOR:].any()


def _truth_text():
    """GRID_FOR + R lines each of a BED file "ctg begin end" and of a truth list "ctg pos ref alt g1 g2"; a line with one
    token (HOST) and a blank line (SKIP) every few thousand lines, behind the line too"""
    rng = np.random.RandomState(103)
    n = GRID_FOR + R
    names = NAMES[:4]
    ctg, _run, _rc = _runs(rng, n, len(names), 2500)
    pool = _pool(rng, n // 8)
    pos = pool[rng.randint(0, len(pool), n)]
    nm, nl = _names_column(names, ctg)
    r = np.arange(n)
    one_token, blank = (r % 4099 == 17) | (r == n - 5), (r % 5003 == 19) | (r == n - 9)
    out = {}
    for fmt in ("bed", "var"):
        pm, pl = _decimal(pos)
        if fmt == "bed":
            em, el = _decimal(pos + rng.randint(0, 60, n))
            cols = [(nm, nl.copy()), (pm, pl), (em, el)]
        else:
            acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
            one = np.ones(n, dtype=np.int64)
            ref, alt = acgt[rng.randint(0, 4, (n, 1))], acgt[rng.randint(0, 4, (n, 3))]
            g = np.frombuffer(b"01", dtype=np.uint8)
            cols = [(nm, nl.copy()), (pm, pl), (ref, one), (alt, rng.randint(1, 4, n)), (g[rng.randint(0, 2, (n, 1))], one),
                    (g[rng.randint(0, 2, (n, 1))], one)]
        for _m, l in cols[1:]:
            l[one_token | blank] = 0
        cols[0][1][blank] = 0
        text, _ro, _co = _join_columns(cols)
        out[fmt] = text
    assert one_token[GRID_FOR:].any() and blank[GRID_FOR:].any() and _everything_behind(GRID_FOR, ctg)
    return out, n, int(one_token.sum()), int(blank.sum())


@pytest.fixture(scope="module")
def truth_text():
    return _truth_text()


@pytest.mark.parametrize("fmt", ["bed", "var"])
def test_truth_lines_past_the_grid_stride_line(truth_text, fmt):
    import torch
    A, lib = _abi()
    texts, n, n_one, n_blank = truth_text
    text_h = texts[fmt]
    code = 1 if fmt == "bed" else 0                              # CV_TRUTH_FORMAT_BED / _VAR
    text_d = _up(text_h)
    o = {"pos": Out(n, "int64"), "end": Out(n, "int64"), "label": Out(n, "float32", 16), "run": Out(n, "int32"), "tok": Out(n, "int64", 2),
         "info": Out(8, "int64")}
    ws, need = _workspace(lib.cv_truth_lines_workspace, len(text_h), n)
    A.check(lib.cv_truth_lines_dev(_p(text_d), len(text_h), code, None, 0, 0, 0, 0, n, o["pos"].p, o["end"].p if fmt == "bed" else None,
                                   None if fmt == "bed" else o["label"].p, o["run"].p, o["tok"].p, o["info"].p, _p(ws), need, _stream()))
    h = {"pos": np.zeros(n, np.int64), "end": np.zeros(n, np.int64), "label": np.zeros((n, 16), np.float32), "run": np.zeros(n, np.int32),
         "tok": np.zeros((n, 2), np.int64), "info": np.zeros(8, np.int64)}
    A.check(lib.cv_truth_lines_host_form(_hp(text_h), len(text_h), code, None, 0, 0, 0, 0, n, _hp(h["pos"]),
                                         _hp(h["end"]) if fmt == "bed" else None, None if fmt == "bed" else _hp(h["label"]), _hp(h["run"]),
                                         _hp(h["tok"]), _hp(h["info"])))
    info = h["info"].tolist()
    nrows, nruns = info[2], info[5]
    assert info[0] == len(text_h) and info[1] == n and nrows + info[3] + info[4] == n and info[3] > 0 and info[4] > 0 and nruns > 300
    assert np.array_equal(o["info"].get(), h["info"])
    for k in ("pos", "run", "end" if fmt == "bed" else "label"):
        assert np.array_equal(o[k].get(nrows), h[k][:nrows]), k
    assert np.array_equal(o["tok"].get(nruns), h["tok"][:nruns])
    if fmt == "var":
        assert len(np.unique(h["label"][:20000], axis=0)) > 8
    del text_d
    torch.cuda.empty_cache()


# ---- 3. the sorted tables (bt_end_keys, bt_begin_keys, bt_gather, bt_finish, tt_keys, tt_tails, tt_emit) ---------------------------
def _bed_definition(ctg, begin, end, nctg):
    """cv_bed_table_dev restated: per contig the intervals sorted by (begin, end), the running maximum of the ends"""
    order = np.lexsort((end, begin, ctg))
    c, b, e = ctg[order].astype(np.int64), begin[order], end[order]
    off = np.searchsorted(c, np.arange(nctg + 1)).astype(np.int64)
    lift = c * (1 << 41)                                         # a later contig starts above every earlier end
    emax = np.maximum.accumulate(e + lift) - lift
    return off, b, emax


def _truth_definition(ctg, pos, label, nctg, bed):
    """cv_truth_tables_dev restated: the LAST arrival of every (contig, pos) wins; those the BED keeps are the truth rows"""
    n = len(pos)
    order = np.lexsort((np.arange(n), pos, ctg))
    c, p = ctg[order].astype(np.int64), pos[order]
    tail = np.concatenate(((c[1:] != c[:-1]) | (p[1:] != p[:-1]), [True])) if n else np.zeros(0, bool)
    ec, ep, ei = c[tail], p[tail], order[tail]
    keep = _stab(bed[0], bed[1], bed[2], ec, ep, nctg) if bed is not None else np.ones(len(ep), bool)
    every_off = np.searchsorted(ec, np.arange(nctg + 1)).astype(np.int64)
    truth_off = np.searchsorted(ec[keep], np.arange(nctg + 1)).astype(np.int64)
    return truth_off, ep[keep], label[ei[keep]], every_off, ep


class Tables(object):
    def __init__(self, n, nctg, seed, run_ctg=None):
        rng = np.random.RandomState(seed)
        self.n, self.nctg = n, nctg
        if run_ctg is None:
            self.ctg, self.run, self.run_ctg = _runs(rng, n, nctg, 700)
        else:                                                     # one run per row
            self.run, self.run_ctg = np.arange(n, dtype=np.int32), np.array(run_ctg, dtype=np.int32)
            self.ctg = self.run_ctg
        pool = _pool(rng, max(n // 6, 16))
        self.begin = pool[rng.randint(0, len(pool), n)]
        self.end = self.begin + rng.randint(0, 3, n)             # (what the line pass leaves: int(end) - 1, never below begin)
        self.pos = pool[rng.randint(0, len(pool), n)]
        self.label = rng.randint(-4, 5, (n, 16)).astype(np.float32) * np.float32(0.25)


@pytest.fixture(scope="module")
def tables():
    return Tables(GRID_FOR + R, 7, 104)


def _bed_table_dev(T, run_ctg=None, nruns=None):
    A, lib = _abi()
    n, nctg = T.n, T.nctg
    run_ctg = T.run_ctg if run_ctg is None else run_ctg
    d = [_up(a) for a in (T.begin, T.end, T.run, run_ctg)]
    off, begin, emax = Out(nctg + 1, "int64"), Out(n, "int64"), Out(n, "int64")
    ws, need = _workspace(lib.cv_bed_table_workspace, n)
    A.check(lib.cv_bed_table_dev(n, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), len(run_ctg), nctg, off.p, begin.p, emax.p, _p(ws), need,
                                 _stream()))
    return off.get(), begin.get(), emax.get()


def _truth_tables_dev(T, bed, run_ctg=None):
    A, lib = _abi()
    n, nctg = T.n, T.nctg
    run_ctg = T.run_ctg if run_ctg is None else run_ctg
    d = [_up(a) for a in (T.pos, T.label, T.run, run_ctg)]
    b = [_up(a) for a in bed] if bed is not None else [None] * 3
    o = {"truth_off": Out(nctg + 1, "int64"), "truth_pos": Out(n, "int64"), "labels": Out(n, "float32", 16),
         "every_off": Out(nctg + 1, "int64"), "every_pos": Out(n, "int64"), "counts": Out(2, "int64")}
    ws, need = _workspace(lib.cv_truth_tables_workspace, n)
    A.check(lib.cv_truth_tables_dev(n, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), len(run_ctg), nctg, 1 if bed is not None else 0, _p(b[0]),
                                    _p(b[1]), _p(b[2]), o["truth_off"].p, o["truth_pos"].p, o["labels"].p, o["every_off"].p,
                                    o["every_pos"].p, o["counts"].p, _p(ws), need, _stream()))
    return o


def test_bed_table_past_the_grid_stride_line(tables):
    """two stable radix sorts and the max scan of GRID_FOR + R intervals: begins repeat (a quarter and more), so the order
    of the ends within one begin is the first sort's, kept by the second"""
    T = tables
    want = _bed_definition(T.ctg, T.begin, T.end, T.nctg)
    key = T.ctg.astype(np.int64) << 40 | T.begin
    assert T.n - len(np.unique(key)) > T.n // 4 and T.begin.max() > 1 << 32 and _everything_behind(GRID_FOR, T.ctg)
    got = _bed_table_dev(T)
    for g, w, name in zip(got, want, ("bed_off", "bed_begin", "bed_emax")):
        assert np.array_equal(g, w), name
    assert (want[2] != np.maximum.accumulate(want[2])).any()     # the running maximum starts again with each contig


def test_truth_tables_past_the_grid_stride_line(tables):
    """one stable sort over GRID_FOR + R truth rows; more than a quarter repeat an earlier (contig, pos) with another
    label, so the row that wins is the LAST arrival only if the sort is stable at this count"""
    T = tables
    bed = _bed_definition(T.ctg, T.begin, T.end + 1, T.nctg)
    want = _truth_definition(T.ctg, T.pos, T.label, T.nctg, bed)
    key = T.ctg.astype(np.int64) << 40 | T.pos
    assert T.n - len(np.unique(key)) > T.n // 4 and T.pos.max() > 1 << 32
    o = _truth_tables_dev(T, bed)
    nt, ne = len(want[1]), len(want[4])
    assert o["counts"].get().tolist() == [nt, ne] and 0 < nt < ne < T.n
    assert np.array_equal(o["truth_off"].get(), want[0]) and np.array_equal(o["every_off"].get(), want[3])
    assert np.array_equal(o["truth_pos"].get(nt), want[1]) and np.array_equal(o["every_pos"].get(ne), want[4])
    assert np.array_equal(o["labels"].get(nt).view(np.uint32), want[2].view(np.uint32))
    # the first arrival of a repeated key would have given other labels
    first = _truth_definition(T.ctg[::-1], T.pos[::-1], T.label[::-1], T.nctg, bed)
    assert np.array_equal(first[1], want[1]) and not np.array_equal(first[2], want[2])


def test_three_rows_over_65535_contigs():
    """the other way round: the second loop of bt_finish / tt_emit walks nctg + 1 = 65 536 offsets over n = 3 rows"""
    T = Tables(3, MAX_CONTIGS, 105, run_ctg=[40000, 7, MAX_CONTIGS - 1])
    T.pos[2] = T.begin[2]                                        # one truth row inside its contig's interval, two outside
    T.end = T.begin + 2
    T.pos[:2] = T.begin[:2] + 5
    want_bed = _bed_definition(T.ctg, T.begin, T.end, T.nctg)
    got = _bed_table_dev(T)
    for g, w, name in zip(got, want_bed, ("bed_off", "bed_begin", "bed_emax")):
        assert np.array_equal(g, w), name
    assert sorted(set(want_bed[0].tolist())) == [0, 1, 2, 3]
    for bed in (want_bed, None):
        want = _truth_definition(T.ctg, T.pos, T.label, T.nctg, bed)
        o = _truth_tables_dev(T, bed)
        nt = len(want[1])
        assert o["counts"].get().tolist() == [nt, 3] and nt == (1 if bed is not None else 3)
        assert np.array_equal(o["truth_off"].get(), want[0]) and np.array_equal(o["every_off"].get(), want[3])
        assert np.array_equal(o["truth_pos"].get(nt), want[1]) and np.array_equal(o["every_pos"].get(3), want[4])
        assert np.array_equal(o["labels"].get(nt), want[2])


# ---- 4. the BED filter of item lines and the sampler (ik_flags, ik_copy, sp_flags, sp_emit) -------------------------------------
def _keep_case(n, seed, want_text):
    """n rows of a slab against the rows' BED tables; with want_text, lines of 4 .. 200 bytes"""
    rng = np.random.RandomState(seed)
    pool = _pool(rng, 50000)
    bed = _per_contig_tables(rng, pool, NTAB, 0.5, True)
    ctg, run, run_ctg = _runs(rng, n, NTAB + 1, 900)
    run_ctg = np.where(run_ctg == NTAB, -1, run_ctg).astype(np.int32)      # a contig the BED lacks
    pos = pool[rng.randint(0, len(pool), n)]
    if want_text:
        llen = rng.randint(4, 201, n).astype(np.int64)
        off = np.concatenate(([0], np.cumsum(llen)))
        text = rng.randint(33, 127, int(off[-1])).astype(np.uint8)
        text[off[1:] - 1] = 10
        off = off[:-1].copy()
    else:
        llen, off, text = np.full(n, 9, dtype=np.int64), 9 * np.arange(n, dtype=np.int64), np.zeros(0, dtype=np.uint8)
    return {"n": n, "pos": pos, "run": run, "run_ctg": run_ctg, "off": off, "len": llen, "text": text, "bed": bed,
            "keep": _stab(bed[0], bed[1], bed[2], run_ctg[run], pos, NTAB)}


def _items_keep(c, want_text, lead=5):
    """cv_items_keep_dev against cv_items_keep_host_form (and against the numpy verdicts)"""
    A, lib = _abi()
    n, text = c["n"], c["text"]
    cols = [c["pos"], c["run"], c["off"], c["len"], c["run_ctg"]] + list(c["bed"])
    want_counts = np.full(4, -7, dtype=np.int64)
    cap = int(c["len"][c["keep"]].sum()) if want_text else 0
    want_out = np.full(cap + 1, 0xAB, dtype=np.uint8)
    A.check(lib.cv_items_keep_host_form(_hp(text) if len(text) else None, len(text), n, *[_hp(a) for a in cols[:5]], len(c["run_ctg"]), NTAB,
                                        *[_hp(a) for a in cols[5:]], want_text, _hp(want_out), cap, _hp(want_counts)))
    assert want_counts.tolist() == [n, int(c["keep"].sum()), cap, 0] and want_out[cap] == 0xAB
    d = [_up(a) for a in cols]
    td = _up(text) if len(text) else None
    room, counts = Out(lead + cap, "uint8"), Out(4, "int64")
    ws, need = _workspace(lib.cv_items_keep_workspace, n)
    A.check(lib.cv_items_keep_dev(_p(td), len(text), n, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), len(c["run_ctg"]), NTAB, _p(d[5]),
                                  _p(d[6]), _p(d[7]), want_text, ctypes.c_void_p(room.t.data_ptr() + lead) if cap else None, cap, counts.p,
                                  _p(ws), need, _stream()))
    assert np.array_equal(counts.get(), want_counts)
    got = room.get()
    assert (got[:lead] == 0xAB).all() and np.array_equal(got[lead:], want_out[:cap])


def test_items_keep_text_past_the_copy_line():
    """ik_copy, one wave per row, over COPY_LINE + R rows: behind the line kept and dropped lines alternate irregularly"""
    c = _keep_case(COPY_LINE + R, 106, True)
    k = c["keep"][COPY_LINE:]
    assert k.any() and not k.all() and len(np.flatnonzero(k[1:] != k[:-1])) > 10
    assert c["len"].min() == 4 and c["len"].max() == 200 and _everything_behind(COPY_LINE, c["run_ctg"][c["run"]])
    _items_keep(c, 1)


@pytest.mark.parametrize("trips", [1, 2])
def test_items_keep_counts_past_the_grid_stride_line(trips):
    """ik_flags sums its kept rows per lane, per block and per grid behind the loop: GRID_FOR + R rows, and 2 * GRID_FOR + R,
    where the lanes of one wave make two and three trips"""
    c = _keep_case(trips * GRID_FOR + R, 107 + trips, False)
    assert c["keep"][trips * GRID_FOR:].any() and 0.2 < c["keep"].mean() < 0.8
    _items_keep(c, 0)


def test_sample_positions_past_the_grid_stride_line():
    """sp_flags / sp_emit over a tile of GRID_FOR + R positions, the scan past its single tile; the draws are cv_draws_host"""
    A, lib = _abi()
    from clairvoyante_amd import draws
    rng = np.random.RandomState(110)
    count, first, seed, prob, h = GRID_FOR + R, (1 << 32) - 500000, 12345, 0.37, draws.fnv1a32("chr20")
    begin = np.sort(rng.choice(np.arange(first - 1000, first + count + 1000, 50), 9000, replace=False)).astype(np.int64)
    emax = np.maximum.accumulate(begin + rng.randint(0, 90, len(begin)))
    pos = first + np.arange(count, dtype=np.int64)
    u = np.zeros(count, dtype=np.float64)
    A.check(lib.cv_draws_host(seed, 2, h, _hp(pos), None, count, _hp(u)))
    k = np.searchsorted(begin, pos, side="right")
    for with_bed in (True, False):
        covered = (k > 0) & (emax[np.maximum(k - 1, 0)] > pos) if with_bed else np.ones(count, bool)
        want = pos[covered & (u <= prob)]
        assert len(want) > count // 20 and (want >= first + GRID_FOR).any() and want.max() > 1 << 32
        db, de = (_up(begin), _up(emax)) if with_bed else (None, None)
        ws, need = _workspace(lib.cv_sample_positions_workspace, count)
        for cap in (len(want), len(want) - R):
            out, cnt = Out(cap, "int64"), Out(2, "int64")
            A.check(lib.cv_sample_positions_dev(seed, h, first, count, prob, len(begin) if with_bed else 0, _p(db), _p(de), out.p, cap, cnt.p,
                                                _p(ws), need, _stream()))
            assert cnt.get().tolist() == [cap, len(want)]
            assert np.array_equal(out.get(), want[:cap])


# ---- 5. the pairing (bt_pair_count, bt_pair_keep) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("trips", [1, 2])
def test_bamtrain_pair_past_the_grid_stride_line(trips):
    """both kernels add up per lane over the loop and per wave behind it (a shuffle tree): GRID_FOR + R rows, and
    2 * GRID_FOR + R, where the lanes of one wave make two and three trips"""
    A, lib = _abi()
    from clairvoyante_amd import draws
    rng = np.random.RandomState(111 + trips)
    n, seed, amp = trips * GRID_FOR + R, 777, 2.0
    names = ("chr1", "chr2", "chrX")
    hashes = np.array([draws.fnv1a32(s) for s in names], dtype=np.uint32)
    ctg, _run, _rc = _runs(rng, n, len(names), 5000)
    pos = rng.randint(1, 1 << 40, n).astype(np.int64)
    flags = (rng.random_sample(n) < 0.12).astype(np.uint8) | (2 * (rng.random_sample(n) < 0.5)).astype(np.uint8)
    acgt = (rng.random_sample(n) < 0.97).astype(np.uint8)
    flags[n - R:], acgt[n - R + 3::9] = np.arange(R) % 4, 0             # (every kind among the R rows behind the line)
    bed = rng.random_sample(n) < 0.7
    truth = (flags & 1) != 0
    v, c = int(truth.sum()), int((~truth & bed).sum())
    ratio = min(1.0, (float(v) * amp) / float(c))
    u = np.zeros(n, dtype=np.float64)
    for k in range(len(names)):
        m = np.flatnonzero(ctg == k)
        pk, uk = np.ascontiguousarray(pos[m]), np.zeros(len(m), dtype=np.float64)
        A.check(lib.cv_draws_host(seed, 1, int(hashes[k]), _hp(pk), None, len(m), _hp(uk)))
        u[m] = uk
    picked = ~truth & bed & (u < ratio)
    want = ((truth & bed) | picked) & (acgt != 0)
    assert 0.05 < ratio < 0.95 and picked[trips * GRID_FOR:].any() and _everything_behind(trips * GRID_FOR, ctg, flags, acgt, want)
    d = [_up(a) for a in (ctg, pos, flags, acgt, hashes)]
    keep, counts, r = Out(n, "uint8"), Out(4, "int64"), Out(1, "float64")
    keep.t[:n] = _up(bed.astype(np.uint8))
    A.check(lib.cv_bamtrain_pair(n, _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), len(names), seed, amp, keep.p, counts.p, r.p, _stream()))
    assert counts.get().tolist() == [v, c, int(picked.sum()), int(want.sum())]
    assert r.get()[0] == ratio
    assert np.array_equal(keep.get().astype(bool), want)


# ---- 6. the candidate list (candorder_flag, candorder_place, candrows_len) ----------------------------------------------------------
def test_candidate_order_and_rows_past_the_grid_stride_line():
    """the stable partition of GRID_FOR + R selected entries and the length pass over as many rows, against numpy and
    cv_candidate_rows_host_form; rows of both verdicts and entries of both parts of the order lie behind the line"""
    import candlist_cases as cc
    A, lib = _abi()
    rng = np.random.RandomState(120)
    n = GRID_FOR + R
    pos0 = np.sort(rng.randint(0, n, n)).astype(np.int64)
    late = np.concatenate(([0], pos0[1:] == pos0[:-1])).astype(np.int32)
    last_pos = int(pos0[n - 40])
    head = (late == 0) & (pos0 < last_pos)
    want_order = np.concatenate((np.flatnonzero(head), np.flatnonzero(~head))).astype(np.int64)
    assert head[GRID_FOR:].any() and not head[GRID_FOR:].all() and 0.3 < head.mean() < 0.9
    d_pos, d_late = _up(pos0), _up(late)
    order = Out(n, "int64")
    ws, need = _workspace(lib.cv_candidate_order_workspace, n)
    A.check(lib.cv_candidate_order_dev(_p(d_pos), _p(d_late), n, last_pos, order.p, _p(ws), need, _stream()))
    assert np.array_equal(order.get(), want_order)
    ref = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.randint(0, 9, n + 64)].copy()
    ref[rng.randint(0, n, 2000)] = 0x80                          # rows for the host
    ref[pos0[want_order[n - 9]]] = 0x80
    c7 = rng.randint(0, 60, (n, 7)).astype(np.int32)
    c7[rng.randint(0, n, 2000), 2] = -1                          # rows for the host
    want_text, want_off, want_status = cc.host_form(b"chr21", want_order, pos0, c7, ref.tobytes(), 0)
    assert 0 < want_status.sum() < n // 50 and want_status[GRID_FOR:].any() and not want_status[GRID_FOR:].all()
    d_c7, d_ref, d_order = _up(c7), _up(ref), _up(want_order)
    off, status, lead = Out(n + 1, "int64"), Out(n, "uint8"), 5
    text = Out(lead + len(want_text), "uint8")
    ws, need = _workspace(lib.cv_candidate_rows_workspace, n)
    A.check(lib.cv_candidate_rows_dev(b"chr21", 5, _p(d_order), n, n, _p(d_pos), None, _p(d_c7), _p(d_ref), 0, len(ref), off.p, status.p,
                                      ctypes.c_void_p(text.t.data_ptr() + lead), len(want_text), _p(ws), need, _stream()))
    assert np.array_equal(off.get(), want_off) and np.array_equal(status.get(), want_status)
    got = text.get()
    assert (got[:lead] == 0xAB).all() and got[lead:].tobytes() == want_text


# ---- 7. the text rows (tp_count_newlines, tp_line_ends, tp_parse_rows) -----------------------------------------------------------------
@pytest.fixture(scope="module")
def producer_rows():
    """64 distinct rows in the producer's format without their first two tokens, and one whose centre base is N"""
    import textparse_cases as T
    rng = np.random.RandomState(112)
    vocab = T._vocabulary()
    tails = [T.good_row(rng, vocab, i).split(" ", 2)[2].encode() for i in range(64)]
    seq = b"ACGTACGTACGTACGTNACGTACGTACGTACGT"
    dropped = T.good_row(rng, vocab, 0, seq=seq.decode()).split(" ", 2)[2].encode()
    return tails, dropped


@pytest.mark.parametrize("trips", [1, 2])
def test_parse_rows_past_the_parse_line(producer_rows, trips):
    """one call over trips * PARSE_LINE + R ordinary lines, then a line for the host, then one whose centre base drops it:
    every wave of tp_parse_rows makes trips + 1 trips with its LDS line and row, its n_row / n_host counters cover all of
    them, and the slab (more than TILE_LINE bytes) takes the two index kernels past their 2 048 tiles"""
    import torch
    import textparse_cases as T
    A, lib = _abi()
    tails, dropped = producer_rows
    k = trips * PARSE_LINE + R
    lines = [b"chr%d %d %s" % (i % 3, 1000 + 7 * i, tails[(i * 37) % 64]) for i in range(k)]
    lines.append(b"chr1\t5\t" + tails[0])                         # tabs: not the producer's format
    lines.append(b"chr2 %d %s" % (1000 + 7 * k, dropped))
    text = b"\n".join(lines) + b"\n"
    n = k + 2
    assert len(text) > TILE_LINE + 4096
    buf = torch.full((len(text) + 64,), 10, dtype=torch.uint8, device="cuda")
    buf[3:3 + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    x, meta, status, info = Out(n, "float32", 528), Out(n, "int64", 6), Out(n, "uint8"), Out(4, "int64")
    ws, need = _workspace(lib.cv_parse_tensor_text_dev_workspace, len(text), n)
    A.check(lib.cv_parse_tensor_text_dev(ctypes.c_void_p(buf.data_ptr() + 3), len(text), n, x.p, meta.p, status.p, info.p, _p(ws), need,
                                         _stream()))
    assert info.get().tolist() == [len(text), n, k, 1]
    st = status.get()
    assert (st[:k] == T.ROW).all() and st[k] == T.HOST and st[k + 1] == T.SKIP
    body = b"\n".join(lines[:k]) + b"\n"
    hc, bad, hx, hmeta = T.host_parse(body)
    assert (hc, bad, len(hx)) == (len(body), 0, k)
    gx, gm = x.get(), meta.get()
    assert np.array_equal(gx[:k].view(np.uint32), hx.view(np.uint32)) and np.array_equal(gm[:k], hmeta)
    assert np.isnan(gx[k:]).all() and (gm[k:] == SENTINEL["int64"]).all()        # neither the host's line nor the dropped one wrote a row
    del buf
    torch.cuda.empty_cache()


# ---- 8. the decoders (gzip_find, gzip_decode, gzip_rest, blosc_decode) ---------------------------------------------------------------
def test_one_gzip_slab_past_the_find_and_decode_lines():
    """one raw DEFLATE stream of GZIP_LINE + R dynamic blocks, each closed by a full flush, so every block starts on a
    byte the test knows: cv_gzip_find_dev with guesses of 64 bytes (three times GZIP_LINE of them), then
    cv_gzip_decode_dev with one chunk per block, counting and writing.  Every wave of both kernels takes a second and a
    third item with the LDS state of the one before.  (Every chunk is shorter than the window: resolving is the test
    below.)"""
    import zlib
    A, lib = _abi()
    rng = np.random.RandomState(130)
    vals = np.array([b"0.0", b"1.0", b"12.0", b"3.0", b"104.0", b"-23.0", b"57.0", b"8.0", b"0.0", b"0.0"], dtype=object)
    blocks = GZIP_LINE + R
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    lines = [b"chr%d %d " % (i % 3, 1000 + i) + b" ".join(vals[rng.randint(0, 10, 150 + i % 50)]) + b"\n" for i in range(blocks)]
    parts = [z.compress(l) + z.flush(zlib.Z_FULL_FLUSH) for l in lines] + [z.flush(zlib.Z_FINISH)]
    comp = np.frombuffer(b"".join(parts), dtype=np.uint8)
    start = 8 * np.concatenate(([0], np.cumsum([len(q) for q in parts[:blocks]])))[:blocks].astype(np.int64)
    assert ((comp[start // 8] >> 1) & 3 == 2).all()              # BTYPE 10: every block is a dynamic one
    nb, spacing = len(comp), 64
    guesses = -(-nb // spacing)
    assert guesses > 2 * GZIP_LINE + R
    d_comp = _up(np.concatenate((comp, np.zeros(8, dtype=np.uint8))))
    found = Out(guesses, "int64")
    A.check(lib.cv_gzip_find_dev(_p(d_comp), nb, 0, spacing, guesses, found.p, _stream()))
    got = found.get()
    # the first block start inside each guess's bits (bit 0 belongs to no guess); a header in front of it that is none
    # of the blocks' is a decoy the finder has to report as well: the host's header test says so
    g_of = start[1:] // (8 * spacing)
    want = np.full(guesses, -1, dtype=np.int64)
    want[g_of[::-1]] = start[1:][::-1]
    odd = np.flatnonzero(got != want)
    assert len(odd) < 8
    for g in odd.tolist():
        assert 8 * spacing * g <= got[g] < (want[g] if want[g] >= 0 else 8 * spacing * (g + 1))
        assert lib.cv_gzip_header_at(comp.ctypes.data_as(ctypes.c_void_p), nb, int(got[g])) == 1
    assert (want[GZIP_LINE:] >= 0).sum() > GZIP_LINE // 4
    # one chunk per block: the counting pass, then the writing pass
    lens = np.array([len(l) for l in lines], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(lens)))
    total = int(off[-1])
    rows = np.zeros((blocks, 6), dtype=np.int64)
    rows[:, 0], rows[:, 1], rows[:, 4] = start, np.append(start[1:], -1), WSIZE
    rows[0, 4] = 0
    want_res = np.stack([lens, np.append(start[1:], 0), np.full(blocks, 1), np.zeros(blocks, dtype=np.int64)], axis=1)
    want_res[-1, 2] = 2                                           # CV_GZIP_LANDED, the last chunk CV_GZIP_FINAL
    text = np.frombuffer(b"".join(lines), dtype=np.uint8)
    for write in (False, True):
        if write:
            rows[:, 2], rows[:, 3] = off[:-1], lens
        d_rows = _up(rows)
        res, sym = Out(blocks, "int64", 4), Out(total, "int16")
        A.check(lib.cv_gzip_decode_dev(_p(d_comp), nb, _p(d_rows), blocks, sym.p if write else None, total if write else 0, res.p,
                                       _stream()))
        r = res.get()
        assert start[-1] < r[-1, 1] <= 8 * nb
        r[-1, 1] = 0
        assert np.array_equal(r, want_res)
        assert np.array_equal(sym.get(total if write else 0), text.astype(np.int16) if write else np.zeros(0, dtype=np.int16))


def test_gzip_resolve_past_the_rest_line():
    """cv_gzip_resolve_dev over GZIP_REST_LINE + 300 000 + R symbols in chunks of 20 000 .. 400 000: what a chunk holds in
    front of its last 32 KiB is gzip_rest's (a binary search over the chunk offsets per symbol, several trips per thread),
    its last 32 KiB gzip_tails'.  A third of the symbols are markers into the 32 KiB in front of their chunk, in chunk 0
    into the caller's window; the reference resolves chunk after chunk with numpy"""
    A, lib = _abi()
    rng = np.random.RandomState(131)
    total, hist = GZIP_REST_LINE + 300000 + R, 5000
    lens = [100000]
    while sum(lens) < total:
        lens.append(int(rng.choice((20000, 31000, 90000, 250000, 400000))) + int(rng.randint(0, 999)))
    lens[-1] -= sum(lens) - total
    assert lens[-1] > 0
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    chunks = len(lens)
    sym = rng.randint(0, 256, total).astype(np.uint16)
    marker = rng.random_sample(total) < 0.33
    j = rng.randint(0, WSIZE, total)
    j[:lens[0]] = rng.randint(WSIZE - hist, WSIZE, lens[0])       # chunk 0 reaches into the window only
    sym[marker] = (MARK | j[marker]).astype(np.uint16)
    window = rng.randint(0, 256, hist).astype(np.uint8)
    full = np.concatenate((window, np.zeros(total, dtype=np.uint8)))
    for c in range(chunks):                                        # (a marker names a byte in front of its chunk: final by then)
        lo, hi = int(off[c]), int(off[c + 1])
        s_c, m_c = sym[lo:hi], marker[lo:hi]
        out = s_c.astype(np.uint8)
        out[m_c] = full[hist + lo - WSIZE + j[lo:hi][m_c]]
        full[hist + lo:hist + hi] = out
    want = full[hist:]
    # the symbols that are gzip_rest's, and those of them behind the line
    chunk_of = np.repeat(np.arange(chunks), lens)
    rest = np.arange(total) < off[1:][chunk_of] - WSIZE
    assert rest[GZIP_REST_LINE:].sum() > 100000 and (rest & marker)[GZIP_REST_LINE:].any() and min(lens) < WSIZE < max(lens)
    assert int(np.maximum(np.array(lens) - WSIZE, 0).sum()) == int(rest.sum()) > GZIP_REST_LINE // 2
    lead = 64 + hist
    text = Out(lead + total, "uint8")
    text.t[64:lead] = _up(window)
    bad = Out(1, "int32")
    bad.t[0] = 0
    d_sym, d_off = _up(sym.view(np.int16)), _up(off)
    A.check(lib.cv_gzip_resolve_dev(_p(d_sym), _p(d_off), chunks, total, hist, ctypes.c_void_p(text.t.data_ptr() + lead), bad.p, _stream()))
    got = text.get()
    assert (got[:64] == 0xAB).all() and np.array_equal(got[64:lead], window)
    assert np.array_equal(got[lead:], want)
    assert bad.get()[0] == 0


def test_blosc_streams_past_the_decode_line():
    """more than BLOSC_LINE streams in one cv_blosc_decode_dev call: blocks of 1 KiB, four byte planes each"""
    import test_gpu_blosc as TB
    import blosc_cases as B
    from clairvoyante_amd import utils_v2
    x, _y = B.candidates(40, seed=7)
    block_bytes = x[:8].nbytes
    one = utils_v2.pack_array(x[:8], 1024)
    per = len(TB.device_unpack([one], block_bytes)[3])
    count = -(-(BLOSC_LINE + R) // per)
    made = {}
    chunks = [made.setdefault(k % 32, utils_v2.pack_array(x[k % 32:k % 32 + 8], 1024)) for k in range(count)]
    chunks.append(utils_v2.pack_array(x[:3], 1024))
    hs, hl, ho = TB.host_unpack(chunks, block_bytes)
    assert not hs.any()
    ds, dl, do, sstat, planned, intact = TB.device_unpack(chunks, block_bytes)
    assert BLOSC_LINE + R <= len(sstat) < BLOSC_LINE + R + 2 * per
    assert intact and planned.all() and np.all(sstat == B.OK)
    assert list(ds) == list(hs) and list(dl) == list(hl) and do == ho


# ---- 9. the packer and the BAM walk (pack_encode, pack_assemble, bam_gather) -------------------------------------------------------
def test_blosc_pack_past_the_stream_line():
    """PACK_LINE + 104 streams in one cv_blosc_pack_dev call: 29 130 one-row chunks in blocks of 64 bytes, 36 streams each,
    so the blocks of pack_encode (whose LDS state serves a second stream) and of pack_assemble make a second trip.  The
    chunks of a call do not depend on one another: the rows are 32 distinct ones in turn, the host form runs once over
    those, and the expected call is its chunks repeated"""
    import torch
    import test_gpu_blosc_pack as TP
    from clairvoyante_amd import utils_v2
    head, tail = utils_v2.pickle_envelope((1,) + TP.SHAPE, np.float32)
    per = -(-(len(head) + TP.ROW + len(tail)) // 64)
    chunks = -(-(PACK_LINE + R) // per)
    assert (chunks - 1) * per < PACK_LINE + R <= chunks * per and chunks <= 65535
    rng = np.random.RandomState(140)
    base = np.zeros((32,) + TP.SHAPE, np.float32)
    base[1::4] = 3.0
    base[2::4] = rng.randint(0, 40, (8,) + TP.SHAPE).astype(np.float32)
    base[3::4] = rng.randint(0, 1 << 32, size=(8,) + TP.SHAPE, dtype=np.uint64).astype(np.uint32).view(np.float32)
    distinct = TP.host_form(base, 0, 32, 1, 64)
    assert any(w is None for w in distinct) and len({len(w) for w in distinct if w is not None}) > 3
    x = np.ascontiguousarray(base[np.arange(chunks) % 32])
    got = TP.device_form(torch.from_numpy(x).cuda(), 0, chunks, 1, 64)         # (sentinels around and behind every buffer)
    want = [distinct[k % 32] for k in range(chunks)]
    assert got == want


def test_one_bam_slab_past_the_walker_line(tmp_path):
    """WALK_LINE + R reads, one in each 16 384-base window of a 68 Mbp contig: the linear index gives the slab a walker
    per window, so the blocks of bam_gather take a second walker; host route and device route give the same pileup"""
    import bam_device_cases as C
    import test_gpu_bam_device as TB
    rng = np.random.RandomState(141)
    nreads = WALK_LINE + R
    unit = "".join("ACGT"[k] for k in rng.randint(0, 4, 16384))
    ref = unit * (nreads + 1)
    lines, centers = [], []
    for w in range(nreads):
        pos1 = w * 16384 + 200 + (w * 37) % 9000                  # 1-based POS
        seq = list(ref[pos1 - 1:pos1 - 1 + 60])
        seq[30] = "ACGT"[("ACGT".index(seq[30]) + 1 + w % 3) % 4]
        lines.append("r%05d\t0\tctgA\t%d\t60\t60M\t*\t0\t0\t%s\t*" % (w, pos1, "".join(seq)))
        centers += [pos1 + 30, pos1 + 41]
    bam = str(tmp_path / "wide.bam")
    C.write_bam(bam, lines, [("ctgA", len(ref)), ("zzz", 50)])
    h, d, cnt = TB.both(bam, ref, centers=np.array(centers), dcov=250)
    TB.clean(cnt)
    assert cnt["walkers"] > WALK_LINE + R - 2 and cnt["device_slabs"] == 1
    assert h[4] == nreads and h[3].all() and h[1].any()


# ---- 10. the VCF merge (vm_fields, vm_sorted, vm_gather, vm_heads, vm_chunks, vm_chunk_out, vw_fill, vw_min, vw_backfill) --------
def _merge_call(a, phase=0):
    """cv_vcf_merge_dev + cv_vcf_windows_dev over the arrays of vcf_merge_big_cases, the output text at `phase` mod 16
    -> dict like vcf_merge_cases.host_form's; what lies behind the used part of an output still holds its sentinel"""
    A, lib = _abi()
    n, nrank, n_text = a["n"], a["nrank"], a["n_text"]
    text, pos, run, off, ln, rr = (_up(a[k]) for k in ("text", "pos", "run", "off", "len", "run_rank"))
    assert text.data_ptr() % 16 == 0 and len(a["text"]) == n_text + 16
    o = {"srank": Out(n, "int32"), "sbeg": Out(n, "int64"), "send": Out(n, "int64"), "ooff": Out(n + 1, "int64"),
         "text": Out(n_text + 16, "uint8"), "chunks": Out(4 * n, "int64"), "stats": Out(4 * nrank, "int64"), "info": Out(8, "int64")}
    shift = (phase - o["text"].t.data_ptr()) % 16
    ws, need = _workspace(lib.cv_vcf_merge_workspace, n)
    assert max(need, 32 * n, n_text) <= TEST_BYTES
    A.check(lib.cv_vcf_merge_dev(_p(text), n_text, n, _p(pos), _p(run), _p(off), _p(ln), _p(rr), a["nruns"], nrank, o["srank"].p, o["sbeg"].p,
                                 o["send"].p, o["ooff"].p, ctypes.c_void_p(o["text"].t.data_ptr() + shift), n_text, o["chunks"].p,
                                 o["stats"].p, o["info"].p, _p(ws), need, _stream()))
    g = {k: v.get() for k, v in o.items() if k != "text"}
    nbytes, nc = int(g["info"][2]), int(g["info"][1])
    full = o["text"].get(shift + nbytes)                            # (asserts the sentinel behind the text's last byte)
    assert (full[:shift] == SENTINEL["uint8"]).all()
    g["text"] = full[shift:]
    g["chunks"], g["stats"] = g["chunks"].reshape(4, n), g["stats"].reshape(4, nrank)
    assert (g["chunks"][:, nc:] == SENTINEL["int64"]).all()
    count, maxend = g["stats"][2], g["stats"][3]
    g["win_off"] = np.concatenate(([0], np.cumsum(np.where(count > 0, ((maxend - 1) >> 14) + 1, 0)))).astype(np.int64)
    nwin = int(g["win_off"][-1])
    win, d_off = Out(nwin, "int64"), _up(g["win_off"])
    A.check(lib.cv_vcf_windows_dev(n, o["srank"].p, o["sbeg"].p, o["send"].p, o["ooff"].p, nrank, _p(d_off), win.p, nwin, _stream()))
    g["win"] = win.get()
    return g


def _merge_same(g, w, a):
    """every output of the two entry points against the host forms': what _same of test_gpu_vcf_merge.py compares"""
    n, nc, nwin, nbytes = a["n"], int(w["info"][1]), int(w["win_off"][-1]), int(w["info"][2])
    assert g["info"].tolist() == w["info"].tolist()
    for k in ("srank", "sbeg", "send"):
        assert np.array_equal(g[k], w[k][:n]), k
    assert np.array_equal(g["ooff"], w["ooff"]) and np.array_equal(g["stats"], w["stats"]) and np.array_equal(g["win_off"], w["win_off"])
    assert np.array_equal(g["chunks"][:, :nc], w["chunks"][:, :nc])
    assert len(g["win"]) == nwin and np.array_equal(g["win"], w["win"][:nwin])
    assert len(g["text"]) == nbytes <= a["n_text"] and np.array_equal(g["text"], w["text"][:nbytes])


def test_vcf_merge_past_the_grid_stride_line():
    """GRID_FOR + R unique lines of eight sorted files laid end to end, over 1 100 contig ranks (vw_backfill's blocks take a
    second contig), 33 of which reach 2^29 (1 162 900 windows: vw_fill strides), 83 430 chunks, four in ten of the records
    tied with a record of another run, one key 5 002 times: only a stable sort gives the host form's order.
    Then the same with one line among the last R that the device does not vouch for"""
    import vcf_merge_big_cases as B
    import vcf_merge_cases as vc
    a, _facts = B.merge_case()
    assert a["n"] == GRID_FOR + R and a["nrank"] > BACKFILL_LINE
    w = vc.host_form(a)
    assert int(w["win_off"][-1]) > GRID_FOR and w["info"][0] == 0
    _merge_same(_merge_call(a), w, a)
    b, facts = B.merge_case(with_end=True)
    assert facts["end_at"] >= GRID_FOR
    wb = vc.host_form(b)
    assert wb["info"][0] == 1
    _merge_same(_merge_call(b, phase=9), wb, b)


def test_vcf_gather_past_the_tile_line():
    """MERGE_TILE_LINE + R records of 20 to 30 bytes: 65 538 tiles, so blocks 0 and 1 of vm_gather write their LDS tile a
    second time, the last tile holds 13 records, and the output stands at phase 5 (granule stores and end bytes).  The
    CV_GRID_STRIDE kernels make four trips and a ragged fifth"""
    import vcf_merge_big_cases as B
    import vcf_merge_cases as vc
    a = B.gather_case()
    assert a["n"] == MERGE_TILE_LINE + R and -(-a["n"] // 64) == 65536 + 2 and a["n"] % 64 == 13
    _merge_same(_merge_call(a, phase=5), vc.host_form(a), a)


def test_vcf_merge_rank_widths():
    """the sort keys are POS_BITS + bits_for(nrank) and 16 + bits_for(nrank + 1) bits wide: records in the lowest and the
    highest rank, either side of every power of two the widths turn at, up to MAX_RANKS; one more is refused"""
    import vcf_merge_big_cases as B
    import vcf_merge_cases as vc
    A, _lib = _abi()
    for nrank in B.RANK_COUNTS:
        a = B.rank_case(nrank)
        w = vc.host_form(a)
        assert w["srank"][a["n"] - 1] == nrank - 1 and w["sbeg"][a["n"] - 1] == (1 << 29) - 1
        _merge_same(_merge_call(a, phase=nrank % 16), w, a)
    a = dict(B.rank_case(B.MAX_RANKS), nrank=B.MAX_RANKS + 1)
    with pytest.raises(A.CvError, match="contig ranks"):
        vc.host_form(a)
    with pytest.raises(A.CvError, match="contig ranks"):
        _merge_call(a)

