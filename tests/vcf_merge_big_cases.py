"""Inputs of the VCF merge's launch-cap, tile-line, rank-width and 4 GiB tests, as the arrays the C ABI takes (what
vcf_merge_cases.line_arrays makes of files): built with numpy from fixed-width byte templates, no Python loop over records.
tests/test_vcf_merge_big_cases_host.py asserts on the CPU what every case here claims about itself."""
import numpy as np

import vcf_merge_cases as vc

GRID_FOR = 4096 * 256              # csrc/cv_dev_common.hpp, cv_grid_for
GATHER_LINE = 65536 * 64           # csrc/cv_vcfmerge_dev.hip, vm_gather: 65 536 one-wave blocks x 64 records
BACKFILL_LINE = 1024               # csrc/cv_vcfmerge_dev.hip, vw_backfill: 1 024 blocks, one contig rank each
TILE_TEXT = 16 * 1024              # csrc/cv_vcfmerge_core.hpp
LINE_CAP = 8192
MAX_RANKS = 1 << 20
MAX_END = 1 << 29
R = 77


def aligned_text(nbytes):
    """a zeroed uint8 array of nbytes + 16 spare bytes whose first byte is 16-byte aligned"""
    raw = np.zeros(nbytes + 48, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + nbytes + 16]


def put_decimal(mat, at, width, values):
    """values, zero-padded to `width` digits, into the columns at .. at + width of every row of mat"""
    v = np.asarray(values, dtype=np.int64)
    for k in range(width):
        mat[:, at + k] = (v // 10 ** (width - 1 - k)) % 10 + 48


def runs_of(rank):
    """the runs of consecutive equal contigs, as the item line pass numbers them -> (run per record, rank per run)"""
    start = np.concatenate(([True], rank[1:] != rank[:-1]))
    return (np.cumsum(start) - 1).astype(np.int32), rank[start].astype(np.int32)


def arrays(text, n_text, rank, pos, off, length, nrank):
    run, run_rank = runs_of(rank) if len(rank) else (np.zeros(0, np.int32), np.zeros(1, np.int32))
    return {"text": text, "n_text": int(n_text), "n": len(rank), "pos": np.ascontiguousarray(pos, dtype=np.int64), "run": run,
            "off": np.ascontiguousarray(off, dtype=np.int64), "len": np.ascontiguousarray(length, dtype=np.int64), "run_rank": run_rank,
            "nruns": len(run_rank) if len(rank) else 0, "nrank": int(nrank), "rank": np.asarray(rank, dtype=np.int64)}


def expected_order(a):
    """the permutation the merge must find: by (rank, POS), input order on a tie -- numpy's, not the code under test's"""
    return np.lexsort((np.arange(a["n"]), a["pos"], a["rank"]))


# ---- 1. GRID_FOR + 77 records over 1 100 contig ranks ---------------------------------------------------------------------------
# three templates of one length: REF of one base, REF of five bases (straddles windows and bins), and a line with END=
T_ONE = b"c0000\t000000000\tid0000000xxxx\tA\tC\t30\tPASS\t.\tGT\t0/1\n"
T_FIVE = b"c0000\t000000000\tid0000000\tACGTA\tA\t30\tPASS\t.\tGT\t1/1\n"
T_END = b"c0000\t000000000\tid0000000\tA\tC\t30\tPASS\tEND=9\tGT\t0/1\n"
assert len(T_ONE) == len(T_FIVE) == len(T_END) == 51
MERGE_NRANK, MERGE_FILES, FAR_RANKS, TIE_RUN = 1100, 8, 33, 5000


def merge_case(with_end=False):
    """n = GRID_FOR + 77 unique lines: eight files, each sorted by (rank, POS), laid end to end, and a ninth of 77 lines.
    -> (arrays, facts) where facts name what was planted"""
    rng = np.random.RandomState(151)
    n, body = GRID_FOR + R, GRID_FOR
    ranks = np.sort(rng.choice(MERGE_NRANK, 701, replace=False))
    new_rank, used = int(ranks[350]), np.delete(ranks, 350)              # new_rank: only among the last 77
    far = used[rng.choice(len(used), FAR_RANKS, replace=False)]
    rank = used[rng.randint(0, len(used), body)]
    dense = rng.random_sample(body) < 0.7
    pos = np.where(dense, rng.randint(1, 1000, body), rng.randint(1, 2000000, body)).astype(np.int64)
    five = rng.random_sample(body) < 1.0 / 16
    tie_rank, tie_pos = int(used[5]), 777
    tied = rng.choice(body, TIE_RUN, replace=False)                       # one (rank, POS) 5 000 times, over all files
    rank[tied], pos[tied] = tie_rank, tie_pos
    at = rng.choice(np.setdiff1d(np.arange(body), tied), FAR_RANKS, replace=False)
    rank[at], pos[at], five[at] = far, MAX_END, False                     # end = 2^29: the last window a .tbi addresses
    file_of = rng.randint(0, MERGE_FILES, body)
    order = np.lexsort((pos, rank, np.array([5, 2, 7, 0, 3, 6, 1, 4])[file_of]))
    rank, pos, five, file_of = rank[order], pos[order], five[order], file_of[order]
    # the 77 behind the line: a new contig, run starts, a tie with a record in front of the line, a window straddler
    t_rank = used[(np.arange(R) // 5 * 37) % len(used)]
    t_pos = rng.randint(1, 200000, R).astype(np.int64)
    t_five = np.zeros(R, dtype=bool)
    t_rank[10:13] = new_rank
    t_rank[20], t_pos[20] = tie_rank, tie_pos                             # behind 5 000 records of the same key
    t_rank[30], t_pos[30] = rank[12345], pos[12345]
    t_pos[40], t_five[40] = 16383, True                                   # [16 382, 16 387): windows 0 and 1
    rank, pos, five = np.concatenate((rank, t_rank)), np.concatenate((pos, t_pos)), np.concatenate((five, t_five))
    width = len(T_ONE)
    text = aligned_text(n * width)
    mat = text[:n * width].reshape(n, width)
    mat[:] = np.frombuffer(T_ONE, dtype=np.uint8)
    mat[five] = np.frombuffer(T_FIVE, dtype=np.uint8)
    end_at = body + 50
    if with_end:
        mat[end_at] = np.frombuffer(T_END, dtype=np.uint8)
    put_decimal(mat, 1, 4, rank)
    put_decimal(mat, 6, 9, pos)
    put_decimal(mat, 18, 7, np.arange(n))
    a = arrays(text, n * width, rank, pos, np.arange(n, dtype=np.int64) * width, np.full(n, width, dtype=np.int64), MERGE_NRANK)
    facts = {"body": body, "file_of": file_of, "new_rank": new_rank, "far": far, "tie": (tie_rank, tie_pos), "five": five,
             "end_at": end_at if with_end else None, "used": used, "width": width}
    return a, facts


def tie_share(a):
    """the share of records whose (rank, POS) a record of ANOTHER run has too, and the longest stretch of one key"""
    key = a["rank"] * (1 << 40) + a["pos"]
    order = np.lexsort((a["run"], key))
    k, r = key[order], a["run"][order]
    head = np.concatenate(([True], k[1:] != k[:-1]))
    group = np.cumsum(head) - 1
    first_run, last_run = r[head], r[np.concatenate((head[1:], [True]))]
    mixed = (first_run != last_run)[group]                                # (runs ascend inside a group: first != last = two runs)
    return float(mixed.mean()), int(np.bincount(group).max())


# ---- 2. GATHER_LINE + 77 minimal records of 20 to 30 bytes ------------------------------------------------------------------------
def gather_case():
    """c TAB 5-digit POS TAB . TAB REF(1 .. 11) TAB C TAB . TAB . TAB . NL: 20 + (len(REF) - 1) bytes; eight stretches
    ("files") of one contig each, sorted by POS, laid end to end out of rank order; three ranks, about 14 records per key"""
    rng = np.random.RandomState(152)
    n = GATHER_LINE + R
    reflen = rng.randint(1, 12, n)
    per = -(-n // 8)
    rank = np.array([2, 0, 1, 0, 2, 1, 0, 2], dtype=np.int64).repeat(per)[:n]
    pos = rng.randint(1, 100000, n).astype(np.int64)
    pos = pos[np.lexsort((pos, np.arange(n) // per))]
    length = (19 + reflen).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(length)))
    n_text = int(off[-1])
    rows = np.zeros((11, 30), dtype=np.uint8)                       # one template per REF length, zeros behind the newline
    for k in range(11):
        ln = b"c\t00000\t.\t" + b"A" * (k + 1) + b"\tC\t.\t.\t.\n"
        rows[k, :len(ln)] = np.frombuffer(ln, dtype=np.uint8)
    mat = rows[reflen - 1]
    mat[:, 0] = np.frombuffer(b"abc", dtype=np.uint8)[rank]
    put_decimal(mat, 2, 5, pos)
    ref = mat[:, 10:21]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, (n, 11))]
    np.copyto(ref, letters, where=ref == 65)
    flat = mat.reshape(-1)
    text = aligned_text(n_text)
    text[:n_text] = flat[flat != 0]
    return arrays(text, n_text, rank, pos, off[:-1], length, 3)


# ---- 3. the rank widths --------------------------------------------------------------------------------------------------------
RANK_COUNTS = (1, 2, 3, 4, 5, 1024, 1025, 65536, 65537, 1 << 20)


def from_lines(items, nrank):
    """items: (rank, POS, line) in input order -> arrays"""
    data = b"".join(ln for _r, _p, ln in items)
    text = aligned_text(len(data))
    text[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    length = np.array([len(ln) for _r, _p, ln in items], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(length)))[:-1]
    return arrays(text, len(data), np.array([r for r, _p, _l in items], dtype=np.int64), np.array([p for _r, p, _l in items], dtype=np.int64),
                  off, length, nrank)


def rank_case(nrank):
    """a few dozen records in ranks 0, 1, nrank / 2 and nrank - 1, the files out of rank order; POS 1 and 2^29 in the highest"""
    places = sorted({0, min(1, nrank - 1), nrank // 2, nrank - 1})
    rs = np.random.RandomState(nrank % 9973)
    items = []
    for r in reversed(places):
        for p in sorted(rs.randint(2, 40000, 44 // len(places) - 2).tolist() + [20000, 20000]):
            items.append((r, p, vc.rec("r%d" % r, p, "ACGT"[p % 4] * (1 + p % 3), "A", 10 + p % 50, "PASS")))
    top = nrank - 1
    items.append((top, MAX_END, vc.rec("r%d" % top, MAX_END, "G", "T", 7, "LowQual")))
    items.append((top, 1, vc.rec("r%d" % top, 1, "G", "T", 8, "LowQual")))
    return from_lines(items, nrank)


# ---- 4. the gather's tile line ---------------------------------------------------------------------------------------------------
def _sized(ctg, pos, size):
    base = vc.rec(ctg, pos, "A", "C", gt="0/1:")
    assert size > len(base)
    return vc.rec(ctg, pos, "A", "C", gt="0/1:" + "x" * (size - len(base)))


def tile_items(total, rank=0, pos0=100):
    """64 records of about total / 64 bytes whose lengths sum to exactly `total`"""
    sizes = [total // 64 - 56 + (37 * k) % 113 for k in range(63)]
    sizes.append(total - sum(sizes))
    assert 60 < sizes[-1] < 600
    items = [(rank, pos0 + 3 * k, _sized("r%d" % rank, pos0 + 3 * k, s)) for k, s in enumerate(sizes)]
    assert sum(len(ln) for _r, _p, ln in items) == total
    return items


def short_items(rank, pos0):
    return [(rank, pos0 + k, vc.rec("r%d" % rank, pos0 + k, "ACGT"[k % 4], "A", 10 + k)) for k in range(64)]


def tile_case(total):
    return from_lines(tile_items(total), 1)


def three_tile_case():
    """192 records, in key order a short tile (LDS path), a long one (wave-per-record path), a short one"""
    return from_lines(short_items(0, 10) + tile_items(3 * TILE_TEXT // 2 + 5, 0, 5000) + short_items(1, 10), 2)


# ---- 5. the gather past 4 GiB: arithmetic and the last MiB alone -------------------------------------------------------------------
BIG_BASE = 1 << 32                 # the records lie in the MiB behind this offset of the source text
BIG_LINES, BIG_COPIES, BIG_SHORT = 64, 8193, 200


def big_case():
    """-> (the last MiB of the source text, arrays without "text"): 64 lines of LINE_CAP bytes used 8 193 times each, in rank
    0, every line its own POS; 200 distinct short records in rank 1.  Offsets are those in the whole text, past 2^32"""
    rng = np.random.RandomState(153)
    mib = np.zeros(1 << 20, dtype=np.uint8)
    head = b"r0\t%07d\t.\tA\tC\t30\tPASS\t.\tGT\t"
    line_pos = rng.permutation(np.arange(1000, 1000 + 50 * BIG_LINES, 50))          # the lines' order is not their POS order
    for k in range(BIG_LINES):
        h = head % line_pos[k]
        body = rng.randint(97, 123, LINE_CAP - len(h) - 1).astype(np.uint8)
        mib[k * LINE_CAP:(k + 1) * LINE_CAP] = np.concatenate((np.frombuffer(h, dtype=np.uint8), body, [10]))
    short = [vc.rec("r1", 5 + 11 * ((k * 77) % BIG_SHORT), "ACGT"[k % 4], "A", 10 + k % 60, "PASS", gt="0/1" + ":y" * (k % 19)) for k in range(BIG_SHORT)]
    assert all(40 <= len(s) <= 90 for s in short) and len(set(short)) == BIG_SHORT
    s_at = BIG_LINES * LINE_CAP
    s_len = np.array([len(s) for s in short], dtype=np.int64)
    s_off = s_at + np.concatenate(([0], np.cumsum(s_len)))
    mib[s_at:int(s_off[-1])] = np.frombuffer(b"".join(short), dtype=np.uint8)
    assert s_off[-1] + 16 <= len(mib)
    line = rng.permutation(np.arange(BIG_LINES).repeat(BIG_COPIES))                 # which line each long record is
    n_long = len(line)
    # the short records come first in input order: they sort behind
    rank = np.concatenate((np.ones(BIG_SHORT, dtype=np.int64), np.zeros(n_long, dtype=np.int64)))
    pos = np.concatenate((5 + 11 * ((np.arange(BIG_SHORT) * 77) % BIG_SHORT), line_pos[line])).astype(np.int64)
    off = BIG_BASE + np.concatenate((s_off[:-1], line.astype(np.int64) * LINE_CAP))
    length = np.concatenate((s_len, np.full(n_long, LINE_CAP, dtype=np.int64)))
    a = arrays(None, BIG_BASE + (1 << 20), rank, pos, off, length, 2)
    return mib, a, line
