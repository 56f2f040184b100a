"""What the inputs of tests/vcf_merge_big_cases.py claim about themselves, asserted without a GPU: the GPU tests that
run them (test_gpu_launch_caps.py, test_gpu_vcf_merge.py, test_gpu_past_4gib.py) cross their lines only if these hold.
Where the host form runs here, its order is held to numpy's lexsort by (rank, POS, input index) on the way."""
import numpy as np
import pytest

import launch_cap_cases as L
import vcf_merge_big_cases as B
import vcf_merge_cases as vc


@pytest.fixture(scope="module")
def merge():
    return B.merge_case()


def test_the_lines_are_the_inventorys():
    K = L.KERNELS
    assert B.GRID_FOR == L.GRID_FOR == K["vm_fields"]["line"] == K["vw_fill"]["line"]
    assert B.GATHER_LINE == K["vm_gather"]["line"] and B.BACKFILL_LINE == K["vw_backfill"]["line"]


def test_merge_case_counts_ties_and_windows(merge):
    a, f = merge
    n = a["n"]
    assert n == B.GRID_FOR + 77 == 1048653 and a["nrank"] == 1100 > B.BACKFILL_LINE and f["body"] == B.GRID_FOR
    # eight files laid end to end, each in (rank, POS) order, the whole not: more than six stretches, runs by the thousand
    body_rank, body_pos, file_of = a["rank"][:f["body"]], a["pos"][:f["body"]], f["file_of"]
    seam = np.flatnonzero(file_of[1:] != file_of[:-1]) + 1
    assert len(seam) == B.MERGE_FILES - 1 >= 5
    key = body_rank * (1 << 40) + body_pos
    down = np.flatnonzero(key[1:] < key[:-1]) + 1
    assert set(down.tolist()) <= set(seam.tolist()) and len(down) == len(seam)
    assert a["nruns"] > 5000 and a["run"][-1] == a["nruns"] - 1 and len(a["run_rank"]) == a["nruns"]
    assert np.array_equal(a["run_rank"][a["run"]], a["rank"])
    # every line is unique and carries its input index
    width = f["width"]
    mat = a["text"][:n * width].reshape(n, width)
    idx = sum((mat[:, 18 + k].astype(np.int64) - 48) * 10 ** (6 - k) for k in range(7))
    assert np.array_equal(idx, np.arange(n)) and (mat[:, -1] == 10).all()
    got_pos = sum((mat[:, 6 + k].astype(np.int64) - 48) * 10 ** (8 - k) for k in range(9))
    got_rank = sum((mat[:, 1 + k].astype(np.int64) - 48) * 10 ** (3 - k) for k in range(4))
    assert np.array_equal(got_pos, a["pos"]) and np.array_equal(got_rank, a["rank"])
    # ties: a quarter or more of the records share (rank, POS) with a record of another run; one key more than 4 096 times
    share, longest = B.tie_share(a)
    print("tie share %.3f, longest tie run %d" % (share, longest))
    assert share >= 0.25 and longest > 4096
    assert int(((a["rank"] == f["tie"][0]) & (a["pos"] == f["tie"][1])).sum()) == longest >= B.TIE_RUN + 1
    # 33 ranks hold POS = 2^29: 32 768 windows each, and the windows in all pass vw_fill's line
    far = np.unique(a["rank"][a["pos"] == B.MAX_END])
    assert len(far) == 33 and ((B.MAX_END - 1) >> 14) + 1 == 32768
    used = np.unique(a["rank"])
    unused = np.setdiff1d(np.arange(a["nrank"]), used)
    assert 33 * 32768 + (len(used) - 33) >= 1081344 > L.GRID_FOR
    assert len(unused) > 300 and unused.min() < used.max() and (np.diff(used) > 1).sum() > 100      # gaps among the used ranks
    assert (used >= B.BACKFILL_LINE).any() and (far >= 0).all()
    # among the last 77: a new contig, run starts, a tie with a record in front of the line, a window straddler
    t_rank, t_pos = a["rank"][-77:], a["pos"][-77:]
    assert f["new_rank"] in t_rank and f["new_rank"] not in body_rank
    assert len(np.unique(a["run"][-77:])) > 10
    front = set(zip(body_rank.tolist(), body_pos.tolist()))
    assert sum((r, p) in front for r, p in zip(t_rank.tolist(), t_pos.tolist())) >= 2
    assert ((t_pos == 16383) & f["five"][-77:]).any()
    assert f["five"][:f["body"]].mean() > 0.05


def test_merge_case_host_form_is_the_stable_order(merge):
    a, f = merge
    w = vc.host_form(a)
    order = B.expected_order(a)
    n = a["n"]
    assert w["info"][0] == 0 and w["info"][2] == a["n_text"]
    assert np.array_equal(w["srank"][:n], a["rank"][order]) and np.array_equal(w["sbeg"][:n], a["pos"][order] - 1)
    width = f["width"]
    assert np.array_equal(w["text"][:a["n_text"]].reshape(n, width), a["text"][:a["n_text"]].reshape(n, width)[order])
    nwin = int(w["win_off"][-1])
    assert nwin >= 1081344 and w["info"][1] > 5000
    # an unstable sort gives another text: the tie run's lines differ in their index field alone
    tie = np.flatnonzero((a["rank"][order] == f["tie"][0]) & (a["pos"][order] == f["tie"][1]))
    assert len(tie) > 4096 and (np.diff(order[tie]) > 0).all() and (np.diff(a["run"][order[tie]]) != 0).sum() >= 7
    # the line the device does not vouch for: counted, its place taken by nothing
    b, fb = B.merge_case(with_end=True)
    wb = vc.host_form(b)
    assert wb["info"][0] == 1 and wb["info"][2] == a["n_text"] - width and fb["end_at"] >= B.GRID_FOR


def test_gather_case_lengths_and_the_ragged_tile():
    a = B.gather_case()
    n = a["n"]
    assert n == B.GATHER_LINE + 77 == 4194381 and n % 64 == 13 and -(-n // 64) == 65536 + 2     # blocks 0 and 1 take a second tile
    assert a["len"].min() == 20 and a["len"].max() == 30 and a["n_text"] == a["len"].sum() and 100e6 < a["n_text"] < 120e6
    assert 64 * 30 <= B.TILE_TEXT                                    # every tile takes the LDS path
    t = a["text"]
    assert (t[a["off"] + a["len"] - 1] == 10).all() and (t[a["off"] + 1] == 9).all()
    assert (np.bincount(t[:a["n_text"]], minlength=256)[9] == 7 * n) and a["nruns"] == 8 and a["nrank"] == 3
    # per-record room: 65 bytes of workspace, 32 of chunks
    assert 65 * n < 273e6 and 32 * n < 135e6


def test_rank_cases_place_records_at_the_edges():
    assert B.RANK_COUNTS == (1, 2, 3, 4, 5, 1024, 1025, 65536, 65537, 1048576) and B.RANK_COUNTS[-1] == B.MAX_RANKS
    for nrank in B.RANK_COUNTS:
        a = B.rank_case(nrank)
        assert set(np.unique(a["rank"]).tolist()) == {0, min(1, nrank - 1), nrank // 2, nrank - 1}
        top = a["pos"][a["rank"] == nrank - 1]
        assert top.min() == 1 and top.max() == 1 << 29 and 20 < a["n"] < 64
        w = vc.host_form(a)
        order = B.expected_order(a)
        assert w["info"][0] == 0 and np.array_equal(w["srank"][:a["n"]], a["rank"][order]) and np.array_equal(w["sbeg"][:a["n"]], a["pos"][order] - 1)
        assert w["stats"][2].sum() == a["n"] and w["win_off"][-1] >= 32768


def test_tile_cases_sum_to_the_line_and_one_more():
    for total in (B.TILE_TEXT, B.TILE_TEXT + 1):
        a = B.tile_case(total)
        assert a["n"] == 64 and a["n_text"] == a["len"].sum() == total
        assert vc.host_form(a)["info"].tolist()[:3] == [0, vc.host_form(a)["info"][1], total]
    assert B.TILE_TEXT == 16384
    a = B.three_tile_case()
    w = vc.host_form(a)
    tiles = np.diff(w["ooff"][[0, 64, 128, 192]])
    assert a["n"] == 192 and tiles[0] < B.TILE_TEXT < tiles[1] and tiles[2] < B.TILE_TEXT and w["info"][0] == 0
    # an output that is too small: nothing of a range that does not fit is written
    full = w["text"][:a["n_text"]]
    for cap, kept in ((int(w["ooff"][64]), 1), (int(w["ooff"][64]) - 1, 0), (a["n_text"] - 1, 2), (0, 0)):
        c = vc.host_form(a, out_cap=cap, fill=0x5A)
        edge = int(w["ooff"][64 * kept])
        assert np.array_equal(c["text"][:edge], full[:edge]) and (c["text"][edge:] == 0x5A).all(), cap
        assert np.array_equal(c["ooff"], w["ooff"]) and c["info"].tolist() == w["info"].tolist()


def test_big_case_offsets_lie_either_side_of_2_32():
    """arithmetic alone: no 4 GiB array on the host"""
    mib, a, line = B.big_case()
    n_long = B.BIG_LINES * B.BIG_COPIES
    assert n_long == 524352 and n_long % 64 == 0 and a["n"] == n_long + 200 and len(mib) == 1 << 20
    assert a["n_text"] == (1 << 32) + (1 << 20) and a["off"].min() >= 1 << 32 and (a["off"] + a["len"]).max() + 16 <= a["n_text"]
    assert n_long * B.LINE_CAP == 4295491584 == (1 << 32) + 524288
    assert np.array_equal(np.bincount(line), np.full(64, 8193))
    order = B.expected_order(a)
    assert (a["rank"][order[:n_long]] == 0).all() and (a["rank"][order[n_long:]] == 1).all()
    ooff = np.concatenate(([0], np.cumsum(a["len"][order])))
    assert ooff[524288] == 1 << 32 and ooff[n_long] == 4295491584 and ooff[524287] < 1 << 32 < ooff[524289]
    assert (ooff[n_long:] > 1 << 32).all() and 40 <= a["len"][order[n_long:]].min() and a["len"][order[n_long:]].max() <= 90
    # each line's copies form one tie run, in input order; the lines come in POS order, which is not their order in the text
    lo = line[order[:n_long] - 200]
    assert (np.diff(np.flatnonzero(np.diff(lo) != 0)) == 8193).all() and len(np.unique(lo[::8193])) == 64 and (np.diff(lo[::8193]) < 0).any()
    assert (np.diff(order[:8193]) > 0).all()
    # the lines themselves: LINE_CAP bytes, one newline, nine tabs in front of the long SAMPLE column, distinct
    rows = mib[:64 * B.LINE_CAP].reshape(64, B.LINE_CAP)
    assert (rows[:, -1] == 10).all() and ((rows == 10).sum(axis=1) == 1).all() and ((rows == 9).sum(axis=1) == 9).all()
    assert (rows[:, :64] == 9).sum(axis=1).min() == 9 and len({r.tobytes() for r in rows}) == 64
    for k in (0, 199):
        o, l = int(a["off"][k]) - B.BIG_BASE, int(a["len"][k])
        assert mib[o + l - 1] == 10 and mib[o:o + 2].tobytes() == b"r1"
