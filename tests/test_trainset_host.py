"""The host side of the device training-set route (utils_v2.GetTrainingSetDevice): the sort key, the index shuffle, the
shared BED / truth reader and its tables, the decisions to hand an input to the host builder.  No GPU needed."""
import os
import random

import numpy as np
import pytest

import trainset_cases as cases

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["chr1", "chr10", "chr2", "1", "10", "Chr1", "chr1_random", "chr1-a", "chr1.b", "chrUn/9", "chr", "chr1 ", "c", "~", "!x", "chr100"]


def test_sort_key_orders_like_sorted_strings():
    """rank << 48 | padded coordinate << 4 | digits against sorted() over "ctg:pos": names that are prefixes of one
    another, bytes on both sides of ':' (0x3a) and of the digits, coordinates that are prefixes of one another"""
    from clairvoyante_amd import utils_v2
    rng = random.Random(5)
    names = [n.encode() for n in NAMES]
    rank = utils_v2.contig_ranks(names)
    coords = [0, 1, 9, 10, 19, 99, 100, 101, 1000, 10 ** 11, 10 ** 12 - 1, 123456789012, 12345678901, 1234567890]
    for d in range(1, 13):
        coords += [rng.randrange(10 ** (d - 1), 10 ** d) for _ in range(150)]
    items = [(rng.randrange(len(names)), rng.choice(coords)) for _ in range(20000)]
    items += [(i, c) for i in range(len(names)) for c in coords[:14]]
    want = sorted(set(NAMES[i] + ":" + str(c) for i, c in items))
    keys = {utils_v2.trainset_sort_key(rank[i], c, len(str(c))): NAMES[i] + ":" + str(c) for i, c in items}
    assert [keys[k] for k in sorted(keys)] == want            # (equal keys <=> equal strings: the dict lost nothing)
    assert len(keys) == len(want) and max(keys) < 1 << 64
    assert utils_v2.trainset_sort_key(65534, 10 ** 12 - 1, 12) < (1 << 64) - 1       # the key of a dropped row stays free


def test_index_shuffle_is_random_shuffle_of_the_keys():
    from clairvoyante_amd import utils_v2
    for n in (0, 1, 2, 499, 1000, 1015):
        keys = ["k%d" % i for i in range(n)]
        random.seed(77); want = list(keys); random.shuffle(want)
        random.seed(77); p = utils_v2.shuffled_indices(n)
        assert [keys[i] for i in p] == want


def test_shared_reader_gives_the_loop_its_labels(tmp_path):
    """_read_bed_truth: last truth row of a key wins, rows outside the BED are dropped, the end += 1 quirk; and the
    tables cv_trainset_join is given answer as _Intervals.hit and the dict do"""
    from clairvoyante_amd import utils_v2
    f = cases.write_case(str(tmp_path), "full")
    tree, Y = utils_v2._read_bed_truth(f["var"], f["bed"])
    assert "chr1:3000" not in Y and "chrX:5" in Y
    assert Y["chr1:1040"] == [0, 0, 1, 0, 0, 1.0, 0, 1.0, 0, 0, 1.0, 0, 0, 0, 0, 0]          # hom C>G replaced het C>T
    assert Y["chr1:1004"][:6] == [0.5, 0.5, 0, 0, 1.0, 0] and Y["chr1:1022"][8] == 1.0 and Y["chr1:1022"][15] == 1.0
    assert Y["chr1:1037"][9] == 1.0 and Y["chr1:1037"][15] == 1.0 and Y["chr1:1034"][14] == 1.0
    hit = tree["chr1"].hit
    assert hit(1000) and hit(1499) and hit(1998) and not hit(1999) and hit(5000) and not hit(5001) and hit(1300) and not hit(999)
    assert hit(0) and hit(148) and not hit(149)
    _tree2, Y2 = utils_v2._read_bed_truth(f["var"], None)
    assert "chr1:3000" in Y2
    names, t = utils_v2._trainset_tables(tree, Y, True)
    assert names[:4] == [b"chr1", b"chr10", b"chr2", b"chrX"]
    for i, name in enumerate(names):
        lo, hi = t["bed_off"][i], t["bed_off"][i + 1]
        for p in list(range(0, 160)) + list(range(990, 2010)) + [4999, 5000, 5001, 123456789012, 123456789099]:
            k = int(np.searchsorted(t["bed_begin"][lo:hi], p, side="right"))
            assert (k > 0 and t["bed_emax"][lo + k - 1] > p) == bool(tree[name.decode()].hit(p))
        lo, hi = t["truth_off"][i], t["truth_off"][i + 1]
        assert list(t["truth_pos"][lo:hi]) == sorted(t["truth_pos"][lo:hi])
        for j in range(lo, hi):
            assert list(t["labels"][j]) == Y["%s:%d" % (name.decode(), t["truth_pos"][j])]
    assert len(t["truth_pos"]) == len(Y)
    with pytest.raises(KeyError):                               # a truth contig the BED file lacks, as the loop always did
        utils_v2._read_bed_truth(f["var"], cases.write_case(str(tmp_path), "k0")["bed"])


def test_tokens_the_device_route_takes():
    from clairvoyante_amd import utils_v2
    ok = [b"0", b"9", b"10", b"123456789012"]
    bad = [b"", b"007", b"00", b"1234567890123", b"+5", b"-1", b"1e3", b"12 ", b"\xb2", b"1_0"]
    assert all(utils_v2.canonical_coordinate(t) for t in ok) and not any(utils_v2.canonical_coordinate(t) for t in bad)
    assert utils_v2.contig_token_ok(b"chrUn/9") and utils_v2.contig_token_ok(b"chr1 ")
    assert not any(utils_v2.contig_token_ok(t) for t in (b"ch:r", b"ch\0r", b"chr\x80", b"\xffhr"))


def test_fallback_decisions(tmp_path, monkeypatch):
    from clairvoyante_amd import utils_v2
    f = cases.write_case(str(tmp_path), "k499")
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    assert utils_v2.trainset_host_reason(f["plain"]) == "no GPU"
    for forced in ("device", "host", None):
        if forced:
            monkeypatch.setenv("CV_TEXT_PARSE", forced)
        else:
            monkeypatch.delenv("CV_TEXT_PARSE", raising=False)
        assert not utils_v2.trains_on_device(f["plain"])
    monkeypatch.setenv("CV_TEXT_PARSE", "gpu")
    with pytest.raises(ValueError):
        utils_v2.trains_on_device(f["plain"])
    monkeypatch.delenv("CV_TEXT_PARSE", raising=False)
    # with a GPU: the floors decide, an ordinary .gz never goes, a budget below twice the rows sends the call to the host
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: True)
    assert utils_v2.TRAINSET_DEVICE_MIN_BYTES[1] is None and not utils_v2.trains_on_device(f["gz"])
    assert not utils_v2.trains_on_device(f["plain"]) and not utils_v2.trains_on_device("PIPE")
    monkeypatch.setattr(utils_v2, "TRAINSET_DEVICE_MIN_BYTES", (1000, None))
    monkeypatch.setattr(utils_v2, "TRAINSET_BGZF_DEVICE_MIN_BYTES", 1000)
    assert utils_v2.trains_on_device(f["plain"]) and utils_v2.trains_on_device(f["bgzf"]) and not utils_v2.trains_on_device(f["gz"])
    rows = utils_v2._estimated_rows(f["plain"])
    assert 499 <= rows <= 520 and 499 <= utils_v2._estimated_rows(f["bgzf"]) <= 520
    monkeypatch.setattr(utils_v2, "TRAINSET_FREE_BYTES", rows * 2112 * 4 + 16)
    assert utils_v2.trainset_host_reason(f["plain"]) is None
    monkeypatch.setattr(utils_v2, "TRAINSET_FREE_BYTES", rows * 2112 * 4 - 16)
    assert "fit" in utils_v2.trainset_host_reason(f["plain"])


def test_without_a_gpu_the_set_is_the_host_loops(tmp_path, monkeypatch):
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    f = cases.write_case(str(tmp_path), "full")
    want = cases.host_result(f, "full", True)
    random.seed(cases.SEED)
    ts = utils_v2.GetTrainingSetDevice(f["plain"], f["var"], f["bed"])
    assert ts.route == "host" and ts.reason == "no GPU" and ts.total == want[0]
    got = cases.arrays_of(ts.blocks())
    assert got[:2] == want[:2] and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and got[4] == want[4]
    assert ts.keys() == want[4] and np.array_equal(np.asarray(ts.X).reshape(-1, 528).view(np.uint32), want[2])
    assert np.array_equal(np.asarray(ts.Y, dtype=np.float64), want[3])


def test_training_array_still_equals_the_golden_fixture_without_a_gpu(monkeypatch):
    from clairvoyante_amd import utils_v2
    monkeypatch.setattr(utils_v2, "_gpu_present", lambda: False)
    monkeypatch.setenv("CV_TEXT_PARSE", "device")              # (forced, and still the host loop: there is no device)
    d = np.load(os.path.join(G, "trainarray.npz"))
    random.seed(1234)
    got = cases.arrays_of(utils_v2.GetTrainingArray(os.path.join(G, "trainarray_tensor.txt.gz"), os.path.join(G, "trainarray_var.txt.gz"),
                                                    os.path.join(G, "trainarray.bed.gz")))
    assert got[0] == int(d["total"]) and got[1] == int(d["nblocks"])
    assert np.array_equal(got[2], d["X"].reshape(got[0], -1).view(np.uint32)) and np.array_equal(got[3], d["Y"])
    assert got[4] == [str(s) for s in d["pos"]]
