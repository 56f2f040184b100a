"""The workspace contract of the device entry points that come as a pair (cv_X_workspace, cv_X_dev): the bytes the first
returns are exactly what the second needs, and a workspace that is too small or not 256-byte aligned is refused on the host,
before anything is launched.  Per pair three calls over the smallest valid inputs (what is under test is the plumbing around
the kernels, not the kernels):

  exact       the workspace holds exactly the bytes asked for, inside a buffer filled with 0xA5: the result is the host
              form's (or the definition the pair's own test uses), and no byte behind the workspace changed
  short       one byte less: non-zero, cv_last_error says "workspace holds", no output byte changed
  misaligned  the base 128 bytes further: non-zero, cv_last_error says "256-byte aligned", no output byte changed
"""
import ctypes

import numpy as np
import pytest

import call_columns_cases as cc
import textparse_cases as T
import trainset_cases
import truth_cases as tc

pytestmark = pytest.mark.gpu
FILL = 0xA5
SLACK = 1024                                                 # bytes of the buffer behind the workspace (and room for the shifted base)

# one BED over two contigs, as cv_bed_table_dev takes it (unsorted) and as it returns it
BED_BEGIN, BED_END, BED_RUN, BED_RUN_CTG = [10, 5, 30], [20, 25, 40], [0, 0, 1], [0, 1]
BED_OFF, BED_SORTED, BED_EMAX = [0, 2, 3], [5, 10, 30], [25, 25, 40]


def _abi():
    from clairvoyante_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _h(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _up(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()     # (a copy: np.frombuffer gives a read-only view)


def _room(shape, dtype):
    """an output buffer of that shape whose every byte is FILL"""
    import torch
    nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda").view(dtype).reshape(shape)


def _bytes_of(t):
    import torch
    return t.reshape(-1).view(torch.uint8).clone()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need(fn, *args):
    A, _lib = _abi()
    need = ctypes.c_int64(-1)
    A.check(fn(*(args + (ctypes.byref(need),))))
    assert need.value > 0 and need.value % 256 == 0
    return need.value


# ---- the twelve pairs: each -> (bytes the workspace function asks for, call(ws, ws_bytes) -> rc, outputs, check()) ------------
def _truth_lines():
    import torch
    A, lib = _abi()
    text = b"\n".join(trainset_cases.TRUTH.encode().split(b"\n")[:3]) + b"\n"
    n = 4
    buf = _up(np.frombuffer(text, dtype=np.uint8))
    pos, label, run = _room((n,), torch.int64), _room((n, 16), torch.float32), _room((n,), torch.int32)
    tok, info = _room((n, 2), torch.int64), _room((8,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_truth_lines_dev(_p(buf), len(text), tc.VAR, None, 0, 0, 0, 0, n, _p(pos), None, _p(label), _p(run), _p(tok), _p(info),
                                      ws, nbytes, st)

    def check():
        hpos, hlab, hrun = np.zeros(n, np.int64), np.zeros((n, 16), np.float32), np.zeros(n, np.int32)
        htok, hinfo = np.zeros((n, 2), np.int64), np.zeros(8, np.int64)
        A.check(lib.cv_truth_lines_host_form(text, len(text), tc.VAR, None, 0, 0, 0, 0, n, _h(hpos), None, _h(hlab), _h(hrun), _h(htok),
                                             _h(hinfo)))
        rows, runs = int(hinfo[2]), int(hinfo[5])
        assert hinfo[:6].tolist() == [len(text), 3, 3, 0, 0, runs] and runs >= 1
        assert info.cpu().numpy().tolist() == hinfo.tolist()
        assert np.array_equal(pos.cpu().numpy()[:rows], hpos[:rows]) and np.array_equal(run.cpu().numpy()[:rows], hrun[:rows])
        assert np.array_equal(label.cpu().numpy()[:rows], hlab[:rows]) and hlab[:rows].any()
        assert np.array_equal(tok.cpu().numpy()[:runs], htok[:runs])
    return _need(lib.cv_truth_lines_workspace, len(text), n), call, [pos, label, run, tok, info], check


def _bed_table():
    import torch
    _A, lib = _abi()
    begin, end, run, rc = _up(BED_BEGIN, np.int64), _up(BED_END, np.int64), _up(BED_RUN, np.int32), _up(BED_RUN_CTG, np.int32)
    off, srt, emax = _room((3,), torch.int64), _room((3,), torch.int64), _room((3,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_bed_table_dev(3, _p(begin), _p(end), _p(run), _p(rc), 2, 2, _p(off), _p(srt), _p(emax), ws, nbytes, st)

    def check():
        assert off.tolist() == BED_OFF and srt.tolist() == BED_SORTED and emax.tolist() == BED_EMAX
    return _need(lib.cv_bed_table_workspace, 3), call, [off, srt, emax], check


def _truth_tables():
    """rows (contig 0): 12, 3, 12 again.  3 lies in front of every interval; of the two rows at 12 the last one wins"""
    import torch
    _A, lib = _abi()
    labels_in = (np.arange(48, dtype=np.float32) / 32).reshape(3, 16)
    pos, label, run, rc = _up([12, 3, 12], np.int64), _up(labels_in), _up([0, 0, 0], np.int32), _up([0], np.int32)
    bed_off, bed_begin, bed_emax = _up(BED_OFF, np.int64), _up(BED_SORTED, np.int64), _up(BED_EMAX, np.int64)
    truth_off, every_off = _room((3,), torch.int64), _room((3,), torch.int64)
    truth_pos, every_pos, labels, counts = _room((3,), torch.int64), _room((3,), torch.int64), _room((3, 16), torch.float32), _room((2,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_truth_tables_dev(3, _p(pos), _p(label), _p(run), _p(rc), 1, 2, 1, _p(bed_off), _p(bed_begin), _p(bed_emax), _p(truth_off),
                                       _p(truth_pos), _p(labels), _p(every_off), _p(every_pos), _p(counts), ws, nbytes, st)

    def check():
        assert counts.tolist() == [1, 2] and truth_off.tolist() == [0, 1, 1] and every_off.tolist() == [0, 2, 2]
        assert truth_pos.tolist()[:1] == [12] and every_pos.tolist()[:2] == [3, 12]
        assert np.array_equal(labels.cpu().numpy()[0], labels_in[2])
    return _need(lib.cv_truth_tables_workspace, 3), call, [truth_off, truth_pos, labels, every_off, every_pos, counts], check


ITEMS = b"chr1 12 a\nchr1 3 bb\nchr2 35 c\n"


def _item_lines_host():
    A, lib = _abi()
    n = 4
    pos, run, off, ln = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    tok, info = np.zeros((n, 2), np.int64), np.zeros(8, np.int64)
    A.check(lib.cv_item_lines_host_form(ITEMS, len(ITEMS), n, _h(pos), _h(run), _h(off), _h(ln), _h(tok), _h(info)))
    assert info[:6].tolist() == [len(ITEMS), 3, 3, 0, 0, 2] and pos[:3].tolist() == [12, 3, 35] and run[:3].tolist() == [0, 0, 1]
    return pos, run, off, ln, tok, info


def _item_lines():
    import torch
    _A, lib = _abi()
    n = 4
    buf = _up(np.frombuffer(ITEMS, dtype=np.uint8))
    pos, run, off, ln = _room((n,), torch.int64), _room((n,), torch.int32), _room((n,), torch.int64), _room((n,), torch.int64)
    tok, info = _room((n, 2), torch.int64), _room((8,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_item_lines_dev(_p(buf), len(ITEMS), n, _p(pos), _p(run), _p(off), _p(ln), _p(tok), _p(info), ws, nbytes, st)

    def check():
        hpos, hrun, hoff, hln, htok, hinfo = _item_lines_host()
        assert info.cpu().numpy().tolist() == hinfo.tolist()
        for got, want in ((pos, hpos), (run, hrun), (off, hoff), (ln, hln)):
            assert np.array_equal(got.cpu().numpy()[:3], want[:3])
        assert np.array_equal(tok.cpu().numpy()[:2], htok[:2])
    return _need(lib.cv_item_lines_workspace, len(ITEMS), n), call, [pos, run, off, ln, tok, info], check


def _items_keep():
    import torch
    A, lib = _abi()
    hpos, hrun, hoff, hln, _tok, _info = _item_lines_host()
    cols = [np.ascontiguousarray(a[:3]) for a in (hpos, hrun, hoff, hln)]
    rc, bed = np.array(BED_RUN_CTG, np.int32), [np.array(a, np.int64) for a in (BED_OFF, BED_SORTED, BED_EMAX)]
    buf = _up(np.frombuffer(ITEMS, dtype=np.uint8))
    d_cols, d_rc, d_bed = [_up(a) for a in cols], _up(rc), [_up(a) for a in bed]
    out, counts = _room((len(ITEMS) + 64,), torch.uint8), _room((4,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_items_keep_dev(_p(buf), len(ITEMS), 3, _p(d_cols[0]), _p(d_cols[1]), _p(d_cols[2]), _p(d_cols[3]), _p(d_rc), 2, 2,
                                     _p(d_bed[0]), _p(d_bed[1]), _p(d_bed[2]), 1, _p(out), len(ITEMS), _p(counts), ws, nbytes, st)

    def check():
        htext, hcounts = np.full(len(ITEMS), FILL, np.uint8), np.zeros(4, np.int64)
        A.check(lib.cv_items_keep_host_form(ITEMS, len(ITEMS), 3, _h(cols[0]), _h(cols[1]), _h(cols[2]), _h(cols[3]), _h(rc), 2, 2, _h(bed[0]),
                                            _h(bed[1]), _h(bed[2]), 1, _h(htext), len(ITEMS), _h(hcounts)))
        kept = b"chr1 12 a\nchr2 35 c\n"                        # (3 lies in front of chr1's intervals)
        assert hcounts.tolist() == [3, 2, len(kept), 0] and htext[:len(kept)].tobytes() == kept
        got = out.cpu().numpy()
        assert counts.tolist() == hcounts.tolist() and got[:len(kept)].tobytes() == kept and (got[len(kept):] == FILL).all()
    return _need(lib.cv_items_keep_workspace, 3), call, [out, counts], check


def _sample_positions():
    import torch
    from clairvoyante_amd import bed_items, draws
    _A, lib = _abi()
    count = 50
    out, counts = _room((count,), torch.int64), _room((2,), torch.int64)
    st = _stream()
    h = draws.fnv1a32("chr7")

    def call(ws, nbytes):
        return lib.cv_sample_positions_dev(11, h, 1, count, 0.5, 0, None, None, _p(out), count, _p(counts), ws, nbytes, st)

    def check():
        want = bed_items.sample_positions_host("chr7", 1, 1 + count, 0.5, None, 11)
        assert 10 < len(want) < 40 and counts.tolist() == [len(want), len(want)]
        assert np.array_equal(out.cpu().numpy()[:len(want)], want)
    return _need(lib.cv_sample_positions_workspace, count), call, [out, counts], check


def _trainset_tokens():
    """three rows: chr1 12, chr1 3, chr2 35; the centre bases A, C, G"""
    import torch
    _A, lib = _abi()
    toks = [(b"chr1", b"12"), (b"chr1", b"3"), (b"chr2", b"35")]
    text, meta = b"", []
    for i, (ctg, p) in enumerate(toks):
        seq = (b"ACGT" * 9)[i:i + 33]
        meta.append([len(text), len(ctg), len(text) + len(ctg) + 1, len(p), len(text) + len(ctg) + len(p) + 2, 33])
        text += ctg + b" " + p + b" " + seq + b"\n"
    buf, d_meta = _up(np.frombuffer(text, dtype=np.uint8)), _up(meta, np.int64)
    pos, run = _room((3,), torch.int64), _room((3,), torch.int32)
    digits, centre, flags = (_room((3,), torch.uint8) for _ in range(3))
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_trainset_tokens(_p(buf), _p(d_meta), None, 3, _p(pos), _p(digits), _p(centre), _p(flags), _p(run), ws, nbytes, st)

    def check():
        assert pos.tolist() == [12, 3, 35] and digits.tolist() == [2, 1, 2] and centre.tolist() == [0, 1, 2]
        assert flags.tolist() == [1, 0, 1] and run.tolist() == [0, 0, 1]         # (1 = CV_TRAINSET_RUN_START)
    return _need(lib.cv_trainset_tokens_workspace, 3), call, [pos, digits, centre, flags, run], check


def _trainset_finish():
    """the rows of _trainset_tokens, all kept, the second one with a truth label: sorted() over "chr1:12", "chr1:3", "chr2:35" """
    import torch
    _A, lib = _abi()
    label = (np.arange(16, dtype=np.float32) / 16).reshape(1, 16)
    ctg, pos, truth, rank = _up([0, 0, 1], np.int32), _up([12, 3, 35], np.int64), _up([-1, 0, -1], np.int32), _up([0, 1], np.int32)
    digits, centre, keep, labels = _up([2, 1, 2], np.uint8), _up([0, 1, 2], np.uint8), _up([1, 1, 1], np.uint8), _up(label)
    src, y, total = _room((3,), torch.int64), _room((3, 16), torch.float32), _room((1,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_trainset_finish(3, _p(ctg), _p(pos), _p(digits), _p(centre), _p(keep), _p(truth), _p(rank), 2, _p(labels), 1, _p(src),
                                      _p(y), _p(total), ws, nbytes, st)

    def check():
        want = np.zeros((3, 16), np.float32)
        want[:, [5, 6, 10]] = 1.0                               # HOM, REF, length 0 ...
        want[0, 0] = want[2, 2] = 1.0                           # ... and the centre base
        want[1] = label[0]
        assert total.tolist() == [3] and src.tolist() == [0, 1, 2] and np.array_equal(y.cpu().numpy(), want)
    return _need(lib.cv_trainset_finish_workspace, 3), call, [src, y, total], check


def _vcf_records():
    import torch
    import test_gpu_vcf_format as V
    _A, lib = _abi()
    b = V.random_batch(4, 77)
    want_text, want_off, want_status, want_info = V.host_form(b)
    n, cap = b.n, len(want_text)
    call_d, qual, x, buf, meta = (_up(a) for a in (b.call, b.qual, b.x, b.buf, b.meta))
    off, status, info = _room((n + 1,), torch.int64), _room((n,), torch.uint8), _room((4,), torch.int64)
    text = _room((cap + 64,), torch.uint8)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_vcf_records_dev(_p(call_d), _p(qual), n, _p(x), None, _p(buf), _p(meta), None, 1, 0, 0, _p(off), _p(status), _p(info),
                                      _p(text), cap, ws, nbytes, st)

    def check():
        assert cap > 0 and (want_status == V.DEVICE).any()
        assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(status.cpu().numpy(), want_status)
        assert np.array_equal(info.cpu().numpy(), want_info)
        got = text.cpu().numpy()
        assert got[:cap].tobytes() == want_text and (got[cap:] == FILL).all()
    return _need(lib.cv_vcf_records_workspace, n), call, [off, status, info, text], check


def _tensor_rows_text():
    import torch
    import test_gpu_rowtext as R
    _A, lib = _abi()
    ref, centres, counts = R.make_ref(200), np.array([100, 105, 110], dtype=np.int64), R.make_counts(3, 4)
    want = R.host_rows("ctgA", centres, ref, 0, counts)
    total = sum(len(w) for w in want)
    cen, rf, cnt = _up(centres), _up(np.frombuffer(ref, dtype=np.uint8)), _up(counts)
    off, status, text = _room((4,), torch.int64), _room((3,), torch.uint8), _room((total + 64,), torch.uint8)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_tensor_rows_text_dev(b"ctgA", 4, _p(cen), 3, _p(rf), 0, len(ref), _p(cnt), _p(off), _p(status), _p(text), total, ws,
                                           nbytes, st)

    def check():
        assert off.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist() and status.tolist() == [0, 0, 0]
        got = text.cpu().numpy()
        assert got[:total].tobytes() == b"".join(want) and (got[total:] == FILL).all()
    return _need(lib.cv_tensor_rows_text_workspace, 3), call, [off, status, text], check


def _call_columns():
    import torch
    import test_gpu_rowtext as R
    _A, lib = _abi()
    ctg, first0, ref = b"chrX", 1000, R.make_ref(200)
    centres, touched = first0 + np.array([40, 50, 60, 70], dtype=np.int64), np.array([1, 0, 1, 1], dtype=np.uint8)
    n, cap = 4, len(ctg) + 43 * 4
    c32, t8, rf = _up(centres, np.int32), _up(touched), _up(np.frombuffer(ref, dtype=np.uint8))
    index, meta, text, info = _room((n,), torch.int64), _room((n, 6), torch.int64), _room((cap + 64,), torch.uint8), _room((4,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_call_columns_dev(ctg, len(ctg), _p(c32), _p(t8), n, _p(rf), first0, len(ref), _p(index), _p(meta), _p(text), cap,
                                       _p(info), ws, nbytes, st)

    def check():
        windex, wtext, wmeta = cc.definition(ctg, centres, touched, ref, first0)
        k = len(windex)
        assert 1 <= k <= 3 and info.tolist() == [k, len(wtext), n, 0]
        assert np.array_equal(index.cpu().numpy()[:k], windex) and np.array_equal(meta.cpu().numpy()[:k], wmeta)
        got = text.cpu().numpy()
        assert got[:len(wtext)].tobytes() == wtext and (got[len(wtext):] == FILL).all()
    return _need(lib.cv_call_columns_workspace, n), call, [index, meta, text, info], check


def _parse_tensor_text():
    import torch
    _A, lib = _abi()
    rng, vocab = np.random.RandomState(9), T._vocabulary()
    rows_text = ("\n".join(T.good_row(rng, vocab, i) for i in range(3)) + "\n").encode()
    lines = 4
    buf = _up(np.frombuffer(rows_text, dtype=np.uint8))
    x, meta = _room((lines, T.NV), torch.float32), _room((lines, 6), torch.int64)
    status, info = _room((lines,), torch.uint8), _room((4,), torch.int64)
    st = _stream()

    def call(ws, nbytes):
        return lib.cv_parse_tensor_text_dev(_p(buf), len(rows_text), lines, _p(x), _p(meta), _p(status), _p(info), ws, nbytes, st)

    def check():
        hc, bad, hx, hmeta = T.host_parse(rows_text)
        assert bad == 0 and hc == len(rows_text) and hx.shape[0] == 3
        assert info.tolist() == [len(rows_text), 3, 3, 0] and status.tolist()[:3] == [T.ROW] * 3
        assert np.array_equal(x.cpu().numpy()[:3].view(np.uint32), hx.view(np.uint32)) and np.array_equal(meta.cpu().numpy()[:3], hmeta)
    return _need(lib.cv_parse_tensor_text_dev_workspace, len(rows_text), lines), call, [x, meta, status, info], check


PAIRS = {"truth_lines": _truth_lines, "bed_table": _bed_table, "truth_tables": _truth_tables, "item_lines": _item_lines,
         "items_keep": _items_keep, "sample_positions": _sample_positions, "trainset_tokens": _trainset_tokens,
         "trainset_finish": _trainset_finish, "vcf_records": _vcf_records, "tensor_rows_text": _tensor_rows_text,
         "call_columns": _call_columns, "parse_tensor_text": _parse_tensor_text}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_workspace_contract(pair):
    import torch
    _A, lib = _abi()
    need, call, outputs, check = PAIRS[pair]()
    slab = torch.full((need + SLACK,), FILL, dtype=torch.uint8, device="cuda")
    lead = -slab.data_ptr() % 256
    base = slab.data_ptr() + lead
    untouched = [_bytes_of(t) for t in outputs]
    same = lambda: all(torch.equal(_bytes_of(t), u) for t, u in zip(outputs, untouched))
    # one byte short, then a base that is not 256-byte aligned: refused on the host, nothing written
    assert call(ctypes.c_void_p(base), need - 1) != 0
    assert b"workspace holds" in lib.cv_last_error(), lib.cv_last_error()
    torch.cuda.synchronize()
    assert same() and bool((slab == FILL).all())
    assert call(ctypes.c_void_p(base + 128), need) != 0
    assert b"256-byte aligned" in lib.cv_last_error(), lib.cv_last_error()
    torch.cuda.synchronize()
    assert same() and bool((slab == FILL).all())
    # exactly the bytes asked for
    assert call(ctypes.c_void_p(base), need) == 0, lib.cv_last_error()
    torch.cuda.synchronize()
    check()
    assert bool((slab[:lead] == FILL).all()) and bool((slab[lead + need:] == FILL).all())
