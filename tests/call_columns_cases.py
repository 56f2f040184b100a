"""The Python definition of callVarBam's hop between the pileup and the call loop -- the filter of
callVarBam.region_tensors (host route) plus utils_v2.PosBatch.from_columns -- and the inputs the tests of the device form
share (test_call_columns_host.py, test_gpu_call_columns.py)."""
import numpy as np

FLANK = 16


def definition(ctg, centres, touched, ref_seq, shift):
    """-> (index int64 [k], text bytes, meta [k,6] int64): the lines of region_tensors, then PosBatch.from_columns"""
    from clairvoyante_amd.utils_v2 import PosBatch
    centres = np.asarray(centres, dtype=np.int64)
    new_pos = centres - shift
    seqs = [ref_seq[max(int(p) - (FLANK + 1), 0):int(p) + FLANK].upper() if p - (FLANK + 1) >= 0 else b"" for p in new_pos]
    ok = np.array([len(sq) > FLANK and sq[FLANK:FLANK + 1] in (b"A", b"C", b"G", b"T") for sq in seqs], dtype=bool)
    idx = np.flatnonzero(np.asarray(touched, dtype=bool) & ok) if len(centres) else np.zeros(0, dtype=np.int64)
    _start, _rows, buf, meta = PosBatch.from_columns(ctg, centres[idx], [seqs[i] for i in idx]).pieces()[0]
    return idx.astype(np.int64), bytes(buf), np.ascontiguousarray(meta, dtype=np.int64).reshape(-1, 6)


def every_byte_reference(rng, length):
    """`length` bytes: mostly bases in both cases and N / n, a fifth of them any byte value, and every one of the 256 values
    at least once"""
    common = np.frombuffer(b"ACGTACGTacgtNnRYKMswbdhv", dtype=np.uint8)
    ref = common[rng.integers(0, len(common), size=length)].copy()
    wild = rng.random(length) < 0.2
    ref[wild] = rng.integers(0, 256, size=int(wild.sum()), dtype=np.uint8)
    at = rng.choice(length, size=256, replace=False)
    ref[at] = np.arange(256, dtype=np.uint8)
    return ref.tobytes()


def random_case(seed, ref_first, n=20000, ref_len=6000, ctg=b"chr21"):
    """centres around and beyond both ends of a reference of every byte value whose first byte is 0-based position
    ref_first; four in five touched"""
    rng = np.random.default_rng(seed)
    ref = every_byte_reference(rng, ref_len)
    centres = rng.integers(ref_first - 40, ref_first + ref_len + 60, size=n).astype(np.int64)
    edges = np.array([ref_first + d for d in (-1, 0, 1, 15, 16, 17, 18, ref_len - 17, ref_len - 16, ref_len - 1, ref_len, ref_len + 1)])
    centres[:len(edges)] = edges
    centres = np.clip(centres, -(2 ** 31), 2 ** 31 - 1)
    touched = (rng.random(n) < 0.8).astype(np.uint8)
    touched[:len(edges)] = 1
    return ctg, centres, touched, ref, ref_first
