#!/usr/bin/env python3
"""Generates tests/golden/cblosc_x.bin: a .bin set of synth candidates packed by the REAL c-blosc (lz4hc, clevel 9, byte
shuffle) through the shim of make_golden_ref.py -- python-blosc's documented pack_array = compress(pickle.dumps(arr,
HIGHEST_PROTOCOL), typesize=itemsize).  One full 500-item X / Y chunk (1 MiB block of 4 / 8 byte-plane streams plus a
leftover block), one partial chunk and the always-appended empty chunk.  Run where libblosc is installed:

    python tests/golden/make_cblosc_x.py [/path/to/libblosc.so.1]
"""
import ctypes
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from clairvoyante_amd import synth
    lib = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else "/opt/conda/lib/libblosc.so.1")
    lib.blosc_compress_ctx.restype = ctypes.c_int

    def pack_array(a):
        data = pickle.dumps(a, pickle.HIGHEST_PROTOCOL)
        out = ctypes.create_string_buffer(len(data) + 16 + 64)
        n = lib.blosc_compress_ctx(ctypes.c_int(9), ctypes.c_int(1), ctypes.c_size_t(a.itemsize), ctypes.c_size_t(len(data)),
                                   data, out, ctypes.c_size_t(len(out)), b"lz4hc", ctypes.c_size_t(0), ctypes.c_int(1))
        assert n > 0
        return out.raw[:n]
    total = 537
    X, cls = synth.make_candidates(total, seed=20261018, return_class=True)[:2]
    X = X.numpy().astype(np.float32)
    cls = cls.numpy().astype(np.int64)
    Y = np.zeros((total, 16), dtype=np.float64)
    Y[np.arange(total), cls % 4] = 1; Y[np.arange(total), 4 + cls % 2] = 1
    Y[np.arange(total), 6 + cls % 4] = 1; Y[np.arange(total), 10 + cls % 6] = 1
    XC, YC = [], []
    for s in range(0, total + 500, 500):              # 0, 500, 1000: full, partial, empty
        XC.append(pack_array(X[s:s + 500])); YC.append(pack_array(Y[s:s + 500]))
    fn = os.path.join(HERE, "cblosc_x.bin")
    with open(fn, "wb") as fh:
        for obj in (total, XC, YC, []):
            pickle.dump(obj, fh)
    print("%s: %d bytes; X chunks %s, Y chunks %s" % (fn, os.path.getsize(fn), [len(c) for c in XC], [len(c) for c in YC]))


if __name__ == "__main__":
    main()
