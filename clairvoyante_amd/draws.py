"""The keyed draws of the training-set routes (csrc/cv_draw_core.hpp): Philox4x32-10 keyed by (seed; position, contig
name, stream, late), the same text on host and device.  Stream SAMPLE is ExtractVariantCandidates --gen4Training
(keep unless u > outputProb, ExtractVariantCandidates.py:203), stream PAIR is PairWithNonVariants (keep if u < r, :119),
stream RANDOM is RandomSampling (keep if u <= prob, RandomSampling.py:67).
"""
import ctypes
import logging
import random

import numpy as np

from . import _lib

SAMPLE, PAIR, RANDOM = 0, 1, 2


def fnv1a32(name):
    """FNV-1a-32 of the contig name's bytes: the fourth counter word"""
    h = 2166136261
    for b in (name.encode() if isinstance(name, str) else bytes(name)):
        h = ((h ^ b) * 16777619) & 0xffffffff
    return h


def resolve_seed(seed, who):
    """--seed N, or 64 bits of Python's generator taken once (random.seed(k) in a driver makes the run repeatable); logged"""
    if seed is None:
        seed = random.getrandbits(64)
    seed = int(seed) & 0xffffffffffffffff
    logging.info("%s: seed %d" % (who, seed))
    return seed


def draws(seed, stream, ctg, pos, late=None):
    """u in [0, 1) (float64) for the rows at the 1-based positions `pos` of contig `ctg`; late: 1 for a late second entry"""
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    u = np.empty(len(pos), dtype=np.float64)
    lt = None if late is None else np.ascontiguousarray(late, dtype=np.int32)
    _lib.check(_lib.load().cv_draws_host(int(seed), int(stream), fnv1a32(ctg), pos.ctypes.data_as(ctypes.c_void_p),
                                         None if lt is None else lt.ctypes.data_as(ctypes.c_void_p), len(pos),
                                         u.ctypes.data_as(ctypes.c_void_p)))
    return u
