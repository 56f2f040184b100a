"""Development probe: training step time with fc5's alpha-dropout at rate 0 against 0.1, full 320 /
1 250 / 10 000 and slim 1 250 / 10 000 candidates.  The two rates alternate in one process, a block of steps each,
on one model and one batch, so that clock and box drift fall on both alike; prints the median ms per step of each.
python tools/gpu_dropout5_probe.py [rounds] [steps per block]"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import common
from oracle import cv_oracle as O
from clairvoyante_amd import clairvoyante_v3, clairvoyante_v3_slim, synth

R = int(sys.argv[1]) if len(sys.argv) > 1 else 7
K = int(sys.argv[2]) if len(sys.argv) > 2 else 20
for arch, n in (("full", 320), ("full", 1250), ("full", 10000), ("slim", 1250), ("slim", 10000)):
    m = clairvoyante_v3.Clairvoyante() if arch == "full" else clairvoyante_v3_slim.Clairvoyante()
    m.setParameters(common.bench_params(O, arch))
    xt, cls, rf, alt, il = synth.make_candidates(n, seed=synth.BASE_SEED, device="cuda", return_class=True)
    x = xt.contiguous(); y = synth.make_labels(cls, rf, alt, il).contiguous()
    ms = {0.0: [], 0.1: []}
    for r in range(R + 1):
        for rate in ((0.0, 0.1) if r % 2 == 0 else (0.1, 0.0)):
            m.dropoutRateFC5Val = rate
            for _ in range(3):
                m.trainDeferred(x, y)
            m.readLosses()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                m.trainDeferred(x, y)
            m.readLosses()
            torch.cuda.synchronize()
            if r > 0:                                  # (round 0: warm-up)
                ms[rate].append((time.perf_counter() - t0) / K * 1e3)
    a, b = statistics.median(ms[0.0]), statistics.median(ms[0.1])
    print("%s %6d  rate5 0: %.4f ms  rate5 0.1: %.4f ms  delta %+.1f us  (spread %.1f / %.1f us)" % (
        arch, n, a, b, (b - a) * 1e3, (max(ms[0.0]) - min(ms[0.0])) * 1e3, (max(ms[0.1]) - min(ms[0.1])) * 1e3), flush=True)
    m.close()
