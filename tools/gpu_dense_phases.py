"""Where the cycles of a k step of the fused fc4 kernel (dense_tm<21, 8, 3, 2>) go, per wave (development tool; needs a
library built with -DCV_WG_STAMP -DCV_DENSE_PHASES: python tools/build_variant_lib.py dphases -DCV_WG_STAMP -DCV_DENSE_PHASES,
CV_HIP_LIB=clairvoyante_amd/csrc/libclairvoyante_hip_dphases.so; add -DCV_DENSE_RING=0 for the three-slot ring the
other dense_tm forms run).  python tools/gpu_dense_phases.py [batch]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from clairvoyante_amd import clairvoyante_v3, synth, _lib
n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
m = clairvoyante_v3.Clairvoyante(); m.setParameters(synth.bench_params("full"))
x = synth.make_candidates(n, seed=synth.BASE_SEED, device="cuda")
for _ in range(3):
    m.predict_device(x)
torch.cuda.synchronize()
lib = ctypes.CDLL(_lib.LIB_PATH)
buf = np.zeros(8 * 4096 * 4, dtype=np.uint64); cnt = np.zeros(8, dtype=np.uint32)
assert lib.cv_debug_wg_stamps(buf.ctypes.data_as(ctypes.c_void_p), cnt.ctypes.data_as(ctypes.c_void_p)) == 0
r = buf.reshape(8, 4096, 4)[6][:min(int(cnt[6]), 4096)]
assert len(r), "no records: is the library built with -DCV_WG_STAMP -DCV_DENSE_PHASES, and does the pass run the fused kernel?"
wave = (r[:, 3] & np.uint64(0xff)).astype(np.int64)
ph = r[:, :3].astype(np.float64)
tot = ph.sum(1)
steps = 288
print("batch %d: %d wave records of dense_tm<21, 8, 3, 2> (newest 4096 of %d), %d k steps each" % (n, len(r), int(cnt[6]), steps))
print("  loop cycles per wave (s_memtime): median %.0f  p10 %.0f  p90 %.0f   = %.0f per k step" % (
    np.median(tot), np.percentile(tot, 10), np.percentile(tot, 90), np.median(tot) / steps))
names = ("barrier exit -> first MFMA issued", "the MFMA block (first -> last MFMA issued)", "last MFMA issued -> barrier exit (counted wait + barrier)")
for i, nm in enumerate(names):
    print("  %-60s %6.4f of the loop   median %7.0f cycles = %6.1f per k step   (p10 %.1f  p90 %.1f)" % (
        nm, (ph[:, i] / tot).mean(), np.median(ph[:, i]), np.median(ph[:, i]) / steps,
        np.percentile(ph[:, i], 10) / steps, np.percentile(ph[:, i], 90) / steps))
for w in range(8):
    sel = wave == w
    if sel.any():
        print("  wave %d: barrier->MFMA %.4f  MFMA block %.4f  wait+barrier %.4f" % (w, *[(ph[sel, i] / tot[sel]).mean() for i in range(3)]))
# the ideal: 168 MFMAs x 32 cycles x 2 waves of a SIMD per k step
print("  MFMA issue of the two waves of a SIMD: %d cycles per k step (168 MFMAs x 32 x 2)" % (168 * 32 * 2))
m.close()
