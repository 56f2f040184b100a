// cv_draw_core.hpp -- the keyed draws of the training-set routes, one text for host and device (like cv_lz4_core.hpp).
//
// The reference samples with Python's unseeded `random`, one call per row in file order
// (ExtractVariantCandidates.py:203, PairWithNonVariants.py:119): nothing reproducible, and nothing a kernel could draw in
// parallel.  Here a draw is a function of WHAT is drawn, not of when: Philox4x32-10 (Salmon et al., "Parallel random
// numbers: as easy as 1, 2, 3", SC'11) with
//   key     = (seed lo32, seed hi32)
//   counter = (pos lo32, pos hi32, stream | late << 8, h)
// pos the 1-based coordinate of the row, h = FNV-1a-32 of the contig name's bytes, stream 0 = the gen4Training sample,
// 1 = the pairing with non-variants, 2 = RandomSampling's draw per position of a range (draws.RANDOM: keep if u <= prob),
// late = 1 for the second ("late") entry of a position in the candidate pass.
//   u = ((x0 << 32 | x1) >> 11) * 2^-53   in [0, 1), a double
// stream 0 keeps a row unless u > outputProb, stream 1 keeps it if u < r -- the reference's two comparisons.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CV_DRAW_FN __host__ __device__ static inline
#else
#define CV_DRAW_FN static inline
#endif

enum { CV_DRAW_SAMPLE = 0, CV_DRAW_PAIR = 1 };

CV_DRAW_FN uint32_t cv_fnv1a32(const uint8_t *s, int64_t n)
{
    uint32_t h = 2166136261u;
    for (int64_t i = 0; i < n; i++) { h ^= s[i]; h *= 16777619u; }
    return h;
}

CV_DRAW_FN void cv_philox4x32_10(uint32_t k0, uint32_t k1, const uint32_t ctr[4], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

CV_DRAW_FN double cv_draw(uint64_t seed, int stream, uint32_t h, int64_t pos, int late)
{
    const uint32_t ctr[4] = {(uint32_t)(uint64_t)pos, (uint32_t)((uint64_t)pos >> 32),
                             (uint32_t)stream | ((uint32_t)(late ? 1 : 0) << 8), h};
    uint32_t x[4];
    cv_philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), ctr, x);
    return (double)((((uint64_t)x[0] << 32) | x[1]) >> 11) * (1.0 / 9007199254740992.0);
}
