// cv_bamtrain.hip -- the labelled training set straight from the pileup (utils_v2.GetTrainingSetFromBam): the steps of
// the reference's recipe between "tensors exist" and "rows are labelled" (dataPrepScripts/PrepDataBeforeDemo.sh: the text
// rows of CreateTensor.py, PairWithNonVariants.py) as columns in HBM.  The sampling and the union of the centres live
// with the handle's state in cv_pileup.hip; everything behind these kernels is cv_trainset.hip (join, finish, gather).
//
//   bt_columns    one lane per centre, behind cv_pileup_finish: does CreateTensor.py print a row for it (:50-51), its
//                 coordinate and decimal length, the upper-cased reference base at the centre -> 0..3, "is one of ACGT"
//   bt_pair_count one lane per row of ALL sources: v = rows of truth centres, c = usable non-variants
//                 (PairWithNonVariants.py:50-86); integer sums only, so the order of the additions is no matter
//   bt_pair_keep  r = min(1, amp * v / c) from those two sums (c == 0: r = 1 -- the reference divides by zero there),
//                 keep = truth ? BED verdict : (BED verdict and stream-1 draw < r) (:93-122), then AND "centre is ACGT":
//                 the reader drops such a row only after the pairing (utils_v2.py:129-133), so it still counted in c
//
// A non-variant row at the key of a truth row (:81-82) cannot arise here: a centre is a truth centre exactly when its
// position is in the truth list inside the source's range, and every centre of a source lies inside that range -- so
// two rows with one key are both truth rows or both not.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_draw_core.hpp"
#include "cv_dev_common.hpp"

int cv_pileup_centres_dev(const cv_pileup *p, const int32_t **centres_dev, const uint8_t **flags_dev, const uint8_t **ref_dev,
                          int64_t *ref_first, int64_t *ref_len, int64_t *n);      // cv_pileup.hip

namespace {

constexpr int FLANK = CV_INPUT_H / 2;                        // 16
constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void bt_columns(int64_t n, const int32_t *centres, const uint8_t *cflags, const uint8_t *ref,
                                                      int64_t ref_first, int64_t ref_len, const int32_t *depth,
                                                      const uint8_t *touched, int64_t min_coverage, int64_t *pos, uint8_t *digits,
                                                      uint8_t *centre, uint8_t *acgt, uint8_t *flags, uint8_t *row)
{
    CV_GRID_STRIDE(i, n) {
        const int64_t c = centres[i];
        const int64_t ri = c - 1 - ref_first;                // the centre in the loaded reference
        const bool inside = ri - FLANK >= 0;                 // the window starts inside it (CreateTensor.py:50)
        unsigned b = ri >= 0 && ri < ref_len ? ref[ri] : 0u;
        if (b >= 'a' && b <= 'z') b -= 32;
        const uint8_t code = b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 255;
        int d = 0;
        for (int64_t v = c; v > 0; v /= 10) ++d;             // (a centre <= 0 has no canonical decimal: no key, no row kept)
        pos[i] = c;
        digits[i] = (uint8_t)d;
        centre[i] = code;
        acgt[i] = code != 255 ? 1 : 0;
        flags[i] = cflags ? cflags[i] : 0;
        row[i] = touched[i] && inside && (int64_t)depth[i] >= min_coverage ? 1 : 0;
    }
}

// adds the lanes' a / b into sums[ia] / sums[ib]: a wave-64 shuffle tree, then one integer atomic per wave
__device__ __forceinline__ void add_up(int a, int b, unsigned long long *sums, int ia, int ib)
{
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (a) atomicAdd(sums + ia, (unsigned long long)a);
        if (b) atomicAdd(sums + ib, (unsigned long long)b);
    }
}

__global__ __launch_bounds__(THREADS) void bt_pair_count(int64_t nrows, const uint8_t *flags, const uint8_t *keep,
                                                         unsigned long long *sums)
{
    int v = 0, c = 0;                                        // (<= 2^30 rows over 2^20 lanes: an int holds a lane's share)
    CV_GRID_STRIDE(r, nrows) {
        if (flags[r] & CV_CENTRE_TRUTH) ++v;                 // not BED-filtered (:50-62)
        else if (keep[r]) ++c;
    }
    add_up(v, c, sums, 0, 1);
}

__device__ __forceinline__ double pair_ratio(unsigned long long v, unsigned long long c, double amp)
{
    if (c == 0) return 1.0;
    const double r = ((double)v * amp) / (double)c;          // t = v * amp; r = float(t) / c (:65, :88)
    return r <= 1.0 ? r : 1.0;
}

__global__ __launch_bounds__(THREADS) void bt_pair_keep(int64_t nrows, const int32_t *ctg, const int64_t *pos, const uint8_t *flags,
                                                        const uint8_t *acgt, const uint32_t *ctg_hash, int32_t nctg, uint64_t seed,
                                                        double amp, uint8_t *keep, unsigned long long *sums, double *r_out)
{
    const double ratio = pair_ratio(sums[0], sums[1], amp);
    int picked = 0, final = 0;
    CV_GRID_STRIDE(r, nrows) {
        bool k = keep[r] != 0;
        if (k && !(flags[r] & CV_CENTRE_TRUTH)) {
            const int32_t c = ctg[r];
            k = c >= 0 && c < nctg && cv_draw(seed, CV_DRAW_PAIR, ctg_hash[c], pos[r], 0) < ratio;
            if (k) ++picked;
        }
        k = k && acgt[r];
        if (k) ++final;
        keep[r] = k ? 1 : 0;
    }
    add_up(picked, final, sums, 2, 3);
    if (blockIdx.x == 0 && threadIdx.x == 0) *r_out = ratio;
}

}  // namespace

extern "C" int cv_draws_host(uint64_t seed, int stream, uint32_t h, const int64_t *pos, const int32_t *late, int64_t n, double *out_u)
{
    if (n < 0 || (n > 0 && (!pos || !out_u))) { cv_set_error("cv_draws_host: bad argument"); return 1; }
    for (int64_t i = 0; i < n; i++) out_u[i] = cv_draw(seed, stream, h, pos[i], late ? late[i] : 0);
    return 0;
}

extern "C" int cv_bamtrain_columns(const cv_pileup *p, const int32_t *depth_dev, const uint8_t *touched_dev, int64_t min_coverage,
                                   int64_t *pos_dev, uint8_t *digits_dev, uint8_t *centre_dev, uint8_t *acgt_dev,
                                   uint8_t *flags_dev, uint8_t *row_dev, void *stream)
{
    const int32_t *centres;
    const uint8_t *cflags, *ref;
    int64_t ref_first, ref_len, n;
    if (cv_pileup_centres_dev(p, &centres, &cflags, &ref, &ref_first, &ref_len, &n)) return 1;
    if (n == 0) return 0;
    if (!depth_dev || !touched_dev || !pos_dev || !digits_dev || !centre_dev || !acgt_dev || !flags_dev || !row_dev) {
        cv_set_error("cv_bamtrain_columns: null argument");
        return 1;
    }
    if (((uintptr_t)pos_dev & 7) || ((uintptr_t)depth_dev & 3)) { cv_set_error("cv_bamtrain_columns: pos must be 8-byte, depth 4-byte aligned"); return 1; }
    hipLaunchKernelGGL(bt_columns, dim3(cv_grid_for(n)), dim3(THREADS), 0, (hipStream_t)stream, n, centres, cflags, ref, ref_first, ref_len,
                       depth_dev, touched_dev, min_coverage, pos_dev, digits_dev, centre_dev, acgt_dev, flags_dev, row_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_bamtrain_pair(int64_t nrows, const int32_t *ctg_dev, const int64_t *pos_dev, const uint8_t *flags_dev,
                                const uint8_t *acgt_dev, const uint32_t *ctg_hash_dev, int32_t nctg, uint64_t seed, double amp,
                                uint8_t *keep_dev, int64_t *counts_dev, double *r_dev, void *stream)
{
    if (nrows < 0 || nrows > CV_TRAINSET_MAX_ROWS) {
        cv_set_error("cv_bamtrain_pair: %lld rows out of range (0 .. %lld)", (long long)nrows, (long long)CV_TRAINSET_MAX_ROWS);
        return 1;
    }
    if (!counts_dev || !r_dev || ((uintptr_t)counts_dev & 7) || ((uintptr_t)r_dev & 7)) {
        cv_set_error("cv_bamtrain_pair: counts_dev / r_dev are null or not 8-byte aligned");
        return 1;
    }
    if (nrows > 0 && (!ctg_dev || !pos_dev || !flags_dev || !acgt_dev || !ctg_hash_dev || !keep_dev || nctg < 1 || ((uintptr_t)pos_dev & 7))) {
        cv_set_error("cv_bamtrain_pair: null argument, no contig, or pos not 8-byte aligned");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *sums = (unsigned long long *)counts_dev;
    CV_HIP(hipMemsetAsync(sums, 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(bt_pair_count, dim3(cv_grid_for(nrows)), dim3(THREADS), 0, st, nrows, flags_dev, (const uint8_t *)keep_dev, sums);
    hipLaunchKernelGGL(bt_pair_keep, dim3(cv_grid_for(nrows)), dim3(THREADS), 0, st, nrows, ctg_dev, pos_dev, flags_dev, acgt_dev,
                       ctg_hash_dev, nctg, seed, amp, keep_dev, sums, r_dev);
    CV_HIP(hipGetLastError());
    return 0;
}
