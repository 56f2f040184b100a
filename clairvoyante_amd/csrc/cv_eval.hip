// cv_eval.hip -- device side of the evaluation report (train.EvaluateReport; the reference's evaluate.py:78-107):
// network outputs and labels of a pass in, 59 counters out.
//
//   eval_counts   one thread per candidate, grid-stride: the truth index of every head (np.argmax of the label columns, in
//                 the labels' own type), the two best bases of the sigmoid head (argsort(kind="stable")[::-1]) and the
//                 arg-maxes of the three softmax heads; top-1 / top-2 hits are counted per wave from ballots, the cells of
//                 the three confusion matrices in a 64-entry int32 histogram in LDS; at its end a workgroup adds its
//                 non-zero entries to the caller's int64 counters, one 64-bit integer atomic each.  Integer sums do not
//                 depend on the order of arrival: the counters are the same from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_dev_common.hpp"

namespace {

constexpr int EV_THREADS = 256;
// One workgroup per CU at most.  The drivers call once per pass of at most 65 536 candidates = 256 workgroups, so the cap
// only bounds what a direct caller with a larger n launches (it then walks n in strides of 65 536); a workgroup would have
// to count 2^31 candidates before an int32 entry of its histogram wrapped -- n beyond 2^39, 35 TB of outputs.
constexpr int EV_GRID = 256;

// np.argmax over v[0..CNT): the first NaN, else the first maximum
template <int CNT, typename T>
__device__ __forceinline__ int first_max(const T *v)
{
    int am = 0;
    T best = v[0];
#pragma unroll
    for (int k = 1; k < CNT; k++) {
        const T w = v[k];
        if (best == best && (w != w || w > best)) { am = k; best = w; }
    }
    return am;
}

// row i of a [n,16] array through 16-byte loads: 4 for fp32 (outputs, labels), 8 for float64 (labels)
__device__ __forceinline__ void load_row16(const float *y, int64_t i, float *v)
{
    const float4 *p = reinterpret_cast<const float4 *>(y) + i * 4;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float4 t = p[q];
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
}

__device__ __forceinline__ void load_row16(const double *y, int64_t i, double *v)
{
    const double2 *p = reinterpret_cast<const double2 *>(y) + i * 8;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const double2 t = p[q];
        v[2 * q] = t.x; v[2 * q + 1] = t.y;
    }
}

template <typename YT>
__global__ __launch_bounds__(EV_THREADS) void eval_counts(const float *__restrict__ out16, const YT *__restrict__ y, int64_t n,
                                                          unsigned long long *__restrict__ counts)
{
    __shared__ int hist[CV_EVAL_COUNTS];
    if (threadIdx.x < CV_EVAL_COUNTS) hist[threadIdx.x] = 0;
    __syncthreads();
    int cand = 0, top1 = 0, top2 = 0;              // of this wave (the same value in every lane)
    const int64_t stride = (int64_t)gridDim.x * EV_THREADS;
    // (the loop bound is the same for the whole workgroup: every lane reaches the ballots)
    for (int64_t first = (int64_t)blockIdx.x * EV_THREADS; first < n; first += stride) {
        const int64_t i = first + threadIdx.x;
        const bool live = i < n;
        bool hit1 = false, hit2 = false;
        if (live) {
            float o[16];
            YT t[16];
            load_row16(out16, i, o);
            load_row16(y, i, t);
            // base change: position 0 and 1 of argsort(kind="stable")[::-1] -- descending, NaN above every number, among
            // equal values (NaN and NaN, +0 and -0) the HIGHER index first.  `ahead(v, w)`: v, met after w, goes before it.
            auto ahead = [](float v, float w) { return v != v || (w == w && v >= w); };
            int b1 = 0, b2 = -1;
            float v1 = o[0], v2 = 0.0f;
#pragma unroll
            for (int k = 1; k < 4; k++) {
                const float w = o[k];
                if (ahead(w, v1)) { b2 = b1; v2 = v1; b1 = k; v1 = w; }
                else if (b2 < 0 || ahead(w, v2)) { b2 = k; v2 = w; }
            }
            const int tb = first_max<4>(t);
            hit1 = tb == b1;
            hit2 = hit1 || tb == b2;
            atomicAdd(&hist[CV_EVAL_ZYGOSITY + first_max<2>(t + 4) * 2 + first_max<2>(o + 4)], 1);
            atomicAdd(&hist[CV_EVAL_VARTYPE + first_max<4>(t + 6) * 4 + first_max<4>(o + 6)], 1);
            atomicAdd(&hist[CV_EVAL_INDEL + first_max<6>(t + 10) * 6 + first_max<6>(o + 10)], 1);
        }
        cand += __popcll(__ballot(live));
        top1 += __popcll(__ballot(hit1));
        top2 += __popcll(__ballot(hit2));
    }
    if ((threadIdx.x & 63) == 0) {
        if (cand) atomicAdd(&hist[CV_EVAL_ALL], cand);
        if (top1) atomicAdd(&hist[CV_EVAL_TOP1], top1);
        if (top2) atomicAdd(&hist[CV_EVAL_TOP2], top2);
    }
    __syncthreads();
    if (threadIdx.x < CV_EVAL_COUNTS) {
        const int v = hist[threadIdx.x];
        if (v) atomicAdd(&counts[threadIdx.x], (unsigned long long)v);
    }
}

}  // namespace

extern "C" int cv_eval_counts(const float *out16_dev, const void *y_dev, int y_is_f64, int64_t n, int64_t *counts_dev,
                              void *stream)
{
    if (n < 0) { cv_set_error("cv_eval_counts: negative candidate count"); return 1; }
    if (n == 0) return 0;
    if (!out16_dev || !y_dev || !counts_dev) { cv_set_error("cv_eval_counts: null argument"); return 1; }
    if (((uintptr_t)out16_dev & 15) || ((uintptr_t)y_dev & 15) || ((uintptr_t)counts_dev & 7)) {
        cv_set_error("cv_eval_counts: the outputs and the labels must be 16-byte, the counters 8-byte aligned");
        return 1;
    }
    const int64_t blocks = (n + EV_THREADS - 1) / EV_THREADS;
    const dim3 grid((unsigned)(blocks < EV_GRID ? blocks : EV_GRID));
    unsigned long long *c = reinterpret_cast<unsigned long long *>(counts_dev);
    if (y_is_f64)
        hipLaunchKernelGGL(eval_counts<double>, grid, dim3(EV_THREADS), 0, (hipStream_t)stream, out16_dev,
                           (const double *)y_dev, n, c);
    else
        hipLaunchKernelGGL(eval_counts<float>, grid, dim3(EV_THREADS), 0, (hipStream_t)stream, out16_dev,
                           (const float *)y_dev, n, c);
    CV_HIP(hipGetLastError());
    return 0;
}
