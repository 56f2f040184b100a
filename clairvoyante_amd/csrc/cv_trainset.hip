// cv_trainset.hip -- the labelled training set built on the device from the rows cv_parse_tensor_text_dev left in HBM
// (utils_v2.GetTrainingSetDevice; the host loop utils_v2.GetTrainingArray is the definition of the result).
//
//   per slab, behind the parser (rows named by an index list, like cv_text_gather_rows):
//   ts_tokens        one thread per row: the coordinate token -> int64 + number of digits (flag: not canonical decimal),
//                    the centre base of the sequence token -> 0..3, flag "the contig token differs byte for byte from the
//                    row before" (row 0: always), flag "sequence token holds ':' or a byte >= 0x80"
//   hipcub InclusiveSum over the run-start flags -> run[r] = index of the row's contig run inside the slab
//   ts_join          one thread per row: contig id of its run (a table the host filled from the run-start tokens), the
//                    BED test of _Intervals.hit (cvb::stab: upper bound on the sorted begins + running maximum of the ends), the
//                    index of (contig id, position) in the truth table
//
//   once, over all rows in arrival order:
//   ts_keys          key = rank(contig) << 48 | position * 10^(12 - digits) << 4 | digits: the order of sorted() over the
//                    strings "contig:position"; rows the BED test dropped get the largest key
//   hipcub SortPairs (stable) of (key, arrival index), ts_heads + ExclusiveSum: one entry per distinct key
//   ts_entries       entry e: src[e] = the LAST arrival with that key (X[key] = ... overwrites), first[e] = the FIRST one
//   ts_labels        Y[e] = the truth label, or HOM / REF / length 0 + the centre base of the first arrival
//   ts_gather        X_out[r] = X_all[src[perm[r]]], Y_out[r] = Y[perm[r]]  (perm: the shuffle; absent = identity)
//
// Byte and integer kernels: nothing here contracts, the label values 0 / 0.5 / 1 are exact in fp32.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"

#include "cv_dev_scan.hpp"
#include "cv_beditems_core.hpp"

namespace {

constexpr int NV = CV_INPUT_H * CV_INPUT_W * CV_INPUT_C;     // 528
constexpr int CENTRE = CV_INPUT_H / 2;                       // 16: the 17th character of the sequence token
constexpr int THREADS = 256;
constexpr uint64_t KEY_DROPPED = ~(uint64_t)0;

__global__ __launch_bounds__(THREADS) void ts_tokens(const uint8_t *text, const int64_t *meta, const int64_t *idx, int64_t nrows,
                                                     int64_t *pos, uint8_t *digits, uint8_t *centre, uint8_t *flags, int32_t *start)
{
    CV_GRID_STRIDE(r, nrows) {
        const int64_t *m = meta + (idx ? idx[r] : r) * 6;
        uint8_t f = 0;
        // coordinate: canonical decimal = digits only, no leading zero unless it is "0", at most 12 digits
        const uint8_t *p = text + m[2];
        const int64_t pl = m[3];
        int64_t v = 0;
        bool canon = pl >= 1 && pl <= CV_TRAINSET_MAX_DIGITS && !(pl > 1 && p[0] == '0');
        for (int64_t k = 0; canon && k < pl; k++) {
            const unsigned d = (unsigned)p[k] - '0';
            if (d > 9) canon = false;
            v = v * 10 + d;
        }
        if (!canon) { f |= CV_TRAINSET_BAD_COORD; v = 0; }
        // sequence: the centre base (the parser kept the row: it is one of ACGT in either case)
        const uint8_t *s = text + m[4];
        const int64_t sl = m[5];
        unsigned c = sl > CENTRE ? s[CENTRE] : 0u;
        if (c >= 'a' && c <= 'z') c -= 32;
        const uint8_t base = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 255;
        if (base == 255) f |= CV_TRAINSET_BAD_SEQ;
        for (int64_t k = 0; k < sl; k++)
            if (s[k] == ':' || s[k] >= 0x80) f |= CV_TRAINSET_BAD_SEQ;
        // contig: a run starts where the token differs from the row before
        bool differs = r == 0;
        if (!differs) {
            const int64_t *q = meta + (idx ? idx[r - 1] : r - 1) * 6;
            differs = q[1] != m[1];
            const uint8_t *a = text + m[0], *b = text + q[0];
            for (int64_t k = 0; !differs && k < m[1]; k++) differs = a[k] != b[k];
        }
        if (differs) f |= CV_TRAINSET_RUN_START;
        pos[r] = v;
        digits[r] = (uint8_t)(canon ? pl : 0);
        centre[r] = base;
        flags[r] = f;
        start[r] = differs ? 1 : 0;
    }
}

__global__ __launch_bounds__(THREADS) void ts_run_index(int32_t *run, int64_t nrows)
{
    // inclusive count of run starts -> index of the run (row 0 starts run 0)
    CV_GRID_STRIDE(r, nrows) run[r] -= 1;
}

__global__ __launch_bounds__(THREADS) void ts_join(int64_t nrows, const int32_t *run, const int32_t *run_ctg, int64_t nruns,
                                                   const int64_t *pos, int32_t ntab, int has_bed, const int64_t *bed_off,
                                                   const int64_t *bed_begin, const int64_t *bed_emax, const int64_t *truth_off,
                                                   const int64_t *truth_pos, int32_t *ctg, uint8_t *keep, int32_t *truth)
{
    CV_GRID_STRIDE(r, nrows) {
        const int32_t k = run[r];
        const int32_t c = k >= 0 && k < nruns ? run_ctg[k] : -1;
        const int64_t p = pos[r];
        const bool tabled = c >= 0 && c < ntab;              // (a contig first seen in the tensor file has no table rows)
        bool kp = c >= 0;
        if (has_bed) {
            kp = false;
            if (tabled) {
                const int64_t lo = bed_off[c], n = bed_off[c + 1] - lo;
                kp = cvb::stab(bed_begin + lo, bed_emax + lo, n, p);
            }
        }
        int32_t t = -1;
        if (tabled && truth_off) {
            const int64_t lo = truth_off[c], n = truth_off[c + 1] - lo;
            const int64_t u = cvb::upper_bound(truth_pos + lo, n, p);
            if (u > 0 && truth_pos[lo + u - 1] == p) t = (int32_t)(lo + u - 1);
        }
        ctg[r] = c;
        keep[r] = kp ? 1 : 0;
        truth[r] = t;
    }
}

__device__ const int64_t ts_pow10[13] = {1ll, 10ll, 100ll, 1000ll, 10000ll, 100000ll, 1000000ll, 10000000ll, 100000000ll,
                                         1000000000ll, 10000000000ll, 100000000000ll, 1000000000000ll};

__global__ __launch_bounds__(THREADS) void ts_keys(int64_t nrows, const int32_t *ctg, const int64_t *pos, const uint8_t *digits,
                                                   const uint8_t *keep, const int32_t *rank, int32_t nctg, uint64_t *key, int64_t *val)
{
    CV_GRID_STRIDE(r, nrows) {
        const int32_t c = ctg[r];
        const int d = digits[r];
        uint64_t k = KEY_DROPPED;
        if (keep[r] && c >= 0 && c < nctg && d >= 1 && d <= CV_TRAINSET_MAX_DIGITS)
            k = (uint64_t)(uint32_t)rank[c] << 48 | (uint64_t)(pos[r] * ts_pow10[CV_TRAINSET_MAX_DIGITS - d]) << 4 | (uint64_t)d;
        key[r] = k;
        val[r] = r;
    }
}

__global__ __launch_bounds__(THREADS) void ts_heads(int64_t nrows, const uint64_t *key, int32_t *head)
{
    CV_GRID_STRIDE(j, nrows + 1)
        head[j] = j < nrows && key[j] != KEY_DROPPED && (j == 0 || key[j] != key[j - 1]) ? 1 : 0;   // (slot nrows: its scanned value is the total)
}

__global__ __launch_bounds__(THREADS) void ts_entries(int64_t nrows, const uint64_t *key, const int64_t *val, const int32_t *head,
                                                      const int32_t *before, int64_t *src, int64_t *first, int64_t *total)
{
    CV_GRID_STRIDE(j, nrows) {
        if (key[j] == KEY_DROPPED) continue;
        const int64_t e = (int64_t)before[j] + head[j] - 1;          // the entry this sorted slot belongs to
        if (head[j]) first[e] = val[j];                              // (stable sort: the lowest arrival index comes first)
        if (j + 1 == nrows || key[j + 1] != key[j]) src[e] = val[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *total = before[nrows];
}

__global__ __launch_bounds__(THREADS) void ts_labels(const int32_t *before, int64_t nrows, const int64_t *src, const int64_t *first,
                                                     const int32_t *truth, const uint8_t *centre, const float *labels,
                                                     int64_t ntruth, float *y)
{
    const int64_t total = before[nrows];
    CV_GRID_STRIDE(i, total * 16) {
        const int64_t e = i >> 4;
        const int k = (int)(i & 15);
        const int32_t t = truth[src[e]];
        float v;
        if (t >= 0 && t < ntruth) v = labels[(int64_t)t * 16 + k];
        else v = (k == 5 || k == 6 || k == 10 || k == (int)centre[first[e]]) ? 1.0f : 0.0f;      // HOM, REF, length 0, the base
        y[i] = v;
    }
}

__global__ void ts_zero_total(int64_t *total) { if (!blockIdx.x && !threadIdx.x) *total = 0; }

__global__ __launch_bounds__(THREADS) void ts_gather(const float4 *x_all, const float4 *y, const int64_t *src, const int64_t *perm,
                                                     int64_t total, float4 *x_out, float4 *y_out)
{
    constexpr int XQ = NV / 4, Q = XQ + 4;                   // 16-byte pieces of one item: its row and its label
    CV_GRID_STRIDE(e, total * Q) {
        const int64_t r = e / Q;
        const int c = (int)(e - r * Q);
        const int64_t from = perm ? perm[r] : r;
        if (c < XQ) x_out[r * XQ + c] = x_all[src[from] * XQ + c];
        else y_out[r * 4 + (c - XQ)] = y[from * 4 + (c - XQ)];
    }
}

struct finish_ws {
    uint64_t *key_in, *key_out;
    int64_t *val_in, *val_out;
    int32_t *head, *before;
    int64_t *first;
    void *tmp;
    size_t tmp_bytes;
};

int finish_plan(cv_carver &c, int64_t nrows, finish_ws *W)
{
    const size_t n = (size_t)(nrows > 0 ? nrows : 1);
    size_t a = 0, b = 0;
    W->key_in = c.take<uint64_t>(n);
    W->key_out = c.take<uint64_t>(n);
    W->val_in = c.take<int64_t>(n);
    W->val_out = c.take<int64_t>(n);
    W->head = c.take<int32_t>(n + 1);
    W->before = c.take<int32_t>(n + 1);
    W->first = c.take<int64_t>(n);
    if (cv_sort_pairs_temp_bytes<uint64_t, int64_t>(n, &a) || cv_scan_temp_bytes<int32_t>(n + 1, &b)) return 1;
    W->tmp_bytes = a > b ? a : b;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

struct tokens_ws {
    int32_t *start;
    void *tmp;
    size_t tmp_bytes;
};

int tokens_plan(cv_carver &c, int64_t nrows, tokens_ws *W)
{
    const size_t n = (size_t)(nrows > 0 ? nrows : 1);
    W->start = c.take<int32_t>(n);
    if (cv_inclusive_sum_temp_bytes<int32_t>(n, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool rows_ok(const char *who, int64_t nrows)
{
    if (nrows < 0 || nrows > CV_TRAINSET_MAX_ROWS) {
        cv_set_error("%s: %lld rows out of range (0 .. %lld)", who, (long long)nrows, (long long)CV_TRAINSET_MAX_ROWS);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int cv_trainset_tokens_workspace(int64_t nrows, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_trainset_tokens_workspace: null argument"); return 1; }
    if (!rows_ok("cv_trainset_tokens_workspace", nrows)) return 1;
    cv_carver c;
    tokens_ws W;
    if (tokens_plan(c, nrows, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_trainset_tokens(const char *text_dev, const int64_t *meta_dev, const int64_t *index_dev, int64_t nrows,
                                  int64_t *pos_dev, uint8_t *digits_dev, uint8_t *centre_dev, uint8_t *flags_dev,
                                  int32_t *run_dev, void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    if (!rows_ok("cv_trainset_tokens", nrows)) return 1;
    if (nrows == 0) return 0;
    if (!text_dev || !meta_dev || !pos_dev || !digits_dev || !centre_dev || !flags_dev || !run_dev || !workspace_dev) {
        cv_set_error("cv_trainset_tokens: null argument");
        return 1;
    }
    if (((uintptr_t)meta_dev & 7) || ((uintptr_t)index_dev & 7) || ((uintptr_t)pos_dev & 7) || ((uintptr_t)run_dev & 3)) {
        cv_set_error("cv_trainset_tokens: meta / index / pos must be 8-byte, run 4-byte aligned");
        return 1;
    }
    cv_carver c(workspace_dev);
    tokens_ws W;
    if (tokens_plan(c, nrows, &W)) return 1;
    if (!cv_workspace_ok("cv_trainset_tokens", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    int32_t *start = W.start;
    size_t tb = W.tmp_bytes;
    hipLaunchKernelGGL(ts_tokens, dim3(cv_grid_for(nrows)), dim3(THREADS), 0, st, (const uint8_t *)text_dev, meta_dev, index_dev, nrows,
                       pos_dev, digits_dev, centre_dev, flags_dev, start);
    CV_HIP(hipcub::DeviceScan::InclusiveSum(W.tmp, tb, (const int32_t *)start, run_dev, (int)nrows, st));
    hipLaunchKernelGGL(ts_run_index, dim3(cv_grid_for(nrows)), dim3(THREADS), 0, st, run_dev, nrows);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_trainset_join(int64_t nrows, const int32_t *run_dev, const int32_t *run_ctg_dev, int64_t nruns,
                                const int64_t *pos_dev, int32_t ntab, int has_bed, const int64_t *bed_off_dev,
                                const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, const int64_t *truth_off_dev,
                                const int64_t *truth_pos_dev, int32_t *ctg_dev, uint8_t *keep_dev, int32_t *truth_dev, void *stream)
{
    if (!rows_ok("cv_trainset_join", nrows)) return 1;
    if (nrows == 0) return 0;
    if (!run_dev || !run_ctg_dev || !pos_dev || !ctg_dev || !keep_dev || !truth_dev || nruns < 1 || ntab < 0) {
        cv_set_error("cv_trainset_join: null argument, or no run / a negative table size");
        return 1;
    }
    if (has_bed && ntab > 0 && (!bed_off_dev || !bed_begin_dev || !bed_emax_dev)) {
        cv_set_error("cv_trainset_join: has_bed without the BED tables");
        return 1;
    }
    if (truth_off_dev && !truth_pos_dev) { cv_set_error("cv_trainset_join: truth_off_dev without truth_pos_dev"); return 1; }
    hipLaunchKernelGGL(ts_join, dim3(cv_grid_for(nrows)), dim3(THREADS), 0, (hipStream_t)stream, nrows, run_dev, run_ctg_dev, nruns,
                       pos_dev, ntab, has_bed, bed_off_dev, bed_begin_dev, bed_emax_dev, truth_off_dev, truth_pos_dev, ctg_dev,
                       keep_dev, truth_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_trainset_finish_workspace(int64_t nrows, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_trainset_finish_workspace: null argument"); return 1; }
    if (!rows_ok("cv_trainset_finish_workspace", nrows)) return 1;
    cv_carver c;
    finish_ws W;
    if (finish_plan(c, nrows, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_trainset_finish(int64_t nrows, const int32_t *ctg_dev, const int64_t *pos_dev, const uint8_t *digits_dev,
                                  const uint8_t *centre_dev, const uint8_t *keep_dev, const int32_t *truth_dev,
                                  const int32_t *rank_dev, int32_t nctg, const float *labels_dev, int64_t ntruth,
                                  int64_t *src_dev, float *y_dev, int64_t *total_dev, void *workspace_dev,
                                  int64_t workspace_bytes, void *stream)
{
    if (!rows_ok("cv_trainset_finish", nrows)) return 1;
    if (!total_dev || ((uintptr_t)total_dev & 7)) { cv_set_error("cv_trainset_finish: total_dev is null or not 8-byte aligned"); return 1; }
    hipStream_t st = (hipStream_t)stream;
    if (nrows == 0) {
        hipLaunchKernelGGL(ts_zero_total, dim3(1), dim3(64), 0, st, total_dev);
        CV_HIP(hipGetLastError());
        return 0;
    }
    if (!ctg_dev || !pos_dev || !digits_dev || !centre_dev || !keep_dev || !truth_dev || !rank_dev || !src_dev || !y_dev ||
        !workspace_dev || nctg < 1 || nctg > CV_TRAINSET_MAX_CONTIGS || ntruth < 0 || (ntruth > 0 && !labels_dev)) {
        cv_set_error("cv_trainset_finish: null argument, or contig / truth counts out of range (1 .. %d contigs)", CV_TRAINSET_MAX_CONTIGS);
        return 1;
    }
    if (((uintptr_t)pos_dev & 7) || ((uintptr_t)src_dev & 7) || ((uintptr_t)y_dev & 3)) {
        cv_set_error("cv_trainset_finish: pos / src must be 8-byte, y 4-byte aligned");
        return 1;
    }
    cv_carver c(workspace_dev);
    finish_ws W;
    if (finish_plan(c, nrows, &W)) return 1;
    if (!cv_workspace_ok("cv_trainset_finish", workspace_dev, workspace_bytes, c.total())) return 1;
    uint64_t *key_in = W.key_in, *key_out = W.key_out;
    int64_t *val_in = W.val_in, *val_out = W.val_out, *first = W.first;
    int32_t *head = W.head, *before = W.before;
    const int grid = cv_grid_for(nrows + 1);
    hipLaunchKernelGGL(ts_keys, dim3(grid), dim3(THREADS), 0, st, nrows, ctg_dev, pos_dev, digits_dev, keep_dev, rank_dev, nctg, key_in, val_in);
    size_t tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, (const uint64_t *)key_in, key_out, (const int64_t *)val_in, val_out,
                                              (int)nrows, 0, 64, st));
    hipLaunchKernelGGL(ts_heads, dim3(grid), dim3(THREADS), 0, st, nrows, (const uint64_t *)key_out, head);
    tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)head, before, (int)(nrows + 1), st));
    hipLaunchKernelGGL(ts_entries, dim3(grid), dim3(THREADS), 0, st, nrows, (const uint64_t *)key_out, (const int64_t *)val_out,
                       (const int32_t *)head, (const int32_t *)before, src_dev, first, total_dev);
    hipLaunchKernelGGL(ts_labels, dim3(cv_grid_for(nrows * 16)), dim3(THREADS), 0, st, (const int32_t *)before, nrows,
                       (const int64_t *)src_dev, (const int64_t *)first, truth_dev, centre_dev, labels_dev, ntruth, y_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_trainset_gather(const float *x_all_dev, const float *y_dev, const int64_t *src_dev, const int64_t *perm_dev,
                                  int64_t total, float *x_out_dev, float *y_out_dev, void *stream)
{
    if (!rows_ok("cv_trainset_gather", total)) return 1;
    if (total == 0) return 0;
    if (!x_all_dev || !y_dev || !src_dev || !x_out_dev || !y_out_dev) { cv_set_error("cv_trainset_gather: null argument"); return 1; }
    if (((uintptr_t)x_all_dev & 15) || ((uintptr_t)y_dev & 15) || ((uintptr_t)x_out_dev & 15) || ((uintptr_t)y_out_dev & 15) ||
        ((uintptr_t)src_dev & 7) || ((uintptr_t)perm_dev & 7)) {
        cv_set_error("cv_trainset_gather: the tensors must be 16-byte, the index lists 8-byte aligned");
        return 1;
    }
    hipLaunchKernelGGL(ts_gather, dim3(cv_grid_for(total * (NV / 4 + 4))), dim3(THREADS), 0, (hipStream_t)stream, (const float4 *)x_all_dev,
                       (const float4 *)y_dev, src_dev, perm_dev, total, (float4 *)x_out_dev, (float4 *)y_out_dev);
    CV_HIP(hipGetLastError());
    return 0;
}
