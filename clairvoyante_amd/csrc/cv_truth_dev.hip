// cv_truth_dev.hip -- the truth list (or truth VCF: GetTruth's rules, one source per call) and the BED file of the
// training-set builders read on the device: from a slab of their text in HBM to the tables
// utils_v2._trainset_tables(*utils_v2._read_bed_truth(...)) returns.  The host loop stays the definition;
// cv_truth_core.hpp says per line whether the device vouches for it (ROW / SKIP) or not (HOST).
//
//   per slab (cv_truth_lines_dev):
//   newline index       cv_text_line_index of cv_textparse.hip
//   tl_verdicts         one thread per line: the core's status and the contig token's span
//   run-start flags     cv_text_run_flags of cv_textparse.hip: "this ROW's contig token differs byte for byte from the line
//                       before" (or that line is no ROW)
//   hipcub ExclusiveSum over the ROW flags and over the run-start flags -> row index, run index
//   tl_rows             the core again for the ROW lines: fields at their row index, run-start token spans at their run index,
//                       the counters
//
//   once over the intervals of all slabs (cv_bed_table_dev):
//   two stable radix sorts, by end and then by (contig id, begin) = sorted() over the (begin, end) tuples of each contig;
//   the running maximum of the ends within a contig is ONE hipcub InclusiveScan(Max) over contig id << 41 | end + 1
//   (the contig ids ascend, so a later contig's values exceed every earlier one's)
//
//   once over the truth rows of all slabs (cv_truth_tables_dev):
//   one stable sort by (contig id, position); the tail of each run of equal keys is the dict's "last row wins"; the BED
//   verdict is cvb::stab, as in ts_join of cv_trainset.hip; hipcub ExclusiveSum over "tail" and over "tail and kept";
//   the offsets per contig from a lower bound on the sorted keys.
//
// Integer and byte kernels; every output slot has exactly one writer and the counters are integer sums, so no result
// depends on the order of the launches' blocks.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <string.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_internal.hpp"
#include "cv_dev_scan.hpp"
#include "cv_beditems_core.hpp"
#include "cv_truth_core.hpp"

namespace {

constexpr int THREADS = 256;
constexpr int POS_BITS = 40;                                  // a canonical coordinate has 12 digits at most: < 2^40
constexpr int END_BITS = 41;                                  // end + 1 of a BED interval: 0 .. 10^12

// ---- the line pass ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void tl_verdicts(const uint8_t *text, const int64_t *line_end, const int64_t *index_info,
                                                       int64_t max_lines, int format, const cvt::Filter filter, uint8_t *status, int64_t *span,
                                                       int32_t *isrow, int64_t *info)
{
    const int64_t lines = index_info[1];
    CV_GRID_STRIDE(i, max_lines + 1) {
        int row = 0;
        if (i < lines) {
            const int64_t start = i ? line_end[i - 1] + 1 : 0;
            cvt::Line L;
            cvt::verdict(text + start, line_end[i] - start, format, &filter, false, &L);
            status[i] = (uint8_t)L.status;
            span[2 * i] = start + L.ctg_off;
            span[2 * i + 1] = L.ctg_len;
            row = L.status == cvt::ROW;
            if (!row) atomicAdd((unsigned long long *)&info[L.status == cvt::SKIP ? 3 : 4], 1ull);
        }
        isrow[i] = row;
    }
}

__global__ __launch_bounds__(THREADS) void tl_rows(const uint8_t *text, const int64_t *line_end, const int64_t *index_info,
                                                   int64_t max_lines, int format, const cvt::Filter filter, const int32_t *isrow, const int32_t *rowidx,
                                                   const int32_t *flag, const int32_t *runidx, const int64_t *span, int64_t *pos,
                                                   int64_t *end, float *label, int32_t *run, int64_t *tok, int64_t *info)
{
    const int64_t lines = index_info[1];
    CV_GRID_STRIDE(i, lines) {
        if (!isrow[i]) continue;
        const int64_t start = i ? line_end[i - 1] + 1 : 0;
        cvt::Line L;
        cvt::verdict(text + start, line_end[i] - start, format, &filter, true, &L);
        const int64_t r = rowidx[i];
        pos[r] = L.pos;
        if (format == cvt::FMT_BED) end[r] = L.end;
        else
            for (int k = 0; k < 16; ++k) label[r * 16 + k] = L.label[k];
        run[r] = runidx[i] + flag[i] - 1;
        if (flag[i]) { tok[2 * (int64_t)runidx[i]] = span[2 * i]; tok[2 * (int64_t)runidx[i] + 1] = span[2 * i + 1]; }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        info[0] = index_info[0];
        info[1] = lines;
        info[2] = rowidx[max_lines];
        info[5] = runidx[max_lines];
    }
}

struct lines_ws {
    void *index;
    int64_t *index_info, *span;
    uint8_t *status;
    int32_t *isrow, *rowidx, *flag, *runidx;
    void *tmp;
    size_t tmp_bytes;
};

int lines_plan(cv_carver &c, int64_t len, int64_t max_lines, lines_ws *W)
{
    const size_t n = (size_t)max_lines + 1;
    size_t ib = 0;
    if (cv_text_line_index_bytes(len, max_lines, &ib)) return 1;
    W->index = c.take_bytes(ib);
    W->index_info = c.take<int64_t>(4);
    W->status = c.take<uint8_t>(n);
    W->span = c.take<int64_t>(2 * n);
    W->isrow = c.take<int32_t>(n);
    W->rowidx = c.take<int32_t>(n);
    W->flag = c.take<int32_t>(n);
    W->runidx = c.take<int32_t>(n);
    if (cv_scan_temp_bytes<int32_t>(n, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool lines_args_ok(const char *who, int64_t len, int format, int64_t max_lines)
{
    if (len < 0 || len > CV_TEXT_SLAB_MAX || max_lines < 0 || max_lines > CV_TRUTH_MAX_LINES ||
        (format != CV_TRUTH_FORMAT_VAR && format != CV_TRUTH_FORMAT_BED && format != CV_TRUTH_FORMAT_VCF)) {
        cv_set_error("%s: len %lld / max_lines %lld / format %d out of range (0 .. %lld bytes, 0 .. %lld lines, format %d, %d or %d)", who,
                     (long long)len, (long long)max_lines, format, (long long)CV_TEXT_SLAB_MAX, (long long)CV_TRUTH_MAX_LINES,
                     CV_TRUTH_FORMAT_VAR, CV_TRUTH_FORMAT_BED, CV_TRUTH_FORMAT_VCF);
        return false;
    }
    return true;
}

// the source of format VCF from the caller's arguments (any other format: all zero)
bool filter_of(const char *who, int format, const char *ctg, int64_t ctg_len, int has_bounds, int64_t lo, int64_t hi, cvt::Filter *f)
{
    memset(f, 0, sizeof *f);
    if (format != CV_TRUTH_FORMAT_VCF) return true;
    if (!ctg || ctg_len < 1 || ctg_len > CV_TRUTH_MAX_CTG) {
        cv_set_error("%s: format VCF needs the wanted contig's name, 1 .. %d bytes", who, CV_TRUTH_MAX_CTG);
        return false;
    }
    f->has_bounds = has_bounds ? 1 : 0; f->lo = lo; f->hi = hi; f->ctg_len = ctg_len;
    memcpy(f->ctg, ctg, (size_t)ctg_len);
    return true;
}

// ---- the tables ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ctg_of(const int32_t *run, const int32_t *run_ctg, int64_t nruns, int64_t i)
{
    const int32_t k = run[i];
    const int32_t c = k >= 0 && k < nruns ? run_ctg[k] : 0;
    return (uint64_t)(c >= 0 && c < CV_TRAINSET_MAX_CONTIGS ? c : 0);
}

__global__ __launch_bounds__(THREADS) void bt_end_keys(int64_t n, const int64_t *end, uint64_t *key, int64_t *val)
{
    CV_GRID_STRIDE(i, n) { key[i] = (uint64_t)(end[i] + 1); val[i] = i; }
}

__global__ __launch_bounds__(THREADS) void bt_begin_keys(int64_t n, const int64_t *by_end, const int64_t *begin, const int32_t *run,
                                                         const int32_t *run_ctg, int64_t nruns, uint64_t *key)
{
    CV_GRID_STRIDE(j, n) { const int64_t i = by_end[j]; key[j] = ctg_of(run, run_ctg, nruns, i) << POS_BITS | (uint64_t)begin[i]; }
}

__global__ __launch_bounds__(THREADS) void bt_gather(int64_t n, const uint64_t *key, const int64_t *order, const int64_t *end,
                                                     int64_t *bed_begin, uint64_t *packed)
{
    CV_GRID_STRIDE(j, n) {
        bed_begin[j] = (int64_t)(key[j] & (((uint64_t)1 << POS_BITS) - 1));
        packed[j] = (key[j] >> POS_BITS) << END_BITS | (uint64_t)(end[order[j]] + 1);
    }
}

__global__ __launch_bounds__(THREADS) void bt_finish(int64_t n, const uint64_t *key, const uint64_t *packed_max, int32_t nctg,
                                                     int64_t *bed_emax, int64_t *bed_off)
{
    CV_GRID_STRIDE(j, n) bed_emax[j] = (int64_t)(packed_max[j] & (((uint64_t)1 << END_BITS) - 1)) - 1;
    CV_GRID_STRIDE(c, (int64_t)nctg + 1) bed_off[c] = c == nctg ? n : cvb::lower_bound(key, n, (uint64_t)c << POS_BITS);
}

struct bed_ws {
    uint64_t *key_a, *key_b;
    int64_t *val_a, *val_b;
    void *tmp;
    size_t tmp_bytes;
};

int bed_plan(cv_carver &c, int64_t n, bed_ws *W)
{
    const size_t m = (size_t)(n > 0 ? n : 1);
    size_t a = 0, b = 0;
    W->key_a = c.take<uint64_t>(m);
    W->key_b = c.take<uint64_t>(m);
    W->val_a = c.take<int64_t>(m);
    W->val_b = c.take<int64_t>(m);
    if (cv_sort_pairs_temp_bytes<uint64_t, int64_t>(m, &a) || cv_max_scan_temp_bytes<uint64_t>(m, &b)) return 1;
    W->tmp_bytes = a > b ? a : b;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

__global__ __launch_bounds__(THREADS) void tt_keys(int64_t n, const int64_t *pos, const int32_t *run, const int32_t *run_ctg,
                                                   int64_t nruns, uint64_t *key, int64_t *val)
{
    CV_GRID_STRIDE(i, n) { key[i] = ctg_of(run, run_ctg, nruns, i) << POS_BITS | (uint64_t)pos[i]; val[i] = i; }
}

__global__ __launch_bounds__(THREADS) void tt_tails(int64_t n, const uint64_t *key, int32_t nctg, int has_bed, const int64_t *bed_off,
                                                    const int64_t *bed_begin, const int64_t *bed_emax, int32_t *every, int32_t *kept)
{
    CV_GRID_STRIDE(j, n + 1) {
        int tail = 0, kp = 0;
        if (j < n && (j + 1 == n || key[j + 1] != key[j])) {
            tail = 1;
            kp = 1;
            if (has_bed) {                                       // _Intervals.hit
                const int64_t c = (int64_t)(key[j] >> POS_BITS), p = (int64_t)(key[j] & (((uint64_t)1 << POS_BITS) - 1));
                kp = 0;
                if (c < nctg) {
                    const int64_t lo = bed_off[c], m = bed_off[c + 1] - lo;
                    kp = cvb::stab(bed_begin + lo, bed_emax + lo, m, p);
                }
            }
        }
        every[j] = tail;
        kept[j] = kp;
    }
}

__global__ __launch_bounds__(THREADS) void tt_emit(int64_t n, const uint64_t *key, const int64_t *val, const int32_t *every,
                                                   const int32_t *every_at, const int32_t *kept, const int32_t *kept_at,
                                                   const float4 *label, int32_t nctg, int64_t *truth_off, int64_t *truth_pos,
                                                   float4 *labels_out, int64_t *every_off, int64_t *every_pos, int64_t *counts)
{
    CV_GRID_STRIDE(j, n) {
        if (!every[j]) continue;
        const int64_t p = (int64_t)(key[j] & (((uint64_t)1 << POS_BITS) - 1));
        every_pos[every_at[j]] = p;
        if (kept[j]) {
            const int64_t t = kept_at[j], i = val[j];            // (stable sort: the tail is the LAST arrival of the key)
            truth_pos[t] = p;
            for (int q = 0; q < 4; ++q) labels_out[t * 4 + q] = label[i * 4 + q];
        }
    }
    CV_GRID_STRIDE(c, (int64_t)nctg + 1) {
        const int64_t lb = c == nctg ? n : cvb::lower_bound(key, n, (uint64_t)c << POS_BITS);
        truth_off[c] = kept_at[lb];
        every_off[c] = every_at[lb];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { counts[0] = kept_at[n]; counts[1] = every_at[n]; }
}

struct tables_ws {
    uint64_t *key_a, *key_b;
    int64_t *val_a, *val_b;
    int32_t *every, *every_at, *kept, *kept_at;
    void *tmp;
    size_t tmp_bytes;
};

int tables_plan(cv_carver &c, int64_t n, tables_ws *W)
{
    const size_t m = (size_t)(n > 0 ? n : 1);
    size_t a = 0, b = 0;
    W->key_a = c.take<uint64_t>(m);
    W->key_b = c.take<uint64_t>(m);
    W->val_a = c.take<int64_t>(m);
    W->val_b = c.take<int64_t>(m);
    W->every = c.take<int32_t>(m + 1);
    W->every_at = c.take<int32_t>(m + 1);
    W->kept = c.take<int32_t>(m + 1);
    W->kept_at = c.take<int32_t>(m + 1);
    if (cv_sort_pairs_temp_bytes<uint64_t, int64_t>(m, &a) || cv_scan_temp_bytes<int32_t>(m + 1, &b)) return 1;
    W->tmp_bytes = a > b ? a : b;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool table_args_ok(const char *who, int64_t n, int64_t nruns, int32_t nctg)
{
    if (n < 0 || n > CV_TRAINSET_MAX_ROWS || nruns < 0 || nruns > n || nctg < 0 || nctg > CV_TRAINSET_MAX_CONTIGS || (n > 0 && nctg < 1)) {
        cv_set_error("%s: %lld rows / %lld runs / %d contigs out of range (0 .. %lld rows, runs <= rows, 0 .. %d contigs)", who, (long long)n,
                     (long long)nruns, (int)nctg, (long long)CV_TRAINSET_MAX_ROWS, CV_TRAINSET_MAX_CONTIGS);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int cv_truth_lines_workspace(int64_t len, int64_t max_lines, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_truth_lines_workspace: null argument"); return 1; }
    if (!lines_args_ok("cv_truth_lines_workspace", len, CV_TRUTH_FORMAT_VAR, max_lines)) return 1;
    cv_carver c;
    lines_ws W;
    if (lines_plan(c, len, max_lines, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_truth_lines_dev(const char *text_dev, int64_t len, int format, const char *ctg, int64_t ctg_len, int has_bounds,
                                  int64_t lower, int64_t upper, int64_t max_lines, int64_t *pos_dev, int64_t *end_dev, float *label_dev,
                                  int32_t *run_dev, int64_t *tok_dev, int64_t *info_dev, void *workspace_dev, int64_t workspace_bytes,
                                  void *stream)
{
    if (!lines_args_ok("cv_truth_lines_dev", len, format, max_lines)) return 1;
    cvt::Filter filter;
    if (!filter_of("cv_truth_lines_dev", format, ctg, ctg_len, has_bounds, lower, upper, &filter)) return 1;
    if (!info_dev || !workspace_dev || (len > 0 && !text_dev) ||
        (max_lines > 0 && (!pos_dev || !run_dev || !tok_dev || (format == CV_TRUTH_FORMAT_BED ? !end_dev : !label_dev)))) {
        cv_set_error("cv_truth_lines_dev: null argument");
        return 1;
    }
    if (((uintptr_t)pos_dev & 7) || ((uintptr_t)end_dev & 7) || ((uintptr_t)label_dev & 3) || ((uintptr_t)run_dev & 3) ||
        ((uintptr_t)tok_dev & 7) || ((uintptr_t)info_dev & 7)) {
        cv_set_error("cv_truth_lines_dev: pos / end / tok / info must be 8-byte, label / run 4-byte aligned");
        return 1;
    }
    cv_carver c(workspace_dev);
    lines_ws W;
    if (lines_plan(c, len, max_lines, &W)) return 1;
    if (!cv_workspace_ok("cv_truth_lines_dev", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t *line_end = nullptr;
    CV_HIP(hipMemsetAsync(info_dev, 0, 8 * sizeof(int64_t), st));
    if (cv_text_line_index(text_dev, len, max_lines, W.index, W.index_info, &line_end, st)) return 1;
    const uint8_t *text = (const uint8_t *)text_dev;
    const int grid = cv_grid_for(max_lines + 1);
    hipLaunchKernelGGL(tl_verdicts, dim3(grid), dim3(THREADS), 0, st, text, line_end, (const int64_t *)W.index_info, max_lines, format,
                       filter, W.status, W.span, W.isrow, info_dev);
    cv_text_run_flags(text, W.span, W.isrow, max_lines, W.flag, st);
    size_t tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)W.isrow, W.rowidx, (int)(max_lines + 1), st));
    tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)W.flag, W.runidx, (int)(max_lines + 1), st));
    hipLaunchKernelGGL(tl_rows, dim3(grid), dim3(THREADS), 0, st, text, line_end, (const int64_t *)W.index_info, max_lines, format,
                       filter, (const int32_t *)W.isrow, (const int32_t *)W.rowidx, (const int32_t *)W.flag, (const int32_t *)W.runidx,
                       (const int64_t *)W.span, pos_dev, end_dev, label_dev, run_dev, tok_dev, info_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_truth_lines_host_form(const char *text, int64_t len, int format, const char *ctg, int64_t ctg_len, int has_bounds,
                                        int64_t lower, int64_t upper, int64_t max_lines, int64_t *pos, int64_t *end, float *label,
                                        int32_t *run, int64_t *tok, int64_t *info)
{
    if (!lines_args_ok("cv_truth_lines_host_form", len, format, max_lines)) return 1;
    cvt::Filter filter;
    if (!filter_of("cv_truth_lines_host_form", format, ctg, ctg_len, has_bounds, lower, upper, &filter)) return 1;
    if (!info || (len > 0 && !text) || (max_lines > 0 && (!pos || !run || !tok || (format == CV_TRUTH_FORMAT_BED ? !end : !label)))) {
        cv_set_error("cv_truth_lines_host_form: null argument");
        return 1;
    }
    if (((uintptr_t)pos & 7) || ((uintptr_t)end & 7) || ((uintptr_t)label & 3) || ((uintptr_t)run & 3) || ((uintptr_t)tok & 7) ||
        ((uintptr_t)info & 7)) {
        cv_set_error("cv_truth_lines_host_form: pos / end / tok / info must be 8-byte, label / run 4-byte aligned");
        return 1;
    }
    cvt::host_form((const uint8_t *)text, len, format, &filter, max_lines, pos, end, label, run, tok, info);
    return 0;
}

extern "C" int cv_bed_table_workspace(int64_t n, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_bed_table_workspace: null argument"); return 1; }
    if (!table_args_ok("cv_bed_table_workspace", n, 0, 1)) return 1;
    cv_carver c;
    bed_ws W;
    if (bed_plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_bed_table_dev(int64_t n, const int64_t *begin_dev, const int64_t *end_dev, const int32_t *run_dev,
                                const int32_t *run_ctg_dev, int64_t nruns, int32_t nctg, int64_t *bed_off_dev, int64_t *bed_begin_dev,
                                int64_t *bed_emax_dev, void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    if (!table_args_ok("cv_bed_table_dev", n, nruns, nctg)) return 1;
    if (!bed_off_dev || !workspace_dev || (n > 0 && (!begin_dev || !end_dev || !run_dev || !run_ctg_dev || !bed_begin_dev || !bed_emax_dev))) {
        cv_set_error("cv_bed_table_dev: null argument");
        return 1;
    }
    if (((uintptr_t)begin_dev & 7) || ((uintptr_t)end_dev & 7) || ((uintptr_t)run_dev & 3) || ((uintptr_t)run_ctg_dev & 3) ||
        ((uintptr_t)bed_off_dev & 7) || ((uintptr_t)bed_begin_dev & 7) || ((uintptr_t)bed_emax_dev & 7)) {
        cv_set_error("cv_bed_table_dev: the int64 arrays must be 8-byte, run / run_ctg 4-byte aligned");
        return 1;
    }
    cv_carver c(workspace_dev);
    bed_ws W;
    if (bed_plan(c, n, &W)) return 1;
    if (!cv_workspace_ok("cv_bed_table_dev", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    uint64_t *key_a = W.key_a, *key_b = W.key_b;
    int64_t *val_a = W.val_a, *val_b = W.val_b;
    const int grid = cv_grid_for(n > nctg ? n : nctg + 1);
    if (n > 0) {
        hipLaunchKernelGGL(bt_end_keys, dim3(grid), dim3(THREADS), 0, st, n, end_dev, key_a, val_a);
        size_t tb = W.tmp_bytes;
        CV_HIP(hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, (const uint64_t *)key_a, key_b, (const int64_t *)val_a, val_b, (int)n, 0,
                                                  END_BITS, st));
        hipLaunchKernelGGL(bt_begin_keys, dim3(grid), dim3(THREADS), 0, st, n, (const int64_t *)val_b, begin_dev, run_dev, run_ctg_dev,
                           nruns, key_a);
        tb = W.tmp_bytes;
        CV_HIP(hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, (const uint64_t *)key_a, key_b, (const int64_t *)val_b, val_a, (int)n, 0,
                                                  POS_BITS + 16, st));
        // key_b: (contig, begin) ascending, val_a: the interval at each slot; key_a <- contig << 41 | end + 1, then its running maximum
        hipLaunchKernelGGL(bt_gather, dim3(grid), dim3(THREADS), 0, st, n, (const uint64_t *)key_b, (const int64_t *)val_a, end_dev,
                           bed_begin_dev, key_a);
        tb = W.tmp_bytes;
        CV_HIP(hipcub::DeviceScan::InclusiveScan(W.tmp, tb, (const uint64_t *)key_a, (uint64_t *)val_b, hipcub::Max(), (int)n, st));
    }
    hipLaunchKernelGGL(bt_finish, dim3(grid), dim3(THREADS), 0, st, n, (const uint64_t *)key_b, (const uint64_t *)val_b, nctg,
                       bed_emax_dev, bed_off_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_truth_tables_workspace(int64_t n, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_truth_tables_workspace: null argument"); return 1; }
    if (!table_args_ok("cv_truth_tables_workspace", n, 0, 1)) return 1;
    cv_carver c;
    tables_ws W;
    if (tables_plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_truth_tables_dev(int64_t n, const int64_t *pos_dev, const float *label_dev, const int32_t *run_dev,
                                   const int32_t *run_ctg_dev, int64_t nruns, int32_t nctg, int has_bed, const int64_t *bed_off_dev,
                                   const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, int64_t *truth_off_dev,
                                   int64_t *truth_pos_dev, float *labels_dev, int64_t *every_off_dev, int64_t *every_pos_dev,
                                   int64_t *counts_dev, void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    if (!table_args_ok("cv_truth_tables_dev", n, nruns, nctg)) return 1;
    if (!truth_off_dev || !every_off_dev || !counts_dev || !workspace_dev ||
        (n > 0 && (!pos_dev || !label_dev || !run_dev || !run_ctg_dev || !truth_pos_dev || !labels_dev || !every_pos_dev)) ||
        (has_bed && nctg > 0 && !bed_off_dev)) {
        cv_set_error("cv_truth_tables_dev: null argument");
        return 1;
    }
    if (((uintptr_t)pos_dev & 7) || ((uintptr_t)label_dev & 15) || ((uintptr_t)run_dev & 3) || ((uintptr_t)run_ctg_dev & 3) ||
        ((uintptr_t)bed_off_dev & 7) || ((uintptr_t)bed_begin_dev & 7) || ((uintptr_t)bed_emax_dev & 7) || ((uintptr_t)truth_off_dev & 7) ||
        ((uintptr_t)truth_pos_dev & 7) || ((uintptr_t)labels_dev & 15) || ((uintptr_t)every_off_dev & 7) || ((uintptr_t)every_pos_dev & 7) ||
        ((uintptr_t)counts_dev & 7)) {
        cv_set_error("cv_truth_tables_dev: the int64 arrays must be 8-byte, the labels 16-byte, run / run_ctg 4-byte aligned");
        return 1;
    }
    cv_carver c(workspace_dev);
    tables_ws W;
    if (tables_plan(c, n, &W)) return 1;
    if (!cv_workspace_ok("cv_truth_tables_dev", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    uint64_t *key_a = W.key_a, *key_b = W.key_b;
    int64_t *val_a = W.val_a, *val_b = W.val_b;
    int32_t *every = W.every, *every_at = W.every_at, *kept = W.kept, *kept_at = W.kept_at;
    const int grid = cv_grid_for(n > nctg ? n + 1 : nctg + 1);
    if (n > 0) {
        hipLaunchKernelGGL(tt_keys, dim3(grid), dim3(THREADS), 0, st, n, pos_dev, run_dev, run_ctg_dev, nruns, key_a, val_a);
        size_t tb = W.tmp_bytes;
        CV_HIP(hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, (const uint64_t *)key_a, key_b, (const int64_t *)val_a, val_b, (int)n, 0,
                                                  POS_BITS + 16, st));
    }
    hipLaunchKernelGGL(tt_tails, dim3(grid), dim3(THREADS), 0, st, n, (const uint64_t *)key_b, nctg, has_bed, bed_off_dev, bed_begin_dev,
                       bed_emax_dev, every, kept);
    size_t tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)every, every_at, (int)(n + 1), st));
    tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)kept, kept_at, (int)(n + 1), st));
    hipLaunchKernelGGL(tt_emit, dim3(grid), dim3(THREADS), 0, st, n, (const uint64_t *)key_b, (const int64_t *)val_b,
                       (const int32_t *)every, (const int32_t *)every_at, (const int32_t *)kept, (const int32_t *)kept_at,
                       (const float4 *)label_dev, nctg, truth_off_dev, truth_pos_dev, (float4 *)labels_dev, every_off_dev, every_pos_dev,
                       counts_dev);
    CV_HIP(hipGetLastError());
    return 0;
}
