// cv_beditems_dev.hip -- the dataPrepScripts helpers on the device: the lines of a file whose first two columns are contig
// and position kept or dropped by a BED (ChooseItemInBed, CountNumInBed), and the positions of a range tested against a
// BED and drawn (RandomSampling).  bed_items.py holds the host loops that define both; cv_truth_core.hpp says per line
// whether the device vouches for it (ROW) or not (HOST; format ITEM has no SKIP); cv_beditems_core.hpp holds the stabbing
// test, the draw and a lane's share of the line copy, one text for host and device.
//
//   per slab (cv_item_lines_dev):
//   newline index       cv_text_line_index of cv_textparse.hip
//   il_verdicts         one thread per line: the core's status, the position and the contig token's span (the core runs ONCE
//                       per line: an item row has two fields and both fit the workspace)
//   run-start flags     cv_text_run_flags of cv_textparse.hip: "this ROW's contig token differs byte for byte from the line
//                       before" (or that line is no ROW)
//   hipcub ExclusiveSum over the ROW flags and over the run-start flags -> row index, run index
//   il_rows             the ROW lines' position, run, start offset and length at their row index, the run-start tokens
//
//   per slab, once the host has named the runs' BED contig ids (cv_items_keep_dev):
//   ik_flags            the stabbing test per row -> the kept line's length or 0; the two counters as integer sums
//   hipcub ExclusiveSum over those lengths -> where each kept line goes
//   ik_copy             ONE WAVE PER KEPT LINE (cvb::copy_lane): lines are about 2.3 KB at arbitrary source and destination
//                       alignment, so consecutive lanes move consecutive 16-byte granules (1 KiB per wave instruction) where
//                       source and destination agree modulo 16 behind a byte head, consecutive aligned 4-byte stores fed by
//                       byte loads where they do not, and single bytes for lines under 64 bytes.
//
//   per slab, for a caller that has the verdicts already (cv_items_copy_dev; PairWithNonVariants' device route):
//   the caller's kept lengths (0: not kept) copied in front of a zero, hipcub ExclusiveSum, ik_copy -- no kernel of its own
//
//   per tile of positions (cv_sample_positions_dev):
//   sp_flags            stabbing test and keyed draw per position; hipcub ExclusiveSum; sp_emit writes the kept positions
//                       ascending, as far as `cap` reaches, and both counts
//
// Integer and byte kernels; every output slot has exactly one writer and the counters are integer sums, so no result
// depends on the order of the launches' blocks.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_internal.hpp"
#include "cv_dev_scan.hpp"
#include "cv_beditems_core.hpp"

namespace {

constexpr int THREADS = 256;

// ---- the line pass ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void il_verdicts(const uint8_t *text, const int64_t *line_end, const int64_t *index_info,
                                                       int64_t max_lines, int64_t *span, int64_t *line_pos, int32_t *isrow, int64_t *info)
{
    const int64_t lines = index_info[1];
    CV_GRID_STRIDE(i, max_lines + 1) {
        int row = 0;
        if (i < lines) {
            const int64_t start = i ? line_end[i - 1] + 1 : 0;
            cvt::Line L;
            cvt::verdict(text + start, line_end[i] - start, cvt::FMT_ITEM, nullptr, false, &L);
            span[2 * i] = start + L.ctg_off;
            span[2 * i + 1] = L.ctg_len;
            line_pos[i] = L.pos;
            row = L.status == cvt::ROW;
            if (!row) atomicAdd((unsigned long long *)&info[4], 1ull);
        }
        isrow[i] = row;
    }
}

__global__ __launch_bounds__(THREADS) void il_rows(const int64_t *line_end, const int64_t *index_info, int64_t max_lines,
                                                   const int32_t *isrow, const int32_t *rowidx, const int32_t *flag, const int32_t *runidx,
                                                   const int64_t *span, const int64_t *line_pos, int64_t *pos, int32_t *run, int64_t *off,
                                                   int64_t *llen, int64_t *tok, int64_t *info)
{
    const int64_t lines = index_info[1];
    CV_GRID_STRIDE(i, lines) {
        if (!isrow[i]) continue;
        const int64_t start = i ? line_end[i - 1] + 1 : 0;
        const int64_t r = rowidx[i];
        pos[r] = line_pos[i];
        run[r] = runidx[i] + flag[i] - 1;
        off[r] = start;
        llen[r] = line_end[i] + 1 - start;
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
    int64_t *index_info, *span, *line_pos;
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
    W->span = c.take<int64_t>(2 * n);
    W->line_pos = c.take<int64_t>(n);
    W->isrow = c.take<int32_t>(n);
    W->rowidx = c.take<int32_t>(n);
    W->flag = c.take<int32_t>(n);
    W->runidx = c.take<int32_t>(n);
    if (cv_scan_temp_bytes<int32_t>(n, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool lines_args_ok(const char *who, int64_t len, int64_t max_lines)
{
    if (len < 0 || len > CV_TEXT_SLAB_MAX || max_lines < 0 || max_lines > CV_TRUTH_MAX_LINES) {
        cv_set_error("%s: len %lld / max_lines %lld out of range (0 .. %lld bytes, 0 .. %lld lines)", who, (long long)len,
                     (long long)max_lines, (long long)CV_TEXT_SLAB_MAX, (long long)CV_TRUTH_MAX_LINES);
        return false;
    }
    return true;
}

// ---- filter, compact, gather --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void ik_flags(int64_t n, const int64_t *pos, const int32_t *run, const int64_t *llen,
                                                    const int32_t *run_ctg, int64_t nruns, int32_t nctg, const int64_t *bed_off,
                                                    const int64_t *bed_begin, const int64_t *bed_emax, int want_text, int64_t *kept_len,
                                                    int64_t *counts)
{
    __shared__ unsigned long long block_kept;
    if (threadIdx.x == 0) block_kept = 0;
    __syncthreads();
    unsigned long long mine = 0;
    CV_GRID_STRIDE(i, n + 1) {
        const bool k = i < n && cvb::keep_row(pos[i], run[i], run_ctg, nruns, nctg, bed_off, bed_begin, bed_emax);
        mine += k;
        if (want_text) kept_len[i] = k && llen[i] > 0 ? llen[i] : 0;
    }
    if (mine) atomicAdd(&block_kept, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (block_kept) atomicAdd((unsigned long long *)&counts[1], block_kept);
        if (blockIdx.x == 0) counts[0] = n;
    }
}

// one wave per row; the waves of the rows that are not kept leave at once
__global__ __launch_bounds__(THREADS) void ik_copy(const uint8_t *text, int64_t len, int64_t n, const int64_t *off, const int64_t *kept_len,
                                                   const int64_t *dst_at, uint8_t *out_text, int64_t out_cap, int64_t *counts)
{
    const int lane = threadIdx.x & (cvb::WAVE - 1);
    const int64_t waves = (int64_t)gridDim.x * (THREADS / cvb::WAVE);
    for (int64_t i = (int64_t)blockIdx.x * (THREADS / cvb::WAVE) + threadIdx.x / cvb::WAVE; i < n; i += waves) {
        const int64_t m = kept_len[i];
        if (m <= 0) continue;
        const int64_t s = off[i], d = dst_at[i];
        if (!cvb::copy_fits(s, m, len, d, out_cap)) continue;         // (the caller's error: nothing outside either buffer is touched)
        cvb::copy_lane(out_text + d, text + s, m, lane);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[2] = dst_at[n];
}

struct keep_ws {
    int64_t *kept_len, *dst_at;
    void *tmp;
    size_t tmp_bytes;
};

int keep_plan(cv_carver &c, int64_t n, keep_ws *W)
{
    const size_t m = (size_t)n + 1;
    W->kept_len = c.take<int64_t>(m);
    W->dst_at = c.take<int64_t>(m);
    if (cv_scan_temp_bytes<int64_t>(m, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool keep_args_ok(const char *who, int64_t len, int64_t n, int64_t nruns, int32_t nctg, int64_t out_cap)
{
    // (the rows may be a part of a slab's rows, so there may be more runs than rows)
    if (len < 0 || len > CV_TEXT_SLAB_MAX || n < 0 || n > CV_TRUTH_MAX_LINES || nruns < 0 || nruns > CV_TRUTH_MAX_LINES || nctg < 0 ||
        nctg > CV_TRAINSET_MAX_CONTIGS || out_cap < 0) {
        cv_set_error("%s: %lld bytes / %lld rows / %lld runs / %d contigs / room for %lld bytes out of range (0 .. %lld bytes, 0 .. %lld "
                     "rows and runs, 0 .. %d contigs)", who, (long long)len, (long long)n, (long long)nruns, (int)nctg,
                     (long long)out_cap, (long long)CV_TEXT_SLAB_MAX, (long long)CV_TRUTH_MAX_LINES, CV_TRAINSET_MAX_CONTIGS);
        return false;
    }
    return true;
}

// ---- the sampler --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void sp_flags(uint64_t seed, uint32_t h, int64_t first, int64_t count, double prob, int64_t nbed,
                                                    const int64_t *bed_begin, const int64_t *bed_emax, int32_t *flag)
{
    CV_GRID_STRIDE(i, count + 1) flag[i] = i < count && cvb::sample_keep(seed, h, first + i, prob, nbed, bed_begin, bed_emax);
}

__global__ __launch_bounds__(THREADS) void sp_emit(int64_t first, int64_t count, const int32_t *flag, const int32_t *at, int64_t *out_pos,
                                                   int64_t cap, int64_t *counts)
{
    CV_GRID_STRIDE(i, count)
        if (flag[i] && at[i] < cap) out_pos[at[i]] = first + i;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t would = at[count];
        counts[0] = would < cap ? would : cap;
        counts[1] = would;
    }
}

struct sample_ws {
    int32_t *flag, *at;
    void *tmp;
    size_t tmp_bytes;
};

int sample_plan(cv_carver &c, int64_t count, sample_ws *W)
{
    const size_t m = (size_t)count + 1;
    W->flag = c.take<int32_t>(m);
    W->at = c.take<int32_t>(m);
    if (cv_scan_temp_bytes<int32_t>(m, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool sample_args_ok(const char *who, int64_t first, int64_t count, double prob, int64_t nbed, int64_t cap)
{
    if (count < 0 || count > CV_SAMPLE_MAX_TILE || first < 0 || first > INT64_MAX - count || nbed < 0 || nbed > CV_TRAINSET_MAX_ROWS ||
        cap < 0 || !(prob == prob)) {
        cv_set_error("%s: first %lld / count %lld / %lld intervals / cap %lld out of range (0 .. %lld positions per tile), or prob is "
                     "not a number", who, (long long)first, (long long)count, (long long)nbed, (long long)cap,
                     (long long)CV_SAMPLE_MAX_TILE);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int cv_item_lines_workspace(int64_t len, int64_t max_lines, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_item_lines_workspace: null argument"); return 1; }
    if (!lines_args_ok("cv_item_lines_workspace", len, max_lines)) return 1;
    cv_carver c;
    lines_ws W;
    if (lines_plan(c, len, max_lines, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_item_lines_dev(const char *text_dev, int64_t len, int64_t max_lines, int64_t *pos_dev, int32_t *run_dev, int64_t *off_dev,
                                 int64_t *len_dev, int64_t *tok_dev, int64_t *info_dev, void *workspace_dev, int64_t workspace_bytes,
                                 void *stream)
{
    if (!lines_args_ok("cv_item_lines_dev", len, max_lines)) return 1;
    if (!info_dev || !workspace_dev || (len > 0 && !text_dev) || (max_lines > 0 && (!pos_dev || !run_dev || !off_dev || !len_dev || !tok_dev))) {
        cv_set_error("cv_item_lines_dev: null argument");
        return 1;
    }
    if (((uintptr_t)pos_dev & 7) || ((uintptr_t)run_dev & 3) || ((uintptr_t)off_dev & 7) || ((uintptr_t)len_dev & 7) ||
        ((uintptr_t)tok_dev & 7) || ((uintptr_t)info_dev & 7)) {
        cv_set_error("cv_item_lines_dev: pos / off / len / tok / info must be 8-byte, run 4-byte aligned");
        return 1;
    }
    cv_carver c(workspace_dev);
    lines_ws W;
    if (lines_plan(c, len, max_lines, &W)) return 1;
    if (!cv_workspace_ok("cv_item_lines_dev", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t *line_end = nullptr;
    CV_HIP(hipMemsetAsync(info_dev, 0, 8 * sizeof(int64_t), st));
    if (cv_text_line_index(text_dev, len, max_lines, W.index, W.index_info, &line_end, st)) return 1;
    const uint8_t *text = (const uint8_t *)text_dev;
    const int grid = cv_grid_for(max_lines + 1);
    hipLaunchKernelGGL(il_verdicts, dim3(grid), dim3(THREADS), 0, st, text, line_end, (const int64_t *)W.index_info, max_lines, W.span,
                       W.line_pos, W.isrow, info_dev);
    cv_text_run_flags(text, W.span, W.isrow, max_lines, W.flag, st);
    size_t tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)W.isrow, W.rowidx, (int)(max_lines + 1), st));
    tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)W.flag, W.runidx, (int)(max_lines + 1), st));
    hipLaunchKernelGGL(il_rows, dim3(grid), dim3(THREADS), 0, st, line_end, (const int64_t *)W.index_info, max_lines,
                       (const int32_t *)W.isrow, (const int32_t *)W.rowidx, (const int32_t *)W.flag, (const int32_t *)W.runidx,
                       (const int64_t *)W.span, (const int64_t *)W.line_pos, pos_dev, run_dev, off_dev, len_dev, tok_dev, info_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_item_lines_host_form(const char *text, int64_t len, int64_t max_lines, int64_t *pos, int32_t *run, int64_t *off,
                                       int64_t *llen, int64_t *tok, int64_t *info)
{
    if (!lines_args_ok("cv_item_lines_host_form", len, max_lines)) return 1;
    if (!info || (len > 0 && !text) || (max_lines > 0 && (!pos || !run || !off || !llen || !tok))) {
        cv_set_error("cv_item_lines_host_form: null argument");
        return 1;
    }
    if (((uintptr_t)pos & 7) || ((uintptr_t)run & 3) || ((uintptr_t)off & 7) || ((uintptr_t)llen & 7) || ((uintptr_t)tok & 7) ||
        ((uintptr_t)info & 7)) {
        cv_set_error("cv_item_lines_host_form: pos / off / len / tok / info must be 8-byte, run 4-byte aligned");
        return 1;
    }
    cvb::lines_host_form((const uint8_t *)text, len, max_lines, pos, run, off, llen, tok, info);
    return 0;
}

extern "C" int cv_items_keep_workspace(int64_t n, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_items_keep_workspace: null argument"); return 1; }
    if (!keep_args_ok("cv_items_keep_workspace", 0, n, 0, 0, 0)) return 1;
    cv_carver c;
    keep_ws W;
    if (keep_plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

static bool keep_pointers_ok(const char *who, const char *text, int64_t len, int64_t n, const int64_t *pos, const int32_t *run,
                             const int64_t *off, const int64_t *llen, const int32_t *run_ctg, int32_t nctg, const int64_t *bed_off,
                             const int64_t *bed_begin, const int64_t *bed_emax, int want_text, const char *out_text, int64_t out_cap,
                             const int64_t *counts)
{
    if (!counts || (len > 0 && !text) || (n > 0 && (!pos || !run || !off || !llen || !run_ctg)) || (nctg > 0 && !bed_off) ||
        (want_text && out_cap > 0 && !out_text)) {
        cv_set_error("%s: null argument", who);
        return false;
    }
    if (((uintptr_t)pos & 7) || ((uintptr_t)run & 3) || ((uintptr_t)off & 7) || ((uintptr_t)llen & 7) || ((uintptr_t)run_ctg & 3) ||
        ((uintptr_t)bed_off & 7) || ((uintptr_t)bed_begin & 7) || ((uintptr_t)bed_emax & 7) || ((uintptr_t)counts & 7)) {
        cv_set_error("%s: the int64 arrays must be 8-byte, run / run_ctg 4-byte aligned", who);
        return false;
    }
    return true;
}

extern "C" int cv_items_keep_dev(const char *text_dev, int64_t len, int64_t n, const int64_t *pos_dev, const int32_t *run_dev,
                                 const int64_t *off_dev, const int64_t *len_dev, const int32_t *run_ctg_dev, int64_t nruns, int32_t nctg,
                                 const int64_t *bed_off_dev, const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, int want_text,
                                 char *out_text_dev, int64_t out_cap, int64_t *counts_dev, void *workspace_dev, int64_t workspace_bytes,
                                 void *stream)
{
    if (!keep_args_ok("cv_items_keep_dev", len, n, nruns, nctg, out_cap)) return 1;
    if (!keep_pointers_ok("cv_items_keep_dev", text_dev, len, n, pos_dev, run_dev, off_dev, len_dev, run_ctg_dev, nctg, bed_off_dev,
                          bed_begin_dev, bed_emax_dev, want_text, out_text_dev, out_cap, counts_dev))
        return 1;
    cv_carver c(workspace_dev);
    keep_ws W;
    if (keep_plan(c, n, &W)) return 1;
    if (!cv_workspace_ok("cv_items_keep_dev", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    int64_t *kept_len = W.kept_len, *dst_at = W.dst_at;
    CV_HIP(hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(ik_flags, dim3(cv_grid_for(n + 1)), dim3(THREADS), 0, st, n, pos_dev, run_dev, len_dev, run_ctg_dev, nruns, nctg,
                       bed_off_dev, bed_begin_dev, bed_emax_dev, want_text, kept_len, counts_dev);
    if (want_text) {
        size_t tb = W.tmp_bytes;
        CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int64_t *)kept_len, dst_at, (int)(n + 1), st));
        const int64_t blocks = (n + THREADS / cvb::WAVE - 1) / (THREADS / cvb::WAVE);
        hipLaunchKernelGGL(ik_copy, dim3((unsigned)(blocks < 1 ? 1 : blocks < 65536 ? blocks : 65536)), dim3(THREADS), 0, st,
                           (const uint8_t *)text_dev, len, n, off_dev, (const int64_t *)kept_len, (const int64_t *)dst_at,
                           (uint8_t *)out_text_dev, out_cap, counts_dev);
    }
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_items_keep_host_form(const char *text, int64_t len, int64_t n, const int64_t *pos, const int32_t *run, const int64_t *off,
                                       const int64_t *llen, const int32_t *run_ctg, int64_t nruns, int32_t nctg, const int64_t *bed_off,
                                       const int64_t *bed_begin, const int64_t *bed_emax, int want_text, char *out_text, int64_t out_cap,
                                       int64_t *counts)
{
    if (!keep_args_ok("cv_items_keep_host_form", len, n, nruns, nctg, out_cap)) return 1;
    if (!keep_pointers_ok("cv_items_keep_host_form", text, len, n, pos, run, off, llen, run_ctg, nctg, bed_off, bed_begin, bed_emax, want_text,
                          out_text, out_cap, counts))
        return 1;
    cvb::keep_host_form((const uint8_t *)text, len, n, pos, run, off, llen, run_ctg, nruns, nctg, bed_off, bed_begin, bed_emax, want_text,
                        (uint8_t *)out_text, out_cap, counts);
    return 0;
}

// ---- the gather by given lengths: cv_items_keep_dev without ik_flags --------------------------------------------------------
static bool copy_pointers_ok(const char *who, const char *text, int64_t len, int64_t n, const int64_t *off, const int64_t *kept_len,
                             const char *out_text, int64_t out_cap, const int64_t *counts)
{
    if (!counts || (len > 0 && !text) || (n > 0 && (!off || !kept_len)) || (out_cap > 0 && !out_text)) {
        cv_set_error("%s: null argument", who);
        return false;
    }
    if (((uintptr_t)off & 7) || ((uintptr_t)kept_len & 7) || ((uintptr_t)counts & 7)) {
        cv_set_error("%s: the int64 arrays must be 8-byte aligned", who);
        return false;
    }
    return true;
}

extern "C" int cv_items_copy_workspace(int64_t n, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_items_copy_workspace: null argument"); return 1; }
    if (!keep_args_ok("cv_items_copy_workspace", 0, n, 0, 0, 0)) return 1;
    cv_carver c;
    keep_ws W;
    if (keep_plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_items_copy_dev(const char *text_dev, int64_t len, int64_t n, const int64_t *off_dev, const int64_t *kept_len_dev,
                                 char *out_text_dev, int64_t out_cap, int64_t *counts_dev, void *workspace_dev, int64_t workspace_bytes,
                                 void *stream)
{
    if (!keep_args_ok("cv_items_copy_dev", len, n, 0, 0, out_cap)) return 1;
    if (!copy_pointers_ok("cv_items_copy_dev", text_dev, len, n, off_dev, kept_len_dev, out_text_dev, out_cap, counts_dev)) return 1;
    cv_carver c(workspace_dev);
    keep_ws W;
    if (keep_plan(c, n, &W)) return 1;
    if (!cv_workspace_ok("cv_items_copy_dev", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    int64_t *kept_len = W.kept_len, *dst_at = W.dst_at;
    CV_HIP(hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), st));
    // the scan reads n + 1 values (its last output is the sum): the caller's n lengths and a zero behind them
    if (n > 0) { CV_HIP(hipMemcpyAsync(kept_len, kept_len_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st)); }
    CV_HIP(hipMemsetAsync(kept_len + n, 0, sizeof(int64_t), st));
    size_t tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int64_t *)kept_len, dst_at, (int)(n + 1), st));
    const int64_t blocks = (n + THREADS / cvb::WAVE - 1) / (THREADS / cvb::WAVE);
    hipLaunchKernelGGL(ik_copy, dim3((unsigned)(blocks < 1 ? 1 : blocks < 65536 ? blocks : 65536)), dim3(THREADS), 0, st,
                       (const uint8_t *)text_dev, len, n, off_dev, (const int64_t *)kept_len, (const int64_t *)dst_at,
                       (uint8_t *)out_text_dev, out_cap, counts_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_items_copy_host_form(const char *text, int64_t len, int64_t n, const int64_t *off, const int64_t *kept_len,
                                       char *out_text, int64_t out_cap, int64_t *counts)
{
    if (!keep_args_ok("cv_items_copy_host_form", len, n, 0, 0, out_cap)) return 1;
    if (!copy_pointers_ok("cv_items_copy_host_form", text, len, n, off, kept_len, out_text, out_cap, counts)) return 1;
    cvb::copy_host_form((const uint8_t *)text, len, n, off, kept_len, (uint8_t *)out_text, out_cap, counts);
    return 0;
}

extern "C" int cv_sample_positions_workspace(int64_t count, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_sample_positions_workspace: null argument"); return 1; }
    if (!sample_args_ok("cv_sample_positions_workspace", 0, count, 0.0, 0, 0)) return 1;
    cv_carver c;
    sample_ws W;
    if (sample_plan(c, count, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_sample_positions_dev(uint64_t seed, uint32_t h, int64_t first, int64_t count, double prob, int64_t nbed,
                                       const int64_t *bed_begin_dev, const int64_t *bed_emax_dev, int64_t *out_pos_dev, int64_t cap,
                                       int64_t *count_dev, void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    if (!sample_args_ok("cv_sample_positions_dev", first, count, prob, nbed, cap)) return 1;
    if (!count_dev || !workspace_dev || (nbed > 0 && (!bed_begin_dev || !bed_emax_dev)) || (cap > 0 && !out_pos_dev)) {
        cv_set_error("cv_sample_positions_dev: null argument");
        return 1;
    }
    if (((uintptr_t)bed_begin_dev & 7) || ((uintptr_t)bed_emax_dev & 7) || ((uintptr_t)out_pos_dev & 7) || ((uintptr_t)count_dev & 7)) {
        cv_set_error("cv_sample_positions_dev: the int64 arrays must be 8-byte aligned");
        return 1;
    }
    cv_carver c(workspace_dev);
    sample_ws W;
    if (sample_plan(c, count, &W)) return 1;
    if (!cv_workspace_ok("cv_sample_positions_dev", workspace_dev, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    int32_t *flag = W.flag, *at = W.at;
    const int grid = cv_grid_for(count + 1);
    hipLaunchKernelGGL(sp_flags, dim3(grid), dim3(THREADS), 0, st, seed, h, first, count, prob, nbed, bed_begin_dev, bed_emax_dev, flag);
    size_t tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int32_t *)flag, at, (int)(count + 1), st));
    hipLaunchKernelGGL(sp_emit, dim3(grid), dim3(THREADS), 0, st, first, count, (const int32_t *)flag, (const int32_t *)at, out_pos_dev, cap,
                       count_dev);
    CV_HIP(hipGetLastError());
    return 0;
}
