// cv_candrows_dev.hip -- the rows of ExtractVariantCandidates.py written in HBM from the entries the candidate pass
// selected there: candidate_rows' bytes, row for row, for the rows cv_candrows_core.hpp vouches for (that header holds
// the length, the stable 7-element sort and the digits once, for these kernels and for cv_candidate_rows_host_form; its
// host form is held to snprintf + std::stable_sort by tests/native/candrows_core_driver.cpp).
//
//   candorder_flag / hipcub ExclusiveSum / candorder_place   candidate_order as a stable partition: the entries with
//                  late == 0 and pos0 < last_pos keep their order in front, all others keep theirs behind
//   candrows_len   one lane per row (a row is 40-110 bytes: a wave per row would idle 63 lanes): the verdict and the
//                  length, 0 and CV_CANDROWS_HOST for a row left to the host
//   hipcub ExclusiveSum over the rows + 1 lengths (int64) -> off[rows + 1]
//   candrows_write one wave takes 64 consecutive rows, whose text is ONE contiguous range of HBM: every lane assembles
//                  its row in LDS at the offset it has in that range, the range standing at the phase (address mod 16)
//                  it has in HBM; the wave then stores the range in aligned 16-byte granules, bytes only at its two ends.
//                  A row is at most cvc::MAX_ROW = 381 bytes, so 64 rows at any phase take 24 400 bytes of LDS: a
//                  workgroup is one wave, six of them fit the CU's 160 KiB
//
// Nothing behind off[rows] is written; a row that does not fit below text_cap is not written at all.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <string.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_dev_scan.hpp"
#include "cv_candrows_core.hpp"

namespace {

constexpr int LANES = 64;
constexpr int WAVE_TEXT = LANES * cvc::MAX_ROW;           // the longest range of one wave
constexpr int WAVE_LDS = (WAVE_TEXT + 16 + 15) & ~15;     // ... at phase 15, in whole granules
static_assert(WAVE_LDS + cvc::MAX_CTG + 1 <= 64 * 1024, "one workgroup's LDS");
static_assert(6 * (WAVE_LDS + cvc::MAX_CTG + 1) <= 160 * 1024, "six one-wave workgroups share the CU's 160 KiB");
static_assert(CV_CANDROWS_DEVICE == cvc::STATUS_DEVICE && CV_CANDROWS_HOST == cvc::STATUS_HOST, "the header's status values");

struct CtgName { char s[cvc::MAX_CTG + 1]; };

__global__ __launch_bounds__(256) void candorder_flag(const int64_t *__restrict__ pos0, const int32_t *__restrict__ late, int64_t n,
                                                       int64_t last_pos, int64_t *__restrict__ head)
{
    CV_GRID_STRIDE(i, n + 1) head[i] = i < n && late[i] == 0 && pos0[i] < last_pos ? 1 : 0;
}

// head_before[i] = heads in front of entry i, head_before[n] = heads in all
__global__ __launch_bounds__(256) void candorder_place(const int64_t *__restrict__ pos0, const int32_t *__restrict__ late, int64_t n,
                                                        int64_t last_pos, const int64_t *__restrict__ head_before,
                                                        int64_t *__restrict__ order)
{
    CV_GRID_STRIDE(i, n) {
        const int64_t h = head_before[i];
        const bool head = late[i] == 0 && pos0[i] < last_pos;
        order[head ? h : head_before[n] + (i - h)] = i;
    }
}

__global__ __launch_bounds__(256) void candrows_len(int ctg_len, const int64_t *__restrict__ order, int64_t rows, int64_t n,
                                                     const int64_t *__restrict__ pos0, const int32_t *__restrict__ counts7,
                                                     const uint8_t *__restrict__ ref, int64_t ref_first0, int64_t ref_len,
                                                     int64_t *__restrict__ len_out, uint8_t *__restrict__ status)
{
    CV_GRID_STRIDE(r, rows + 1) {
        if (r == rows) { len_out[r] = 0; continue; }       // the scan's last input: off[rows] becomes the total
        int64_t e; uint8_t b;
        const int len = cvc::row_verdict(ctg_len, order, r, n, pos0, counts7, ref, ref_first0, ref_len, &e, &b);
        len_out[r] = len;
        status[r] = len ? CV_CANDROWS_DEVICE : CV_CANDROWS_HOST;
    }
}

__global__ __launch_bounds__(LANES) void candrows_write(CtgName ctg, int ctg_len, const int64_t *__restrict__ order, int64_t rows,
                                                         int64_t n, const int64_t *__restrict__ pos0,
                                                         const int32_t *__restrict__ counts7, const uint8_t *__restrict__ ref,
                                                         int64_t ref_first0, int64_t ref_len, const int64_t *__restrict__ off,
                                                         const uint8_t *__restrict__ status, char *__restrict__ text, int64_t text_cap)
{
    __shared__ __attribute__((aligned(16))) char s_text[WAVE_LDS];
    __shared__ char s_ctg[cvc::MAX_CTG + 1];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * LANES, r = r0 + lane;
    for (int i = lane; i < ctg_len; i += LANES) s_ctg[i] = ctg.s[i];
    const int64_t start = off[r0];                          // (r0 < rows: the grid holds no empty wave)
    const int phase = (int)((uintptr_t)(text + start) & 15);
    int64_t e = 0, rel = 0;
    uint8_t b = 0;
    int len = 0;
    if (r < rows && status[r] == CV_CANDROWS_DEVICE) {
        len = cvc::row_verdict(ctg_len, order, r, n, pos0, counts7, ref, ref_first0, ref_len, &e, &b);
        const int64_t at = off[r];
        rel = at - start;
        // the length the scan summed, inside the wave's range and below the cap -- or the row stays unwritten
        if (len <= 0 || off[r + 1] - at != len || rel < 0 || rel + len > WAVE_TEXT || at < 0 || at + len > text_cap) len = 0;
    }
    __syncthreads();                                        // s_ctg
    if (len) cvc::row_write(s_text + phase + rel, s_ctg, ctg_len, pos0[e], b, counts7 + e * cvc::NSYM);
    // the end of the wave's range: behind the last row written (the rows that fit are a prefix of the wave's)
    int end = len ? (int)rel + len : 0;
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(end, d, 64); end = o > end ? o : end; }
    __syncthreads();                                        // s_text
    if (end == 0) return;
    end += phase;
    char *base = text + start - phase;                      // 16-byte aligned, s_text[i] belongs to base[i]
    for (int s = lane * 16; s < end; s += LANES * 16) {
        if (s >= phase && s + 16 <= end) {
            *reinterpret_cast<uint4 *>(base + s) = *reinterpret_cast<const uint4 *>(s_text + s);
        } else {
            const int lo = s < phase ? phase : s, hi = s + 16 < end ? s + 16 : end;
            for (int i = lo; i < hi; ++i) base[i] = s_text[i];
        }
    }
}

constexpr int64_t MAX_ROWS = (int64_t)1 << 30;

// the workspace of both calls: n + 1 int64 (row lengths / heads in front) | hipcub's
struct scan_ws {
    int64_t *val;
    void *tmp;
    size_t tmp_bytes;
};

int plan(cv_carver &c, int64_t n, scan_ws *W)
{
    W->val = c.take<int64_t>((size_t)(n + 1));
    if (cv_scan_temp_bytes<int64_t>(n + 1, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool rows_ok(const char *who, int64_t rows)
{
    if (rows < 0 || rows > MAX_ROWS) {
        cv_set_error("%s: %lld rows out of range (0 .. %lld)", who, (long long)rows, (long long)MAX_ROWS);
        return false;
    }
    return true;
}

int workspace_of(const char *who, int64_t n, int64_t *bytes)
{
    if (!bytes) { cv_set_error("%s: null argument", who); return 1; }
    if (!rows_ok(who, n)) return 1;
    cv_carver c;
    scan_ws W;
    if (plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

}  // namespace

extern "C" int cv_candidate_order_workspace(int64_t n, int64_t *bytes) { return workspace_of("cv_candidate_order_workspace", n, bytes); }

extern "C" int cv_candidate_order_dev(const int64_t *pos0_dev, const int32_t *late_dev, int64_t n, int64_t last_pos,
                                      int64_t *order_dev, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_candidate_order_dev";
    if (!rows_ok(who, n)) return 1;
    if (!workspace || (n > 0 && (!pos0_dev || !late_dev || !order_dev))) { cv_set_error("%s: null argument", who); return 1; }
    cv_carver c(workspace);
    scan_ws W;
    if (plan(c, n, &W)) return 1;
    if (!cv_workspace_ok(who, workspace, workspace_bytes, c.total())) return 1;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    size_t tb = W.tmp_bytes;
    hipLaunchKernelGGL(candorder_flag, dim3(cv_grid_for(n + 1)), dim3(256), 0, st, pos0_dev, late_dev, n, last_pos, W.val);
    CV_HIP(hipGetLastError());
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int64_t *)W.val, W.val, (int)(n + 1), st));
    hipLaunchKernelGGL(candorder_place, dim3(cv_grid_for(n)), dim3(256), 0, st, pos0_dev, late_dev, n, last_pos,
                       (const int64_t *)W.val, order_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_candidate_rows_workspace(int64_t rows, int64_t *bytes) { return workspace_of("cv_candidate_rows_workspace", rows, bytes); }

extern "C" int cv_candidate_rows_dev(const char *ctg, int64_t ctg_len, const int64_t *order_dev, int64_t rows, int64_t n,
                                     const int64_t *pos0_dev, const int32_t *late_dev, const int32_t *counts7_dev,
                                     const uint8_t *ref_dev, int64_t ref_first0, int64_t ref_len, int64_t *off_dev,
                                     uint8_t *status_dev, char *text_dev, int64_t text_cap, void *workspace,
                                     int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_candidate_rows_dev";
    (void)late_dev;                                     // (a late entry differs in its counts alone)
    if (!rows_ok(who, rows) || !rows_ok(who, n)) return 1;
    if (!ctg || ctg_len < 0 || !off_dev || !workspace || (rows > 0 && !status_dev) || (n > 0 && (!pos0_dev || !counts7_dev)) ||
        (ref_len > 0 && !ref_dev) || ref_len < 0 || text_cap < 0) {
        cv_set_error("%s: null argument, or a negative length", who);
        return 1;
    }
    if (((uintptr_t)pos0_dev & 7) || ((uintptr_t)off_dev & 7) || ((uintptr_t)order_dev & 7) || ((uintptr_t)counts7_dev & 3)) {
        cv_set_error("%s: order / pos0 / off must be 8-byte, counts7 4-byte aligned", who);
        return 1;
    }
    cv_carver c(workspace);
    scan_ws W;
    if (plan(c, rows, &W)) return 1;
    if (!cv_workspace_ok(who, workspace, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (ctg_len > cvc::MAX_CTG) {                   // the whole call is the host's: no lengths, every row CV_CANDROWS_HOST
        CV_HIP(hipMemsetAsync(off_dev, 0, (size_t)(rows + 1) * 8, st));
        if (rows) CV_HIP(hipMemsetAsync(status_dev, CV_CANDROWS_HOST, (size_t)rows, st));
        return 0;
    }
    size_t tb = W.tmp_bytes;
    hipLaunchKernelGGL(candrows_len, dim3(cv_grid_for(rows + 1)), dim3(256), 0, st, (int)ctg_len, order_dev, rows, n, pos0_dev,
                       counts7_dev, ref_dev, ref_first0, ref_len, W.val, status_dev);
    CV_HIP(hipGetLastError());
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int64_t *)W.val, off_dev, (int)(rows + 1), st));
    if (text_dev && rows) {
        CtgName name;
        memset(&name, 0, sizeof(name));
        memcpy(name.s, ctg, (size_t)ctg_len);
        const unsigned blocks = (unsigned)((rows + LANES - 1) / LANES);
        hipLaunchKernelGGL(candrows_write, dim3(blocks), dim3(LANES), 0, st, name, (int)ctg_len, order_dev, rows, n, pos0_dev,
                           counts7_dev, ref_dev, ref_first0, ref_len, (const int64_t *)off_dev, (const uint8_t *)status_dev,
                           text_dev, text_cap);
        CV_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int cv_candidate_rows_host_form(const char *ctg, int64_t ctg_len, const int64_t *order, int64_t rows, int64_t n,
                                           const int64_t *pos0, const int32_t *late, const int32_t *counts7, const uint8_t *ref,
                                           int64_t ref_first0, int64_t ref_len, int64_t *off, uint8_t *status, char *text,
                                           int64_t text_cap)
{
    const char *who = "cv_candidate_rows_host_form";
    (void)late;
    if (!rows_ok(who, rows) || !rows_ok(who, n)) return 1;
    if (!ctg || ctg_len < 0 || !off || (rows > 0 && !status) || (n > 0 && (!pos0 || !counts7)) || (ref_len > 0 && !ref) ||
        ref_len < 0 || text_cap < 0) {
        cv_set_error("%s: null argument, or a negative length", who);
        return 1;
    }
    cvc::rows_host_form(ctg, ctg_len, order, rows, n, pos0, counts7, ref, ref_first0, ref_len, off, status, text, text_cap);
    return 0;
}
