// cv_rowtext_dev.hip -- the text rows of CreateTensor.py (:52) written in HBM from the count tensors the pileup left
// there: cv_format_tensor_row + "\n" per candidate, byte for byte, for the rows whose values the host formatter would
// print through its integer branch (cv_rowtext_core.hpp holds the predicate and the digits; the host form of that header
// is held to snprintf by tests/native/rowtext_core_driver.cpp).
//
//   rowtext_len    one wave per row: value_len() of the 528 values (coalesced float4 loads, the order does not matter for
//                  a sum), a wave reduction, the header's length; a row with a value the device does not vouch for gets
//                  length 0 and status CV_ROWTEXT_HOST
//   hipcub ExclusiveSum over the rows + 1 lengths (int64: a batch can exceed 2^31 bytes) -> off[rows + 1]
//   rowtext_write  one wave per row: the counts staged in LDS, lane l formats the values [9 l, 9 l + 9), one wave scan of
//                  the lanes' byte counts places them; the row is assembled in LDS at the phase (address mod 16) it has in
//                  HBM and leaves in aligned 16-byte stores, bytes only at its two ends.  A row is at most 6 118 bytes
//                  (cvr::MAX_ROW), so 8 KiB of LDS per wave hold it at any phase
//
// Nothing behind off[rows] is written; a row that does not fit below text_cap is not written at all.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <string.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_dev_scan.hpp"
#include "cv_rowtext_core.hpp"

namespace {

constexpr int ROWS_PER_BLOCK = 4;                 // waves of a workgroup, each with its own row
constexpr int THREADS = ROWS_PER_BLOCK * cvr::LANES;
constexpr int ROW_LDS = 8192;                     // text of one row at any 16-byte phase
constexpr int NV4 = cvr::NVALS / 4;               // 132 float4 of a row
static_assert(cvr::MAX_ROW + 16 <= ROW_LDS, "a row at phase 15 must fit its LDS buffer");
static_assert(cvr::PER_LANE * cvr::LANES >= cvr::NVALS, "the lanes cover the row");

struct CtgName { char s[cvr::MAX_CTG + 1]; };

__device__ inline int wave_sum(int v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// lengths: len_out[r] = bytes of row r with its newline, 0 for a row left to the host; len_out[rows] = 0
__global__ __launch_bounds__(THREADS) void rowtext_len(int ctg_len, const int64_t *__restrict__ centres, int64_t rows,
                                                        int64_t ref_first0, int64_t ref_len, const float *__restrict__ counts,
                                                        int64_t *__restrict__ len_out, uint8_t *__restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (r > rows) return;
    if (r == rows) {                              // the scan's last input: off[rows] becomes the total
        if (lane == 0) len_out[rows] = 0;
        return;
    }
    const float4 *row = reinterpret_cast<const float4 *>(counts + r * cvr::NVALS);
    int sum = 0, bad = 0;
    for (int i = lane; i < NV4; i += cvr::LANES) {
        const float4 q = row[i];
        const int a = cvr::value_len(q.x), b = cvr::value_len(q.y), c = cvr::value_len(q.z), d = cvr::value_len(q.w);
        bad |= (a == 0) | (b == 0) | (c == 0) | (d == 0);
        sum += a + b + c + d;
    }
    sum = wave_sum(sum);
    bad = wave_sum(bad);
    if (lane == 0) {
        int64_t s0; int sl;
        const int head = cvr::header_len(ctg_len, centres[r], ref_first0, ref_len, &s0, &sl);
        const bool host = bad != 0 || head == 0;
        len_out[r] = host ? 0 : (int64_t)head + sum + 1;
        status[r] = host ? CV_ROWTEXT_HOST : CV_ROWTEXT_DEVICE;
    }
}

__global__ __launch_bounds__(THREADS) void rowtext_write(CtgName ctg, int ctg_len, const int64_t *__restrict__ centres, int64_t rows,
                                                          const uint8_t *__restrict__ ref, int64_t ref_first0, int64_t ref_len,
                                                          const float *__restrict__ counts, const int64_t *__restrict__ off,
                                                          const uint8_t *__restrict__ status, char *__restrict__ text, int64_t text_cap)
{
    __shared__ __attribute__((aligned(16))) char s_text[ROWS_PER_BLOCK][ROW_LDS];
    __shared__ __attribute__((aligned(16))) float s_cnt[ROWS_PER_BLOCK][cvr::NVALS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * ROWS_PER_BLOCK + w;
    // every wave meets both barriers; a wave without a row to write only skips the work between them
    int64_t at = 0, len = 0;
    bool active = r < rows && status[r] == CV_ROWTEXT_DEVICE;
    if (active) {
        at = off[r];
        len = off[r + 1] - at;
        active = len > 0 && len <= cvr::MAX_ROW && at >= 0 && at + len <= text_cap;
    }
    char *buf = s_text[w];
    float *cnt = s_cnt[w];
    const int phase = active ? (int)((uintptr_t)(text + at) & 15) : 0;
    if (active) {
        const float4 *row = reinterpret_cast<const float4 *>(counts + r * cvr::NVALS);
        for (int i = lane; i < NV4; i += cvr::LANES) reinterpret_cast<float4 *>(cnt)[i] = row[i];
    }
    __syncthreads();
    if (active) {
        const int64_t centre = centres[r];
        int64_t s0 = 0; int sl = 0;
        const int head = cvr::header_len(ctg_len, centre, ref_first0, ref_len, &s0, &sl);
        // header: "<ctg> <centre> <seq>"
        char *p = buf + phase;
        for (int i = lane; i < ctg_len; i += cvr::LANES) p[i] = ctg.s[i];
        const int nd = cvr::digits_i64(centre);
        if (lane == 0) {
            p[ctg_len] = ' ';
            cvr::centre_write(p + ctg_len + 1, centre, nd);
            p[ctg_len + 1 + nd] = ' ';
        }
        if (lane < sl) p[ctg_len + 2 + nd + lane] = (char)ref[s0 + lane];
        // values: lane l holds [9 l, 9 l + 9); an inclusive wave scan of the lanes' byte counts places them
        const int k0 = lane * cvr::PER_LANE;
        int mine = 0;
        for (int j = 0; j < cvr::PER_LANE; ++j)
            if (k0 + j < cvr::NVALS) mine += cvr::value_len(cnt[k0 + j]);
        int incl = mine;
        for (int d = 1; d < cvr::LANES; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        char *q = p + head + (incl - mine);
        for (int j = 0; j < cvr::PER_LANE; ++j)
            if (k0 + j < cvr::NVALS) {
                const uint32_t u = (uint32_t)(int32_t)cnt[k0 + j];
                q += cvr::value_write(q, u, cvr::digits_u32(u));
            }
        if (lane == cvr::LANES - 1) *q = '\n';      // (its scan value is the row's: q stands behind the last value)
    }
    __syncthreads();
    if (active) {
        // out: the 16-byte slots of HBM the row touches; whole ones as one store, the two ends by the byte
        char *base = text + at - phase;             // 16-byte aligned, buf[i] belongs to base[i]
        const int end = phase + (int)len;
        for (int s = lane * 16; s < end; s += cvr::LANES * 16) {
            if (s >= phase && s + 16 <= end) {
                *reinterpret_cast<uint4 *>(base + s) = *reinterpret_cast<const uint4 *>(buf + s);
            } else {
                const int lo = s < phase ? phase : s, hi = s + 16 < end ? s + 16 : end;
                for (int i = lo; i < hi; ++i) base[i] = buf[i];
            }
        }
    }
}

constexpr int64_t MAX_ROWS = (int64_t)1 << 30;

// the workspace: the row lengths (rows + 1 int64) | hipcub's
struct rows_ws {
    int64_t *len;
    void *tmp;
    size_t tmp_bytes;
};

int plan(cv_carver &c, int64_t rows, rows_ws *W)
{
    W->len = c.take<int64_t>((size_t)(rows + 1));
    if (cv_scan_temp_bytes<int64_t>(rows + 1, &W->tmp_bytes)) return 1;
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

}  // namespace

extern "C" int cv_tensor_rows_text_workspace(int64_t rows, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_tensor_rows_text_workspace: null argument"); return 1; }
    if (!rows_ok("cv_tensor_rows_text_workspace", rows)) return 1;
    cv_carver c;
    rows_ws W;
    if (plan(c, rows, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_tensor_rows_text_dev(const char *ctg, int64_t ctg_len, const int64_t *centres_dev, int64_t rows,
                                       const uint8_t *ref_dev, int64_t ref_first0, int64_t ref_len, const float *counts_dev,
                                       int64_t *off_dev, uint8_t *status_dev, char *text_dev, int64_t text_cap,
                                       void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_tensor_rows_text_dev";
    if (!rows_ok(who, rows)) return 1;
    if (!ctg || ctg_len < 0 || !off_dev || !workspace || (rows > 0 && (!centres_dev || !counts_dev || !status_dev)) ||
        (ref_len > 0 && !ref_dev) || ref_len < 0 || ref_first0 < 0 || text_cap < 0) {
        cv_set_error("%s: null argument, or a negative length", who);
        return 1;
    }
    if (((uintptr_t)centres_dev & 7) || ((uintptr_t)off_dev & 7) || ((uintptr_t)counts_dev & 15)) {
        cv_set_error("%s: centres / off must be 8-byte, counts 16-byte aligned", who);
        return 1;
    }
    cv_carver c(workspace);
    rows_ws W;
    if (plan(c, rows, &W)) return 1;
    if (!cv_workspace_ok(who, workspace, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (ctg_len > cvr::MAX_CTG) {                   // the whole call is the host's: no lengths, every row CV_ROWTEXT_HOST
        CV_HIP(hipMemsetAsync(off_dev, 0, (size_t)(rows + 1) * 8, st));
        if (rows) CV_HIP(hipMemsetAsync(status_dev, CV_ROWTEXT_HOST, (size_t)rows, st));
        return 0;
    }
    int64_t *len = W.len;
    size_t tb = W.tmp_bytes;
    const unsigned len_blocks = (unsigned)((rows + 1 + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
    hipLaunchKernelGGL(rowtext_len, dim3(len_blocks), dim3(THREADS), 0, st, (int)ctg_len, centres_dev, rows, ref_first0, ref_len,
                       counts_dev, len, status_dev);
    CV_HIP(hipGetLastError());
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int64_t *)len, off_dev, (int)(rows + 1), st));
    if (text_dev && rows) {
        CtgName name;
        memset(&name, 0, sizeof(name));
        memcpy(name.s, ctg, (size_t)ctg_len);
        const unsigned blocks = (unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
        hipLaunchKernelGGL(rowtext_write, dim3(blocks), dim3(THREADS), 0, st, name, (int)ctg_len, centres_dev, rows, ref_dev, ref_first0,
                           ref_len, counts_dev, (const int64_t *)off_dev, (const uint8_t *)status_dev, text_dev, text_cap);
        CV_HIP(hipGetLastError());
    }
    return 0;
}
