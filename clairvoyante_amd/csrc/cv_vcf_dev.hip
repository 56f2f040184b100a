// cv_vcf_dev.hip -- the VCF records of callVar.py (:72-153) written in HBM from what cv_call_postproc left there:
// cv_format_vcf's lines, byte for byte, for the candidates cv_vcf_core.hpp vouches for (the host form of that header is
// held to cv_format_vcf by tests/native/vcf_core_driver.cpp).
//
//   vcf_len     one lane per candidate: record<Count> -> the line's length and the status (NONE / DEVICE / HOST); a wave
//               adds its records and its HOST candidates to info with one atomic each
//   hipcub ExclusiveSum over the n + 1 lengths -> off[n + 1]
//   vcf_write   one lane per DEVICE candidate: record<Write> at text + off[i]; lane 0 of the grid stores info[0] = off[n]
//
// A record is ~53 bytes and a candidate reads at most 17 positions x 8 floats of its row, so a lane per candidate and byte
// stores are enough; nothing here is staged.  Nothing behind off[n] is written; a line that does not fit below text_cap
// is not written at all.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_dev_scan.hpp"
#include "cv_vcf_core.hpp"


static_assert(CV_VCF_NONE == cvv::NONE && CV_VCF_DEVICE == cvv::DEVICE && CV_VCF_HOST == cvv::HOST, "the header's status words");

namespace {

constexpr int THREADS = 256;
constexpr int64_t MAX_N = (int64_t)1 << 30;

struct Batch {
    const int32_t *call; const float *qual; const float *x; const int64_t *xrow;
    const char *pos_buf; const int64_t *pos_meta; const int64_t *pos_row;
    int show_ref, has_qual, qual_min;
};

__host__ __device__ inline cvv::Cand cand_of(const Batch &b, int64_t i)
{
    return cvv::candidate(b.call, b.qual, b.x, b.xrow, b.pos_buf, b.pos_meta, b.pos_row, b.show_ref, b.has_qual, b.qual_min, i);
}

// len_out[i] = bytes of line i (0 for NONE and HOST), len_out[n] = 0 (the scan's last input: off[n] becomes the total);
// info[1] += records, info[2] += HOST candidates (info is zero when the kernel starts)
__global__ __launch_bounds__(THREADS) void vcf_len(Batch b, int64_t n, int64_t *__restrict__ len_out, uint8_t *__restrict__ status,
                                                   unsigned long long *__restrict__ info)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    int st = cvv::NONE;
    if (i < n) {
        cvv::Count s{0};
        int why;
        st = cvv::record(cand_of(b, i), s, &why);
        len_out[i] = st == cvv::DEVICE ? (int64_t)s.n : 0;
        status[i] = (uint8_t)st;
    } else if (i == n) {
        len_out[n] = 0;
    }
    // (every lane of the wave is here: the ballots see the whole wave)
    const unsigned long long dev = __ballot(st == cvv::DEVICE), host = __ballot(st == cvv::HOST);
    if ((threadIdx.x & 63) == 0) {
        if (dev) atomicAdd(info + 1, (unsigned long long)__popcll(dev));
        if (host) atomicAdd(info + 2, (unsigned long long)__popcll(host));
    }
}

__global__ __launch_bounds__(THREADS) void vcf_write(Batch b, int64_t n, const int64_t *__restrict__ off, const uint8_t *__restrict__ status,
                                                     int64_t *__restrict__ info, char *__restrict__ text, int64_t text_cap)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i == 0) info[0] = off[n];
    if (i >= n || !text || status[i] != cvv::DEVICE) return;
    const int64_t at = off[i], len = off[i + 1] - at;
    if (len <= 0 || at < 0 || at + len > text_cap) return;
    cvv::Write s{text + at};
    int why;
    cvv::record(cand_of(b, i), s, &why);
}

// the workspace: the record lengths (n + 1 int64) | hipcub's
struct records_ws {
    int64_t *len;
    void *tmp;
    size_t tmp_bytes;
};

int plan(cv_carver &c, int64_t n, records_ws *W)
{
    W->len = c.take<int64_t>((size_t)(n + 1));
    if (cv_scan_temp_bytes<int64_t>(n + 1, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool n_ok(const char *who, int64_t n)
{
    if (n < 0 || n > MAX_N) {
        cv_set_error("%s: %lld candidates out of range (0 .. %lld)", who, (long long)n, (long long)MAX_N);
        return false;
    }
    return true;
}

// the pointers of a batch: all there, 4-byte (call, qual, x) and 8-byte (the int64 arrays) aligned
bool batch_ok(const char *who, const Batch &b, const int64_t *off, const uint8_t *status, const int64_t *info, int64_t text_cap)
{
    if (!b.call || !b.qual || !b.x || !b.pos_buf || !b.pos_meta || !off || !status || !info || text_cap < 0) {
        cv_set_error("%s: null argument, or a negative capacity", who);
        return false;
    }
    if (((uintptr_t)b.call & 3) || ((uintptr_t)b.qual & 3) || ((uintptr_t)b.x & 3) || ((uintptr_t)b.xrow & 7) || ((uintptr_t)b.pos_meta & 7) ||
        ((uintptr_t)b.pos_row & 7) || ((uintptr_t)off & 7) || ((uintptr_t)info & 7)) {
        cv_set_error("%s: call / qual / x must be 4-byte, xrow / pos_meta / pos_row / off / info 8-byte aligned", who);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int cv_vcf_records_workspace(int64_t n, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_vcf_records_workspace: null argument"); return 1; }
    if (!n_ok("cv_vcf_records_workspace", n)) return 1;
    cv_carver c;
    records_ws W;
    if (plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_vcf_records_dev(const int32_t *call_dev, const float *qual_dev, int64_t n, const float *x_dev, const int64_t *xrow_dev,
                                  const char *pos_buf_dev, const int64_t *pos_meta_dev, const int64_t *pos_row_dev, int show_ref,
                                  int has_qual, int qual_min, int64_t *off_dev, uint8_t *status_dev, int64_t *info_dev, char *text_dev,
                                  int64_t text_cap, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_vcf_records_dev";
    if (!n_ok(who, n)) return 1;
    if (n == 0) return 0;
    const Batch b{call_dev, qual_dev, x_dev, xrow_dev, pos_buf_dev, pos_meta_dev, pos_row_dev, show_ref, has_qual, qual_min};
    if (!batch_ok(who, b, off_dev, status_dev, info_dev, text_cap)) return 1;
    cv_carver c(workspace);
    records_ws W;
    if (plan(c, n, &W)) return 1;
    if (!cv_workspace_ok(who, workspace, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    int64_t *len = W.len;
    size_t tb = W.tmp_bytes;
    CV_HIP(hipMemsetAsync(info_dev, 0, 32, st));
    hipLaunchKernelGGL(vcf_len, dim3((unsigned)((n + 1 + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, b, n, len, status_dev,
                       (unsigned long long *)info_dev);
    CV_HIP(hipGetLastError());
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int64_t *)len, off_dev, (int)(n + 1), st));
    hipLaunchKernelGGL(vcf_write, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, b, n, (const int64_t *)off_dev,
                       (const uint8_t *)status_dev, info_dev, text_dev, text_cap);
    CV_HIP(hipGetLastError());
    return 0;
}

// the same core on the CPU, one candidate after the other: what the kernels must give, byte for byte
extern "C" int cv_vcf_records_host_form(const int32_t *call, const float *qual, int64_t n, const float *x, const int64_t *xrow,
                                        const char *pos_buf, const int64_t *pos_meta, const int64_t *pos_row, int show_ref, int has_qual,
                                        int qual_min, int64_t *off, uint8_t *status, int64_t *info, char *text, int64_t text_cap)
{
    const char *who = "cv_vcf_records_host_form";
    if (!n_ok(who, n)) return 1;
    if (n == 0) return 0;
    const Batch b{call, qual, x, xrow, pos_buf, pos_meta, pos_row, show_ref, has_qual, qual_min};
    if (!batch_ok(who, b, off, status, info, text_cap)) return 1;
    int64_t at = 0, recs = 0, hosts = 0;
    for (int64_t i = 0; i < n; i++) {
        const cvv::Cand k = cand_of(b, i);
        cvv::Count s{0};
        int why;
        const int st = cvv::record(k, s, &why);
        status[i] = (uint8_t)st;
        off[i] = at;
        if (st == cvv::HOST) hosts++;
        if (st != cvv::DEVICE) continue;
        recs++;
        if (text && at + s.n <= text_cap) { cvv::Write w{text + at}; cvv::record(k, w, &why); }
        at += s.n;
    }
    off[n] = at;
    info[0] = at; info[1] = recs; info[2] = hosts; info[3] = 0;
    return 0;
}
