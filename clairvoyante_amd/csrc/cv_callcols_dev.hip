// cv_callcols_dev.hip -- callVarBam's hop between the pileup and the call loop, in HBM: which candidate centres give a
// row (touched, the window starts inside the loaded reference, the centre base is ACGT) and the tokens of those rows in the
// layout of utils_v2.PosBatch.from_columns -- contig name, all coordinates end to end, all upper-cased reference windows
// end to end, meta [k,6] -- byte for byte.  cv_callcols_core.hpp holds the verdict, the digits and the window; its host
// form is held to the Python definition by tests/test_call_columns_host.py.
//
//   cc_verdict   one lane per centre: row_of() -> a[i] = kept << 32 | digits, b[i] = window bytes; a[n] = b[n] = 0
//   hipcub ExclusiveSum over the n + 1 values of a and of b: in front of centre i, the kept rows (the row's rank: the
//                compaction is stable), their digits and their window bytes; at n, the totals
//   cc_write     16 lanes per centre (16 centres per workgroup): a kept centre's lanes store its index, the six values of
//                its meta, its digits and its window.  Neighbouring lane groups hold neighbouring rows, whose coordinates
//                and windows are neighbours in the text, so a wave's stores fall into a few runs of bytes.  Workgroup 0 also
//                lays down the contig name and info = {k, bytes of text, n, 0}
//
// The text is at most ctg_len + 43 n bytes, known before anything runs: there is no sizing pass, and nothing behind
// info[1] is written.  At most 2^27 centres, so that the digits in front of a row fit the low half of a.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_dev_scan.hpp"
#include "cv_callcols_core.hpp"

int cv_pileup_centres_dev(const cv_pileup *p, const int32_t **centres_dev, const uint8_t **flags_dev, const uint8_t **ref_dev,
                          int64_t *ref_first, int64_t *ref_len, int64_t *n);      // cv_pileup.hip

static_assert(CV_CALL_COLUMNS_MAX_CTG == 1024 && CV_CALL_COLUMNS_ROW_TEXT == cvk::MAX_ROW_TEXT, "the header's bounds");

namespace {

constexpr int THREADS = 256;
constexpr int GROUP = 16;                         // lanes of a centre in cc_write
constexpr int PER_BLOCK = THREADS / GROUP;
constexpr int64_t MAX_N = (int64_t)1 << 27;
static_assert(MAX_N * cvk::MAX_DIGITS < ((int64_t)1 << 32), "the digits in front of a row fit 32 bits");

struct CtgName { char s[CV_CALL_COLUMNS_MAX_CTG]; };

__global__ __launch_bounds__(THREADS) void cc_verdict(int64_t n, const int32_t *__restrict__ centres, const uint8_t *__restrict__ touched,
                                                      const uint8_t *__restrict__ ref, int64_t ref_first, int64_t ref_len,
                                                      int64_t *__restrict__ a, int64_t *__restrict__ b)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i > n) return;
    int64_t va = 0, vb = 0;
    if (i < n) {
        const cvk::Row r = cvk::row_of(centres[i], touched[i] != 0, ref, ref_first, ref_len);
        if (r.keep) { va = ((int64_t)1 << 32) | r.digits; vb = r.wlen; }
    }
    a[i] = va;                                    // (i == n: the scans' last input, so that a[n] / b[n] become the totals)
    b[i] = vb;
}

__global__ __launch_bounds__(THREADS) void cc_write(CtgName ctg, int64_t ctg_len, int64_t n, const int32_t *__restrict__ centres,
                                                    const uint8_t *__restrict__ ref, int64_t ref_first,
                                                    const int64_t *__restrict__ a, const int64_t *__restrict__ b,
                                                    int64_t *__restrict__ index, int64_t *__restrict__ meta, char *__restrict__ text,
                                                    int64_t text_cap, int64_t *__restrict__ info)
{
    const int64_t all_digits = a[n] & 0xffffffffll;
    if (blockIdx.x == 0) {
        for (int t = threadIdx.x; t < ctg_len; t += THREADS) text[t] = ctg.s[t];
        if (threadIdx.x < 4)
            info[threadIdx.x] = threadIdx.x == 0 ? a[n] >> 32 : threadIdx.x == 1 ? ctg_len + all_digits + b[n] : threadIdx.x == 2 ? n : 0;
    }
    const int l = threadIdx.x & (GROUP - 1);
    const int64_t i = (int64_t)blockIdx.x * PER_BLOCK + (threadIdx.x / GROUP);
    if (i >= n) return;
    const int64_t a0 = a[i], a1 = a[i + 1];
    if ((a1 >> 32) == (a0 >> 32)) return;         // not kept
    const int64_t j = a0 >> 32;                   // kept rows in front of it
    const int nd = (int)((a1 - a0) & 0xffffffffll);
    const int64_t w_before = b[i];
    const int wlen = (int)(b[i + 1] - w_before);
    const int64_t coord_at = ctg_len + (a0 & 0xffffffffll), seq_at = ctg_len + all_digits + w_before;
    if (j >= n || nd > cvk::MAX_DIGITS || wlen > cvk::WIDTH || seq_at + wlen > text_cap) return;     // (cannot be: the bound holds)
    const int64_t c = centres[i];
    const int64_t w0 = c - 1 - ref_first - cvk::FLANK;
    if (l == 0) index[j] = i;
    if (l < 6) meta[j * 6 + l] = cvk::meta_at(l, ctg_len, coord_at, nd, seq_at, wlen);
    if (l < nd) text[coord_at + l] = cvk::digit_at(c, nd, l);
    for (int t = l; t < wlen; t += GROUP) text[seq_at + t] = (char)cvk::upper(ref[w0 + t]);
}

// the workspace: a_in | b_in | a_out | b_out (n + 1 int64 each) | hipcub's
struct columns_ws {
    int64_t *a_in, *b_in, *a, *b;
    void *tmp;
    size_t tmp_bytes;
};

int plan(cv_carver &c, int64_t n, columns_ws *W)
{
    W->a_in = c.take<int64_t>((size_t)(n + 1));
    W->b_in = c.take<int64_t>((size_t)(n + 1));
    W->a = c.take<int64_t>((size_t)(n + 1));
    W->b = c.take<int64_t>((size_t)(n + 1));
    if (cv_scan_temp_bytes<int64_t>(n + 1, &W->tmp_bytes)) return 1;
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool args_ok(const char *who, const char *ctg, int64_t ctg_len, int64_t n, int64_t ref_first, int64_t ref_len)
{
    if (n < 0 || n > MAX_N) {
        cv_set_error("%s: %lld centres out of range (0 .. %lld)", who, (long long)n, (long long)MAX_N);
        return false;
    }
    if (ctg_len < 0 || ctg_len > CV_CALL_COLUMNS_MAX_CTG || (ctg_len > 0 && !ctg)) {
        cv_set_error("%s: a contig name of %lld bytes (0 .. %d), or none", who, (long long)ctg_len, CV_CALL_COLUMNS_MAX_CTG);
        return false;
    }
    if (ref_first < 0 || ref_len < 0) {
        cv_set_error("%s: the reference starts at %lld and holds %lld bytes", who, (long long)ref_first, (long long)ref_len);
        return false;
    }
    return true;
}

bool outputs_ok(const char *who, int64_t n, int64_t ctg_len, const void *centres, const void *touched, const void *ref, int64_t ref_len,
                const int64_t *index, const int64_t *meta, const char *text, int64_t text_cap, const int64_t *info)
{
    if (!info || !text || (n > 0 && (!centres || !touched || !index || !meta)) || (ref_len > 0 && !ref)) {
        cv_set_error("%s: null argument", who);
        return false;
    }
    if (((uintptr_t)centres & 3) || ((uintptr_t)index & 7) || ((uintptr_t)meta & 7) || ((uintptr_t)info & 7)) {
        cv_set_error("%s: the centres must be 4-byte, index / meta / info 8-byte aligned", who);
        return false;
    }
    if (text_cap < ctg_len + cvk::MAX_ROW_TEXT * n) {
        cv_set_error("%s: text_cap %lld is below the bound %lld (contig name + 43 bytes per centre)", who, (long long)text_cap,
                     (long long)(ctg_len + cvk::MAX_ROW_TEXT * n));
        return false;
    }
    return true;
}

int run_dev(const char *who, const char *ctg, int64_t ctg_len, const int32_t *centres, const uint8_t *touched, int64_t n, const uint8_t *ref,
            int64_t ref_first, int64_t ref_len, int64_t *index, int64_t *meta, char *text, int64_t text_cap, int64_t *info, void *workspace,
            int64_t workspace_bytes, void *stream)
{
    if (!args_ok(who, ctg, ctg_len, n, ref_first, ref_len)) return 1;
    if (!outputs_ok(who, n, ctg_len, centres, touched, ref, ref_len, index, meta, text, text_cap, info)) return 1;
    cv_carver c(workspace);
    columns_ws W;
    if (plan(c, n, &W)) return 1;
    if (!cv_workspace_ok(who, workspace, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    int64_t *a_in = W.a_in, *b_in = W.b_in, *a = W.a, *b = W.b;
    void *tmp = W.tmp;
    size_t tb = W.tmp_bytes;
    CtgName name;
    for (int64_t t = 0; t < CV_CALL_COLUMNS_MAX_CTG; t++) name.s[t] = t < ctg_len ? ctg[t] : 0;
    hipLaunchKernelGGL(cc_verdict, dim3((unsigned)((n + 1 + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, n, centres, touched, ref, ref_first,
                       ref_len, a_in, b_in);
    CV_HIP(hipGetLastError());
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, (const int64_t *)a_in, a, (int)(n + 1), st));
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, (const int64_t *)b_in, b, (int)(n + 1), st));
    const int64_t blocks = n > 0 ? (n + PER_BLOCK - 1) / PER_BLOCK : 1;
    hipLaunchKernelGGL(cc_write, dim3((unsigned)blocks), dim3(THREADS), 0, st, name, ctg_len, n, centres, ref, ref_first, (const int64_t *)a,
                       (const int64_t *)b, index, meta, text, text_cap, info);
    CV_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int cv_call_columns_workspace(int64_t n, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_call_columns_workspace: null argument"); return 1; }
    if (n < 0 || n > MAX_N) {
        cv_set_error("cv_call_columns_workspace: %lld centres out of range (0 .. %lld)", (long long)n, (long long)MAX_N);
        return 1;
    }
    cv_carver c;
    columns_ws W;
    if (plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_call_columns_dev(const char *ctg, int64_t ctg_len, const int32_t *centres_dev, const uint8_t *touched_dev, int64_t n,
                                   const uint8_t *ref_dev, int64_t ref_first, int64_t ref_len, int64_t *index_dev, int64_t *meta_dev,
                                   char *text_dev, int64_t text_cap, int64_t *info_dev, void *workspace, int64_t workspace_bytes,
                                   void *stream)
{
    return run_dev("cv_call_columns_dev", ctg, ctg_len, centres_dev, touched_dev, n, ref_dev, ref_first, ref_len, index_dev, meta_dev, text_dev,
                   text_cap, info_dev, workspace, workspace_bytes, stream);
}

extern "C" int cv_pileup_call_columns(const cv_pileup *p, const char *ctg, int64_t ctg_len, const uint8_t *touched_dev, int64_t *index_dev,
                                      int64_t *meta_dev, char *text_dev, int64_t text_cap, int64_t *info_dev, void *workspace,
                                      int64_t workspace_bytes, void *stream)
{
    const int32_t *centres;
    const uint8_t *cflags, *ref;
    int64_t ref_first, ref_len, n;
    if (cv_pileup_centres_dev(p, &centres, &cflags, &ref, &ref_first, &ref_len, &n)) return 1;
    return run_dev("cv_pileup_call_columns", ctg, ctg_len, centres, touched_dev, n, ref, ref_first, ref_len, index_dev, meta_dev, text_dev,
                   text_cap, info_dev, workspace, workspace_bytes, stream);
}

// the same core on the CPU over HOST pointers: what the kernels must give, byte for byte
extern "C" int cv_call_columns_host_form(const char *ctg, int64_t ctg_len, const int32_t *centres, const uint8_t *touched, int64_t n,
                                         const uint8_t *ref, int64_t ref_first, int64_t ref_len, int64_t *index, int64_t *meta, char *text,
                                         int64_t text_cap, int64_t *info)
{
    const char *who = "cv_call_columns_host_form";
    if (!args_ok(who, ctg, ctg_len, n, ref_first, ref_len)) return 1;
    if (!outputs_ok(who, n, ctg_len, centres, touched, ref, ref_len, index, meta, text, text_cap, info)) return 1;
    cvk::host_form(ctg, ctg_len, centres, touched, n, ref, ref_first, ref_len, index, meta, text, info);
    return 0;
}
