// cv_vcfmerge_dev.hip -- the chunk VCFs of callVarBamParallel merged in HBM: the order, the sorted text and the tables of
// a tabix index, from the lines cv_item_lines_dev found in the record bytes of all inputs laid end to end.
// clairvoyante_amd/vcf_merge.py holds the definition, cv_vcfmerge_core.hpp the per-line function, the bins and the record
// copy once for these kernels and for cv_vcf_merge_host_form / cv_vcf_windows_host_form.
//
//   vm_fields      one lane per line: REF and INFO by their tabs -> end, bin, verdict; the key rank << 40 | POS
//   hipcub SortPairs (key, line), stable, over the key bits the data needs -> the permutation
//   vm_sorted      rank, beg, end, bin and length in output order; hipcub ExclusiveSum of the lengths -> ooff[n + 1], the
//                  place of every record in the output and the index's uncompressed offsets
//   vm_gather      one wave per 64 consecutive OUTPUT records, whose text is one contiguous range of the output: every lane
//                  copies its record into LDS at the offset it has in that range (cvm::copy_record: the scattered,
//                  unaligned source read as aligned 16-byte granules and funnel-shifted, no byte loads), the range standing
//                  at the phase (address mod 16) it has in HBM; the wave then stores the range as aligned 16-byte
//                  granules, bytes only at its two ends.  The tile is 16 416 bytes: a workgroup is one wave, nine of them
//                  fit the CU's 160 KiB.  A tile of more than 16 KiB (records of 256 bytes and more) takes the
//                  wave-per-record path: the lanes stride over the destination's dwords, each from two aligned dwords.
//   vm_heads / InclusiveSum / vm_chunks   a head where (rank, bin) changes, one chunk (rank, bin, ubeg, uend) per run; the
//                  per-contig first and last offset, record count and largest end beside them
//   hipcub SortPairs (rank << 16 | bin, chunk), stable -> vm_chunk_out: the chunks in file order per bin
//   vw_fill / vw_min / vw_backfill (cv_vcf_windows_dev)   per contig n_intv windows: the smallest ubeg of a record that
//                  overlaps the window (64-bit vector atomicMin: a minimum is deterministic), then the back-fill, which is
//                  a suffix minimum because the offsets of touched windows ascend
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <string.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_dev_scan.hpp"
#include "cv_vcfmerge_core.hpp"

namespace {

constexpr int LANES = cvm::LANES;
static_assert(cvm::TILE_BYTES % 16 == 0 && 9 * cvm::TILE_BYTES <= 160 * 1024, "nine one-wave workgroups share the CU's 160 KiB");
constexpr uint64_t POS_MASK = ((uint64_t)1 << cvm::POS_BITS) - 1;
typedef unsigned long long u64;

__global__ __launch_bounds__(256) void vm_fields(const char *__restrict__ text, int64_t text_len, int64_t n,
                                                  const int64_t *__restrict__ pos, const int32_t *__restrict__ run,
                                                  const int64_t *__restrict__ off, const int64_t *__restrict__ llen,
                                                  const int32_t *__restrict__ run_rank, int64_t nruns, int32_t nrank,
                                                  uint64_t *__restrict__ key, int64_t *__restrict__ val, int64_t *__restrict__ end,
                                                  int32_t *__restrict__ bin, uint8_t *__restrict__ good, int64_t *__restrict__ info)
{
    CV_GRID_STRIDE(i, n) {
        cvm::Fields f;
        f.verdict = cvm::STATUS_HOST; f.end = 0; f.bin = 0;
        int64_t rank = 0;
        const int64_t o = off[i], l = llen[i];
        const int32_t r = run[i];
        if (o >= 0 && l > 0 && l <= text_len && o <= text_len - l && r >= 0 && r < nruns) {
            rank = run_rank[r];
            if (rank >= 0 && rank < nrank) f = cvm::line_fields(text + o, l, pos[i]);
        }
        const bool ok = f.verdict == cvm::STATUS_DEVICE;
        if (!ok) atomicAdd((u64 *)&info[0], (u64)1);
        key[i] = ok ? (uint64_t)rank << cvm::POS_BITS | (uint64_t)pos[i] : 0;
        val[i] = i;
        end[i] = f.end;
        bin[i] = f.bin;
        good[i] = ok;
    }
}

__global__ __launch_bounds__(256) void vm_sorted(int64_t n, const uint64_t *__restrict__ skey, const int64_t *__restrict__ perm,
                                                  const int64_t *__restrict__ end, const int32_t *__restrict__ bin,
                                                  const uint8_t *__restrict__ good, const int64_t *__restrict__ llen,
                                                  int32_t *__restrict__ srank, int64_t *__restrict__ sbeg, int64_t *__restrict__ send,
                                                  int32_t *__restrict__ sbin, int64_t *__restrict__ slen)
{
    CV_GRID_STRIDE(i, n + 1) {
        if (i == n) { slen[i] = 0; continue; }          // the scan's last input: ooff[n] becomes the total
        const int64_t j = perm[i];
        const uint64_t k = skey[i];
        srank[i] = (int32_t)(k >> cvm::POS_BITS);
        sbeg[i] = (int64_t)(k & POS_MASK) - 1;
        send[i] = end[j];
        sbin[i] = bin[j];
        slen[i] = good[j] ? llen[j] : 0;
    }
}

__global__ __launch_bounds__(LANES) void vm_gather(const char *__restrict__ text, int64_t n, const int64_t *__restrict__ perm,
                                                    const int64_t *__restrict__ off, const int64_t *__restrict__ llen,
                                                    const uint8_t *__restrict__ good, const int64_t *__restrict__ ooff,
                                                    char *__restrict__ out, int64_t out_cap)
{
    __shared__ __attribute__((aligned(16))) char s_text[cvm::TILE_BYTES];
    const int lane = threadIdx.x;
    const int64_t tiles = (n + LANES - 1) / LANES;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = tile * LANES, r = r0 + lane;
        const int64_t cnt = n - r0 < LANES ? n - r0 : LANES;
        const int64_t start = ooff[r0], bytes = ooff[r0 + cnt] - start;      // (wave-uniform)
        if (start < 0 || bytes <= 0 || bytes > out_cap - start) continue;    // nothing of a range that does not fit is written
        if (bytes <= cvm::TILE_TEXT) {
            const int phase = (int)((uintptr_t)(out + start) & 15);
            if (r < n) {
                const int64_t j = perm[r], at = ooff[r], l = llen[j];
                // the length the scan summed -- or the record stays unwritten (vm_fields held off / len to the text)
                if (good[j] && ooff[r + 1] - at == l) cvm::copy_record(s_text, phase + (int)(at - start), text, off[j], (int)l);
            }
            __syncthreads();
            const int end = phase + (int)bytes;
            char *base = out + start - phase;               // 16-byte aligned, s_text[i] belongs to base[i]
            for (int s = lane * 16; s < end; s += LANES * 16) {
                if (s >= phase && s + 16 <= end) {
                    *reinterpret_cast<uint4 *>(base + s) = *reinterpret_cast<const uint4 *>(s_text + s);
                } else {
                    const int lo = s < phase ? phase : s, hi = s + 16 < end ? s + 16 : end;
                    for (int i = lo; i < hi; ++i) base[i] = s_text[i];
                }
            }
            __syncthreads();                                // the next tile of this wave writes s_text again
        } else {
            const uint32_t *text32 = reinterpret_cast<const uint32_t *>(text);
            for (int64_t k = r0; k < r0 + cnt; ++k) {       // record by record, the whole wave on each
                const int64_t j = perm[k], at = ooff[k], l = llen[j], s = off[j];
                if (!good[j] || ooff[k + 1] - at != l) continue;
                char *dst = out + at;
                int64_t head = (4 - (int64_t)((uintptr_t)dst & 3)) & 3;
                if (head > l) head = l;
                const int64_t nw = (l - head) >> 2, p = s + head, a = p >> 2;
                const int sh = (int)(p & 3) * 8;
                uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst + head);
                for (int64_t w = lane; w < nw; w += LANES) {
                    const uint32_t lo = text32[a + w];
                    dst32[w] = sh ? (lo >> sh) | (text32[a + w + 1] << (32 - sh)) : lo;
                }
                const int64_t done = head + 4 * nw;         // the ragged ends: at most three bytes each
                if (lane < head) dst[lane] = text[s + lane];
                if (lane < l - done) dst[done + lane] = text[s + done + lane];
            }
        }
    }
}

__global__ __launch_bounds__(256) void vm_heads(int64_t n, const int32_t *__restrict__ srank, const int32_t *__restrict__ sbin,
                                                 int64_t *__restrict__ head)
{
    CV_GRID_STRIDE(i, n + 1) head[i] = i < n && (i == 0 || srank[i] != srank[i - 1] || sbin[i] != sbin[i - 1]) ? 1 : 0;
}

// inc[i] = heads up to and including record i (record i lies in chunk inc[i] - 1), inc[n] = chunks in all
__global__ __launch_bounds__(256) void vm_chunks(int64_t n, int32_t nrank, const int32_t *__restrict__ srank,
                                                  const int32_t *__restrict__ sbin, const int64_t *__restrict__ send,
                                                  const int64_t *__restrict__ ooff, const int64_t *__restrict__ inc,
                                                  uint64_t *__restrict__ ckey, int64_t *__restrict__ cval, int64_t *__restrict__ cubeg,
                                                  int64_t *__restrict__ cuend, int64_t *__restrict__ stats)
{
    const int64_t nc = inc[n];
    CV_GRID_STRIDE(i, n) {
        const int32_t r = srank[i], b = sbin[i];
        const int64_t c = inc[i] - 1;
        const bool head = i == 0 || inc[i - 1] != inc[i], tail = i == n - 1 || inc[i + 1] != inc[i];
        if (head) { ckey[c] = (uint64_t)(uint32_t)r << 16 | (uint32_t)(b & 0xffff); cval[c] = c; cubeg[c] = ooff[i]; }
        if (tail) cuend[c] = ooff[i + 1];
        if (i >= nc) { ckey[i] = (uint64_t)(uint32_t)nrank << 16; cval[i] = i; }    // the sort's padding: behind every chunk
        if (r < 0 || r >= nrank) continue;
        // per contig: first offset, offset behind the last, records (the tail's index + 1 minus the head's), largest end
        if (i == 0 || srank[i - 1] != r) { stats[r] = ooff[i]; atomicAdd((u64 *)&stats[2 * (int64_t)nrank + r], (u64)(-i)); }
        if (i == n - 1 || srank[i + 1] != r) { stats[nrank + r] = ooff[i + 1]; atomicAdd((u64 *)&stats[2 * (int64_t)nrank + r], (u64)(i + 1)); }
        int64_t *mx = &stats[3 * (int64_t)nrank + r];
        if (send[i] > *(volatile int64_t *)mx) atomicMax((long long *)mx, (long long)send[i]);
    }
}

__global__ __launch_bounds__(256) void vm_chunk_out(int64_t n, const int64_t *__restrict__ inc, const uint64_t *__restrict__ ckey_s,
                                                     const int64_t *__restrict__ cval_s, const int64_t *__restrict__ cubeg,
                                                     const int64_t *__restrict__ cuend, const int64_t *__restrict__ ooff,
                                                     int64_t *__restrict__ chunks, int64_t *__restrict__ info)
{
    const int64_t nc = inc[n];
    CV_GRID_STRIDE(c, n) {
        if (c == 0) { info[1] = nc; info[2] = ooff[n]; }
        if (c >= nc) continue;
        const int64_t v = cval_s[c];
        chunks[c] = (int64_t)(ckey_s[c] >> 16);
        chunks[n + c] = (int64_t)(ckey_s[c] & 0xffff);
        chunks[2 * n + c] = cubeg[v];
        chunks[3 * n + c] = cuend[v];
    }
}

__global__ __launch_bounds__(256) void vw_fill(int64_t nwin, int64_t *__restrict__ win)
{
    CV_GRID_STRIDE(w, nwin) win[w] = cvm::UNSET;
}

__global__ __launch_bounds__(256) void vw_min(int64_t n, const int32_t *__restrict__ srank, const int64_t *__restrict__ sbeg,
                                               const int64_t *__restrict__ send, const int64_t *__restrict__ ooff, int32_t nrank,
                                               const int64_t *__restrict__ win_off, int64_t *__restrict__ win, int64_t nwin)
{
    CV_GRID_STRIDE(i, n) {
        const int32_t r = srank[i];
        const int64_t b = sbeg[i], e = send[i], u = ooff[i];
        if (r < 0 || r >= nrank || b < 0 || e <= b || e > cvm::MAX_END) continue;
        const int64_t base = win_off[r], cnt = win_off[r + 1] - base;
        for (int64_t w = b >> cvm::WINDOW_SHIFT; w <= (e - 1) >> cvm::WINDOW_SHIFT; ++w) {
            if (w >= cnt || base + w < 0 || base + w >= nwin) break;
            int64_t *at = &win[base + w];
            if (u < *(volatile int64_t *)at) atomicMin((long long *)at, (long long)u);
        }
    }
}

// a window nobody touches takes the next one's value: the offsets of touched windows ascend, so this is the minimum over
// the windows from w on.  One workgroup per contig, tiles of 256 windows from the right, the carry in a register.
__global__ __launch_bounds__(256) void vw_backfill(int32_t nrank, const int64_t *__restrict__ win_off, int64_t *__restrict__ win,
                                                    int64_t nwin)
{
    __shared__ int64_t s[256];
    const int t = threadIdx.x;
    for (int32_t r = blockIdx.x; r < nrank; r += gridDim.x) {
        int64_t lo = win_off[r], hi = win_off[r + 1];
        if (lo < 0) lo = 0;
        if (hi > nwin) hi = nwin;
        int64_t carry = cvm::UNSET;
        for (int64_t top = hi; top > lo; top -= 256) {      // (wave-uniform: every thread takes every barrier)
            const int64_t idx = top - 1 - t;                 // thread t: the t-th window from the right
            int64_t v = idx >= lo ? win[idx] : cvm::UNSET;
            s[t] = v;
            __syncthreads();
            for (int d = 1; d < 256; d <<= 1) {
                const int64_t x = t >= d ? s[t - d] : cvm::UNSET;
                __syncthreads();
                if (x < s[t]) s[t] = x;
                __syncthreads();
            }
            v = s[t] < carry ? s[t] : carry;
            if (idx >= lo) win[idx] = v;
            const int64_t all = s[255];
            __syncthreads();
            if (all < carry) carry = all;
        }
    }
}

constexpr int64_t MAX_RECORDS = (int64_t)1 << 30;

// the workspace of cv_vcf_merge_dev
struct merge_ws {
    uint64_t *key, *skey;            // later: the chunk keys, unsorted and sorted
    int64_t *val, *perm;             // later: the chunk numbers, unsorted and sorted
    int64_t *end;                    // later: cubeg
    int64_t *slen;                   // n + 1; later: the head flags, then cuend
    int64_t *inc;                    // n + 1
    int32_t *bin, *sbin;
    uint8_t *good;
    void *tmp;
    size_t tmp_bytes;
};

int plan(cv_carver &c, int64_t n, merge_ws *W)
{
    const size_t m = (size_t)n;
    W->key = c.take<uint64_t>(m); W->skey = c.take<uint64_t>(m);
    W->val = c.take<int64_t>(m); W->perm = c.take<int64_t>(m);
    W->end = c.take<int64_t>(m); W->slen = c.take<int64_t>(m + 1); W->inc = c.take<int64_t>(m + 1);
    W->bin = c.take<int32_t>(m); W->sbin = c.take<int32_t>(m);
    W->good = c.take<uint8_t>(m);
    size_t a = 0, b = 0, d = 0;
    if (cv_sort_pairs_temp_bytes<uint64_t, int64_t>(n, &a) || cv_scan_temp_bytes<int64_t>(n + 1, &b) ||
        cv_inclusive_sum_temp_bytes<int64_t>(n + 1, &d))
        return 1;
    W->tmp_bytes = a > b ? (a > d ? a : d) : (b > d ? b : d);
    W->tmp = c.take_bytes(W->tmp_bytes);
    return 0;
}

bool count_ok(const char *who, int64_t n, int32_t nrank)
{
    if (n < 0 || n > MAX_RECORDS) {
        cv_set_error("%s: %lld records out of range (0 .. %lld)", who, (long long)n, (long long)MAX_RECORDS);
        return false;
    }
    if (nrank < 1 || nrank > cvm::MAX_RANKS) {
        cv_set_error("%s: %d contig ranks out of range (1 .. %d)", who, (int)nrank, cvm::MAX_RANKS);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int cv_vcf_merge_workspace(int64_t n, int64_t *bytes)
{
    const char *who = "cv_vcf_merge_workspace";
    if (!bytes) { cv_set_error("%s: null argument", who); return 1; }
    if (!count_ok(who, n, 1)) return 1;
    cv_carver c;
    merge_ws W;
    if (plan(c, n, &W)) return 1;
    *bytes = (int64_t)c.total();
    return 0;
}

extern "C" int cv_vcf_merge_dev(const char *text_dev, int64_t text_len, int64_t n, const int64_t *pos_dev, const int32_t *run_dev,
                                const int64_t *off_dev, const int64_t *len_dev, const int32_t *run_rank_dev, int64_t nruns,
                                int32_t nrank, int32_t *srank_dev, int64_t *sbeg_dev, int64_t *send_dev, int64_t *ooff_dev,
                                char *out_text_dev, int64_t out_cap, int64_t *chunks_dev, int64_t *stats_dev, int64_t *info_dev,
                                void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_vcf_merge_dev";
    if (!count_ok(who, n, nrank)) return 1;
    if (!ooff_dev || !stats_dev || !info_dev || !workspace || text_len < 0 || out_cap < 0 || nruns < 0 ||
        (n > 0 && (!text_dev || !pos_dev || !run_dev || !off_dev || !len_dev || !run_rank_dev || !srank_dev || !sbeg_dev || !send_dev ||
                   !chunks_dev))) {
        cv_set_error("%s: null argument, or a negative length", who);
        return 1;
    }
    if (((uintptr_t)text_dev & 15) || ((uintptr_t)pos_dev & 7) || ((uintptr_t)off_dev & 7) || ((uintptr_t)len_dev & 7) ||
        ((uintptr_t)sbeg_dev & 7) || ((uintptr_t)send_dev & 7) || ((uintptr_t)ooff_dev & 7) || ((uintptr_t)chunks_dev & 7) ||
        ((uintptr_t)stats_dev & 7) || ((uintptr_t)info_dev & 7) || ((uintptr_t)run_dev & 3) || ((uintptr_t)run_rank_dev & 3) ||
        ((uintptr_t)srank_dev & 3)) {
        cv_set_error("%s: the text must be 16-byte, the int64 arrays 8-byte, the int32 arrays 4-byte aligned", who);
        return 1;
    }
    cv_carver c(workspace);
    merge_ws W;
    if (plan(c, n, &W)) return 1;
    if (!cv_workspace_ok(who, workspace, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    CV_HIP(hipMemsetAsync(info_dev, 0, 8 * sizeof(int64_t), st));
    CV_HIP(hipMemsetAsync(stats_dev, 0, 4 * (size_t)nrank * sizeof(int64_t), st));
    CV_HIP(hipMemsetAsync(ooff_dev, 0, sizeof(int64_t), st));
    if (n == 0) return 0;
    size_t tb = W.tmp_bytes;
    hipLaunchKernelGGL(vm_fields, dim3(cv_grid_for(n)), dim3(256), 0, st, text_dev, text_len, n, pos_dev, run_dev, off_dev, len_dev,
                       run_rank_dev, nruns, nrank, W.key, W.val, W.end, W.bin, W.good, info_dev);
    CV_HIP(hipGetLastError());
    const int key_bits = cvm::POS_BITS + cvm::bits_for(nrank);
    CV_HIP(hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, (const uint64_t *)W.key, W.skey, (const int64_t *)W.val, W.perm, (int)n, 0,
                                              key_bits, st));
    hipLaunchKernelGGL(vm_sorted, dim3(cv_grid_for(n + 1)), dim3(256), 0, st, n, (const uint64_t *)W.skey, (const int64_t *)W.perm,
                       (const int64_t *)W.end, (const int32_t *)W.bin, (const uint8_t *)W.good, len_dev, srank_dev, sbeg_dev, send_dev,
                       W.sbin, W.slen);
    CV_HIP(hipGetLastError());
    tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.tmp, tb, (const int64_t *)W.slen, ooff_dev, (int)(n + 1), st));
    if (out_text_dev) {
        hipLaunchKernelGGL(vm_gather, dim3(cv_grid_for((n + LANES - 1) / LANES, 1, 1 << 16)), dim3(LANES), 0, st, text_dev, n,
                           (const int64_t *)W.perm, off_dev, len_dev, (const uint8_t *)W.good, (const int64_t *)ooff_dev, out_text_dev,
                           out_cap);
        CV_HIP(hipGetLastError());
    }
    // chunks: the flags take the place of the lengths (they are summed), the chunk arrays that of the first sort's
    int64_t *head = W.slen;
    hipLaunchKernelGGL(vm_heads, dim3(cv_grid_for(n + 1)), dim3(256), 0, st, n, (const int32_t *)srank_dev, (const int32_t *)W.sbin, head);
    CV_HIP(hipGetLastError());
    tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceScan::InclusiveSum(W.tmp, tb, (const int64_t *)head, W.inc, (int)(n + 1), st));
    uint64_t *ckey = W.key, *ckey_s = W.skey;
    int64_t *cval = W.val, *cval_s = W.perm, *cubeg = W.end, *cuend = W.slen;
    hipLaunchKernelGGL(vm_chunks, dim3(cv_grid_for(n)), dim3(256), 0, st, n, nrank, (const int32_t *)srank_dev, (const int32_t *)W.sbin,
                       (const int64_t *)send_dev, (const int64_t *)ooff_dev, (const int64_t *)W.inc, ckey, cval, cubeg, cuend, stats_dev);
    CV_HIP(hipGetLastError());
    tb = W.tmp_bytes;
    CV_HIP(hipcub::DeviceRadixSort::SortPairs(W.tmp, tb, (const uint64_t *)ckey, ckey_s, (const int64_t *)cval, cval_s, (int)n, 0,
                                              16 + cvm::bits_for((int64_t)nrank + 1), st));
    hipLaunchKernelGGL(vm_chunk_out, dim3(cv_grid_for(n)), dim3(256), 0, st, n, (const int64_t *)W.inc, (const uint64_t *)ckey_s,
                       (const int64_t *)cval_s, (const int64_t *)cubeg, (const int64_t *)cuend, (const int64_t *)ooff_dev, chunks_dev,
                       info_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_vcf_merge_host_form(const char *text, int64_t text_len, int64_t n, const int64_t *pos, const int32_t *run,
                                      const int64_t *off, const int64_t *len, const int32_t *run_rank, int64_t nruns, int32_t nrank,
                                      int32_t *srank, int64_t *sbeg, int64_t *send, int64_t *ooff, char *out_text, int64_t out_cap,
                                      int64_t *chunks, int64_t *stats, int64_t *info)
{
    const char *who = "cv_vcf_merge_host_form";
    if (!count_ok(who, n, nrank)) return 1;
    if (!ooff || !stats || !info || text_len < 0 || out_cap < 0 || nruns < 0 ||
        (n > 0 && (!text || !pos || !run || !off || !len || !run_rank || !srank || !sbeg || !send || !chunks)) || ((uintptr_t)text & 15)) {
        cv_set_error("%s: null argument, a negative length, or a text that is not 16-byte aligned", who);
        return 1;
    }
    cvm::merge_host_form(text, text_len, n, pos, run, off, len, run_rank, nruns, nrank, srank, sbeg, send, ooff, out_text, out_cap, chunks,
                         stats, info);
    return 0;
}

static bool windows_ok(const char *who, int64_t n, const void *srank, const void *sbeg, const void *send, const void *ooff, int32_t nrank,
                       const void *win_off, const void *win, int64_t nwin)
{
    if (!count_ok(who, n, nrank)) return false;
    if (nwin < 0 || nwin > ((int64_t)1 << 40) || !win_off || (nwin > 0 && !win) || (n > 0 && (!srank || !sbeg || !send || !ooff))) {
        cv_set_error("%s: null argument, or a window count out of range", who);
        return false;
    }
    if (((uintptr_t)sbeg & 7) || ((uintptr_t)send & 7) || ((uintptr_t)ooff & 7) || ((uintptr_t)win_off & 7) || ((uintptr_t)win & 7) ||
        ((uintptr_t)srank & 3)) {
        cv_set_error("%s: the int64 arrays must be 8-byte, srank 4-byte aligned", who);
        return false;
    }
    return true;
}

extern "C" int cv_vcf_windows_dev(int64_t n, const int32_t *srank_dev, const int64_t *sbeg_dev, const int64_t *send_dev,
                                  const int64_t *ooff_dev, int32_t nrank, const int64_t *win_off_dev, int64_t *win_dev, int64_t nwin,
                                  void *stream)
{
    const char *who = "cv_vcf_windows_dev";
    if (!windows_ok(who, n, srank_dev, sbeg_dev, send_dev, ooff_dev, nrank, win_off_dev, win_dev, nwin)) return 1;
    if (nwin == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(vw_fill, dim3(cv_grid_for(nwin)), dim3(256), 0, st, nwin, win_dev);
    CV_HIP(hipGetLastError());
    if (n) {
        hipLaunchKernelGGL(vw_min, dim3(cv_grid_for(n)), dim3(256), 0, st, n, srank_dev, sbeg_dev, send_dev, ooff_dev, nrank, win_off_dev,
                           win_dev, nwin);
        CV_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(vw_backfill, dim3(cv_grid_for(nrank, 1, 1024)), dim3(256), 0, st, nrank, win_off_dev, win_dev, nwin);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_vcf_windows_host_form(int64_t n, const int32_t *srank, const int64_t *sbeg, const int64_t *send, const int64_t *ooff,
                                        int32_t nrank, const int64_t *win_off, int64_t *win, int64_t nwin)
{
    const char *who = "cv_vcf_windows_host_form";
    if (!windows_ok(who, n, srank, sbeg, send, ooff, nrank, win_off, win, nwin)) return 1;
    cvm::windows_host_form(n, srank, sbeg, send, ooff, nrank, win_off, win, nwin);
    return 0;
}
