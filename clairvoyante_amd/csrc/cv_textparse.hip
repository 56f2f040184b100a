// cv_textparse.hip -- the text-tensor reader on the device: a slab of text in HBM -> rows [lines,528] fp32.
// The host reader (cv_hostio.cpp, cv_parse_tensor_text) is the checker of this one and the only parser of lines that
// are not in the producer's format (dataPrepScripts/CreateTensor.py:24,56: "%s %d %s" + 528 x " %0.1f"): such a line
// gets status HOST here and is neither accepted nor rejected.
//
//   tp_count_newlines   per 4 KiB tile of the slab: number of '\n' (16-byte loads, a grid-stride loop over tiles)
//   hipcub ExclusiveSum tile counts -> number of the first line that ENDS in each tile (+ the total behind the last)
//   tp_line_ends        the tiles again: line_end[i] = byte offset of the newline that closes line i (i < max_lines)
//   tp_begin            info = {bytes consumed, lines, 0, 0}
//   tp_parse_rows       one wave per line: the line goes to LDS in 1 KiB steps, 64 bytes are classified at a time,
//                       __ballot gives the masks of blanks and token starts, the lane that owns a token start parses
//                       that token (<= 12 bytes) from LDS into an LDS row, the wave checks the row, subtracts matrix 0
//                       and stores it with 16-byte stores
//   tp_gather_rows      rows named by an index list, in list order, into a dense tensor (cv_text_gather_rows)
//   tp_find_newline     the first newline at or behind a few given offsets (cv_text_find_newline_dev): where the lines
//                       of ONE rank begin and end in text that several ranks share
//
// The slab may start at any address: the kernels read the 16-byte granules that CONTAIN the slab (so up to 15 bytes in
// front of it and behind it, inside the granules the allocation owns anyway) and mask what lies outside.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_internal.hpp"
#include "cv_dev_scan.hpp"

namespace {

constexpr int NV = CV_INPUT_H * CV_INPUT_W * CV_INPUT_C;     // 528
constexpr int TILE_THREADS = 256;
constexpr int TILE = TILE_THREADS * 16;                      // bytes of the slab one block looks at per step
constexpr int INDEX_GRID = 2048;
constexpr int WAVE = 64;
constexpr int PARSE_WAVES = 4;                               // waves (= lines in flight) per block of tp_parse_rows
constexpr int LINE_LDS = CV_TEXT_LINE_CAP + 32;              // a line of the cap at any offset inside its first granule
constexpr int PARSE_GRID = 2048;
constexpr int FIND_GRID = 1024;                              // blocks of tp_find_newline: 4 MiB of text per step of the grid

__device__ __forceinline__ uint32_t newline_mask(const uint4 v, int64_t g0, int64_t lo, int64_t hi)
{
    // bit k = byte k of the granule at granule-relative offset g0 is '\n' and lies inside [lo, hi)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        m |= (uint32_t)(b == 10u) << k;
    }
    if (g0 < lo) { const int64_t d = lo - g0; m = d >= 16 ? 0u : m & (0xffffu << d); }
    if (g0 + 16 > hi) { const int64_t d = hi - g0; m = d <= 0 ? 0u : m & (0xffffu >> (16 - d)); }
    return m;
}

// `gran` = the 16-byte granule that holds the slab's first byte, `shift` = offset of that byte inside it
__global__ __launch_bounds__(TILE_THREADS) void tp_count_newlines(const uint4 *gran, int shift, int64_t len, int64_t ntiles,
                                                                   uint32_t *tile_cnt)
{
    using Reduce = hipcub::BlockReduce<uint32_t, TILE_THREADS>;
    __shared__ typename Reduce::TempStorage tmp;
    const int64_t lo = shift, hi = shift + len;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t g0 = t * TILE + (int64_t)threadIdx.x * 16;
        uint32_t c = 0;
        if (g0 < hi) c = (uint32_t)__popc(newline_mask(gran[g0 >> 4], g0, lo, hi));
        const uint32_t sum = Reduce(tmp).Sum(c);
        if (threadIdx.x == 0) tile_cnt[t] = sum;
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_cnt[ntiles] = 0;        // its scanned value is the total
}

__global__ __launch_bounds__(TILE_THREADS) void tp_line_ends(const uint4 *gran, int shift, int64_t len, int64_t ntiles,
                                                              const uint32_t *tile_first, int64_t max_lines, int64_t *line_end)
{
    using Scan = hipcub::BlockScan<uint32_t, TILE_THREADS>;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t lo = shift, hi = shift + len;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t first = tile_first[t];
        if (first >= max_lines) continue;                                  // (uniform over the block)
        const int64_t g0 = t * TILE + (int64_t)threadIdx.x * 16;
        uint32_t m = 0;
        if (g0 < hi) m = newline_mask(gran[g0 >> 4], g0, lo, hi);
        uint32_t before = 0;
        Scan(tmp).ExclusiveSum((uint32_t)__popc(m), before);
        int64_t line = first + before;
        while (m && line < max_lines) {
            const int k = __ffs(m) - 1;
            line_end[line++] = g0 + k - shift;
            m &= m - 1;
        }
        __syncthreads();
    }
}

__global__ void tp_begin(const uint32_t *tile_first, int64_t ntiles, int64_t max_lines, const int64_t *line_end, int64_t *info)
{
    if (blockIdx.x || threadIdx.x) return;
    int64_t lines = ntiles > 0 ? (int64_t)tile_first[ntiles] : 0;
    if (lines > max_lines) lines = max_lines;
    info[0] = lines > 0 ? line_end[lines - 1] + 1 : 0;
    info[1] = lines;
    info[2] = 0;
    info[3] = 0;
}

// LDS written by some lanes of a wave is read by others: order the accesses within the wave
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t lanes_below() { return (1ull << (threadIdx.x & (WAVE - 1))) - 1ull; }

// the ten constants of cv_hostio.cpp's parse_row_fast (copied to LDS by tp_parse_rows: a lane looks its digit up there,
// a divergent load from global memory per token cost more than the rest of the token)
__device__ const double tp_tenth[10] = {0.0 / 10.0, 1.0 / 10.0, 2.0 / 10.0, 3.0 / 10.0, 4.0 / 10.0,
                                        5.0 / 10.0, 6.0 / 10.0, 7.0 / 10.0, 8.0 / 10.0, 9.0 / 10.0};

// One value token "[-]d{1,9}[.d]" that starts at L[j] and must end at a blank or at the end of the line (L[n..] is
// never read).  Returns false for anything else.
__device__ __forceinline__ bool parse_value(const unsigned char *L, int j, int n, const double *tenth, float *out)
{
    auto at = [&](int k) -> unsigned { return k < n ? (unsigned)L[k] : 10u; };
    const bool neg = at(j) == '-';
    j += neg;
    unsigned d = at(j) - '0';
    if (d > 9) return false;
    uint32_t ip = d;
    int nd = 1;
    j++;
    while (nd <= 9 && (d = at(j) - '0') <= 9) { ip = ip * 10u + d; j++; nd++; }
    if (nd > 9) return false;                               // ten digits or more: the host's general path
    double v = (double)ip;
    if (at(j) == '.') {
        const unsigned f = at(j + 1) - '0';
        if (f > 9) return false;
        v += tenth[f];
        j += 2;
    }
    const unsigned e = at(j);
    if (e != ' ' && e != 10u) return false;
    *out = (float)(neg ? -v : v);
    return true;
}

__global__ __launch_bounds__(PARSE_WAVES * WAVE) void tp_parse_rows(const uint4 *gran, int shift, const int64_t *line_end,
                                                                     int64_t *info, float *x, int64_t *meta, uint8_t *status)
{
    __shared__ uint4 text_lds[PARSE_WAVES][LINE_LDS / 16];
    __shared__ float4 row_lds[PARSE_WAVES][NV / 4];
    __shared__ double tenth_lds[10];
    if (threadIdx.x < 10) tenth_lds[threadIdx.x] = tp_tenth[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int64_t lines = info[1];
    const int64_t nwaves = (int64_t)gridDim.x * PARSE_WAVES;
    unsigned long long n_row = 0, n_host = 0;
    float *row = (float *)row_lds[w];
    for (int64_t i = (int64_t)blockIdx.x * PARSE_WAVES + w; i < lines; i += nwaves) {
        const int64_t start = i ? line_end[i - 1] + 1 : 0;
        const int64_t n64 = line_end[i] - start;             // bytes of the line without its newline
        uint8_t st = CV_TEXT_ROW;
        int64_t sp[3] = {0, 0, 0};
        if (n64 == 0) st = CV_TEXT_SKIP;
        else if (n64 > CV_TEXT_LINE_CAP) st = CV_TEXT_HOST;
        else {
            const int n = (int)n64;
            const int64_t a = shift + start;                  // offset of the line's first byte from granule 0
            const int head = (int)(a & 15);
            const int ngran = (head + n + 15) >> 4;
            for (int g = lane; g < ngran; g += WAVE) text_lds[w][g] = gran[(a >> 4) + g];
            wave_sync();
            const unsigned char *L = (const unsigned char *)text_lds[w] + head;
            // pass over the line, 64 bytes at a time: blanks, forbidden bytes, the first three blanks
            int nblank = 0;
            bool bad = L[0] == ' ' || L[n - 1] == ' ';        // (wave-uniform reads)
            int carry_blank = 0;                              // the byte in front of this step was a blank
            for (int b = 0; b < n && !bad; b += WAVE) {
                const int j = b + lane;
                const unsigned c = j < n ? (unsigned)L[j] : 'x';
                const uint64_t blank = __ballot(c == ' ');
                const uint64_t other = __ballot(c == '\t' || c == '\r' || c == '\v' || c == '\f');
                if (other || (blank & (blank << 1)) || (carry_blank && (blank & 1))) { bad = true; break; }
                carry_blank = (int)(blank >> 63);
                // the first three blanks close the three header tokens
                uint64_t m = blank;
                while (m && nblank < 3) { sp[nblank++] = b + __ffsll((long long)m) - 1; m &= m - 1; }
                if (nblank >= 3) nblank += __popcll(m);
            }
            if (bad || nblank != 3 + NV - 1) st = CV_TEXT_HOST;        // 3 header tokens + 528 values: 530 blanks
            else {
                // values: every byte behind a blank, from the third blank on, starts a token
                const int v0 = (int)sp[2];
                int before = 0;                                // value tokens in front of this step
                int ok = 1;
                for (int b = v0 & ~(WAVE - 1); b < n; b += WAVE) {
                    const int j = b + lane;
                    const bool starts = j > v0 && j < n && L[j - 1] == ' ';
                    const uint64_t sm = __ballot(starts);
                    if (starts) {
                        const int t = before + __popcll(sm & lanes_below());
                        float v;
                        if (parse_value(L, j, n, tenth_lds, &v)) row[t] = v;      // t < 528: the line has 530 blanks
                        else ok = 0;
                    }
                    before += __popcll(sm);
                }
                if (__ballot(!ok)) st = CV_TEXT_HOST;
                else {
                    const int sl = (int)(sp[2] - sp[1] - 1);
                    unsigned c = sl > CV_INPUT_H / 2 ? (unsigned)L[sp[1] + 1 + CV_INPUT_H / 2] : 0u;
                    if (c >= 'a' && c <= 'z') c -= 32;
                    if (c != 'A' && c != 'C' && c != 'G' && c != 'T') st = CV_TEXT_SKIP;
                }
            }
            if (st == CV_TEXT_ROW) {
                wave_sync();
                float4 *dst = (float4 *)(x + i * NV);
                for (int e = lane; e < NV / 4; e += WAVE) {
                    float4 q = row_lds[w][e];
                    q.y -= q.x; q.z -= q.x; q.w -= q.x;
                    dst[e] = q;
                }
                if (lane < 6) {
                    const int k = lane >> 1;
                    const int64_t tb = k == 0 ? 0 : sp[k - 1] + 1;
                    meta[i * 6 + lane] = (lane & 1) ? sp[k] - tb : start + tb;
                }
            }
            wave_sync();                   // the LDS line and row are reused by the next line
        }
        if (lane == 0) status[i] = st;
        n_row += st == CV_TEXT_ROW;
        n_host += st == CV_TEXT_HOST;
    }
    if (lane == 0) {
        if (n_row) atomicAdd((unsigned long long *)&info[2], n_row);
        if (n_host) atomicAdd((unsigned long long *)&info[3], n_host);
    }
}

__global__ __launch_bounds__(256) void tp_gather_rows(const float4 *x, const int64_t *idx, int64_t nrows, float4 *out)
{
    const int64_t total = nrows * (NV / 4);
    CV_GRID_STRIDE(e, total) {
        const int64_t r = e / (NV / 4), c = e - r * (NV / 4);
        out[e] = x[idx[r] * (NV / 4) + c];
    }
}

// cv_text_gather_tokens: the three header tokens of the lines idx[0 .. nrows) back to back.  One workgroup walks the
// lines in steps of its size and scans their token lengths (the offsets of a line depend on every line in front of it);
// a grid then copies the ~60 bytes of each line.
constexpr int TOKEN_THREADS = 1024;

__global__ __launch_bounds__(TOKEN_THREADS) void tp_token_offsets(const int64_t *meta, const int64_t *idx, int64_t nrows, int64_t *meta_out)
{
    typedef hipcub::BlockScan<int64_t, TOKEN_THREADS> scan_t;
    __shared__ typename scan_t::TempStorage tmp;
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t r0 = 0; r0 < nrows; r0 += TOKEN_THREADS) {
        const int64_t r = r0 + threadIdx.x;
        int64_t l0 = 0, l1 = 0, l2 = 0;
        if (r < nrows) {
            const int64_t *m = meta + idx[r] * 6;
            l0 = m[1] > 0 ? m[1] : 0; l1 = m[3] > 0 ? m[3] : 0; l2 = m[5] > 0 ? m[5] : 0;
        }
        int64_t before, total;
        scan_t(tmp).ExclusiveSum(l0 + l1 + l2, before, total);
        const int64_t base = carry + before;
        if (r < nrows) {
            int64_t *o = meta_out + r * 6;
            o[0] = base; o[1] = l0; o[2] = base + l0; o[3] = l1; o[4] = base + l0 + l1; o[5] = l2;
        }
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void tp_token_copy(const uint8_t *text, const int64_t *meta, const int64_t *idx, int64_t nrows,
                                                     const int64_t *meta_out, uint8_t *bytes, int64_t cap)
{
    CV_GRID_STRIDE(r, nrows) {
        const int64_t *m = meta + idx[r] * 6, *o = meta_out + r * 6;
        for (int t = 0; t < 3; t++) {
            const int64_t from = m[2 * t], to = o[2 * t], n = o[2 * t + 1];
            if (to + n > cap) return;                        // (the caller sized the buffer from these very lengths)
            for (int64_t k = 0; k < n; k++) bytes[to + k] = text[from + k];
        }
    }
}

// cv_text_find_newline_dev: for up to CV_TEXT_FIND_MAX offsets, the first '\n' at or behind each.  The waves walk the
// text front to back in grid-sized steps of 16-byte granules; lane i of every wave watches query i: the query is OPEN for
// the wave while its current answer lies behind the wave's first byte, and it is IN REACH when its offset lies in front
// of the wave's last byte.  A wave without an open query leaves; one whose open queries are all out of reach steps on
// without loading; the others load their granule and lower the answers of the queries a newline of theirs serves.
struct find_queries {
    int64_t from[CV_TEXT_FIND_MAX];
};

__global__ void tp_find_begin(int64_t *out, int k, int64_t len)
{
    if ((int)threadIdx.x < k) out[threadIdx.x] = len;
}

__global__ __launch_bounds__(TILE_THREADS) void tp_find_newline(const uint4 *gran, int shift, int64_t len, const find_queries q,
                                                                 int k, int64_t *out)
{
    const int64_t lo = shift, hi = shift + len;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t mine = lane < k ? q.from[lane] : len;                    // (the offset of the query this lane watches)
    for (int64_t g0 = ((int64_t)blockIdx.x * TILE_THREADS + threadIdx.x) * 16; ; g0 += (int64_t)gridDim.x * TILE) {
        const int64_t w0 = g0 - (int64_t)lane * 16 - shift;                // the wave's first byte, relative to the text
        if (w0 >= len) break;                                              // (uniform over the wave)
        bool open = false, reach = false;
        if (lane < k) {
            open = __atomic_load_n(&out[lane], __ATOMIC_RELAXED) > w0;
            reach = open && mine < w0 + WAVE * 16;
        }
        if (!__any(open)) break;
        if (!__any(reach) || g0 >= hi) continue;
        const uint32_t m = newline_mask(gran[g0 >> 4], g0, lo, hi);
        if (!m) continue;
        const int64_t p0 = g0 - shift;                                     // the granule's first byte, relative to the text
        for (int i = 0; i < k; i++) {
            const int64_t d = q.from[i] - p0;
            const uint32_t mm = d <= 0 ? m : (d >= 16 ? 0u : m & (0xffffu << d));
            if (mm) atomicMin((unsigned long long *)&out[i], (unsigned long long)(p0 + __ffs(mm) - 1));
        }
    }
}

struct index_ws {
    int64_t ntiles_max;         // tiles of a slab of `len` bytes at the worst offset inside its first granule
    uint32_t *tile_cnt, *tile_first;
    int64_t *line_end;
    void *scan_tmp;
    size_t scan_bytes;
};

int index_plan(cv_carver &c, int64_t len, int64_t max_lines, index_ws *W)
{
    W->ntiles_max = (len + 15 + TILE - 1) / TILE;
    W->tile_cnt = c.take<uint32_t>((size_t)(W->ntiles_max + 1));
    W->tile_first = c.take<uint32_t>((size_t)(W->ntiles_max + 1));
    W->line_end = c.take<int64_t>((size_t)(max_lines > 0 ? max_lines : 1));
    if (cv_scan_temp_bytes<uint32_t>(W->ntiles_max + 1, &W->scan_bytes)) return 1;
    W->scan_tmp = c.take_bytes(W->scan_bytes);
    return 0;
}

// cv_text_run_flags: one thread per line
__global__ __launch_bounds__(256) void tp_run_flags(const uint8_t *text, const int64_t *span, const int32_t *isrow, int64_t max_lines,
                                                    int32_t *flag)
{
    CV_GRID_STRIDE(i, max_lines + 1) {
        int f = 0;
        if (i < max_lines && isrow[i]) {
            f = i == 0 || !isrow[i - 1] || span[2 * i + 1] != span[2 * i - 1];
            const uint8_t *a = text + span[2 * i], *b = f ? a : text + span[2 * i - 2];
            for (int64_t k = 0; !f && k < span[2 * i + 1]; ++k) f = a[k] != b[k];
        }
        flag[i] = f;
    }
}

}  // namespace

// The newline index of a slab, for every reader of text in HBM (declared in cv_internal.hpp): workspace_dev (256-byte
// aligned, cv_text_line_index_bytes) receives line_end[i] = offset of the newline that closes line i < max_lines, info_dev
// {bytes consumed, lines, 0, 0}.  Enqueued on st; allocates nothing.
int cv_text_line_index_bytes(int64_t len, int64_t max_lines, size_t *bytes)
{
    cv_carver c;
    index_ws W;
    if (index_plan(c, len, max_lines, &W)) return 1;
    *bytes = c.total();
    return 0;
}

int cv_text_line_index(const char *text_dev, int64_t len, int64_t max_lines, void *workspace_dev, int64_t *info_dev,
                       const int64_t **line_end_dev, hipStream_t st)
{
    cv_carver c(workspace_dev);
    index_ws W;
    if (index_plan(c, len, max_lines, &W)) return 1;
    uint32_t *tile_cnt = W.tile_cnt, *tile_first = W.tile_first;
    int64_t *line_end = W.line_end;
    const int shift = (int)((uintptr_t)text_dev & 15);
    const uint4 *gran = (const uint4 *)(text_dev - shift);
    // (the tile count of the worst offset: what the workspace and the scan were sized for; a tile behind the slab counts 0)
    const int64_t ntiles = len > 0 && max_lines > 0 ? W.ntiles_max : 0;
    if (ntiles > 0) {
        const int grid = (int)(ntiles < INDEX_GRID ? ntiles : INDEX_GRID);
        hipLaunchKernelGGL(tp_count_newlines, dim3(grid), dim3(TILE_THREADS), 0, st, gran, shift, len, ntiles, tile_cnt);
        size_t need = W.scan_bytes;
        CV_HIP(hipcub::DeviceScan::ExclusiveSum(W.scan_tmp, need, (const uint32_t *)tile_cnt, tile_first, (int)(ntiles + 1), st));
        hipLaunchKernelGGL(tp_line_ends, dim3(grid), dim3(TILE_THREADS), 0, st, gran, shift, len, ntiles,
                           (const uint32_t *)tile_first, max_lines, line_end);
    }
    hipLaunchKernelGGL(tp_begin, dim3(1), dim3(64), 0, st, (const uint32_t *)tile_first, ntiles, max_lines,
                       (const int64_t *)line_end, info_dev);
    CV_HIP(hipGetLastError());
    *line_end_dev = line_end;
    return 0;
}

void cv_text_run_flags(const uint8_t *text_dev, const int64_t *span_dev, const int32_t *isrow_dev, int64_t max_lines, int32_t *flag_dev,
                       hipStream_t st)
{
    hipLaunchKernelGGL(tp_run_flags, dim3(cv_grid_for(max_lines + 1)), dim3(256), 0, st, text_dev, span_dev, isrow_dev, max_lines, flag_dev);
}

extern "C" int cv_parse_tensor_text_dev_workspace(int64_t len, int64_t max_lines, int64_t *bytes)
{
    if (!bytes) { cv_set_error("cv_parse_tensor_text_dev_workspace: null argument"); return 1; }
    if (len < 0 || max_lines < 0 || len > CV_TEXT_SLAB_MAX) {
        cv_set_error("cv_parse_tensor_text_dev_workspace: len %lld / max_lines %lld out of range (0 .. %lld bytes)",
                     (long long)len, (long long)max_lines, (long long)CV_TEXT_SLAB_MAX);
        return 1;
    }
    size_t need = 0;
    if (cv_text_line_index_bytes(len, max_lines, &need)) return 1;
    *bytes = (int64_t)need;
    return 0;
}

extern "C" int cv_parse_tensor_text_dev(const char *text_dev, int64_t len, int64_t max_lines, float *x_dev,
                                        int64_t *meta_dev, uint8_t *status_dev, int64_t *info_dev, void *workspace_dev,
                                        int64_t workspace_bytes, void *stream)
{
    if (!text_dev || !x_dev || !meta_dev || !status_dev || !info_dev || !workspace_dev) {
        cv_set_error("cv_parse_tensor_text_dev: null argument");
        return 1;
    }
    if (len < 0 || max_lines < 0 || len > CV_TEXT_SLAB_MAX) {
        cv_set_error("cv_parse_tensor_text_dev: len %lld / max_lines %lld out of range (0 .. %lld bytes)", (long long)len,
                     (long long)max_lines, (long long)CV_TEXT_SLAB_MAX);
        return 1;
    }
    if (((uintptr_t)x_dev & 15) || ((uintptr_t)meta_dev & 7) || ((uintptr_t)info_dev & 7)) {
        cv_set_error("cv_parse_tensor_text_dev: x_dev must be 16-byte, meta_dev / info_dev 8-byte aligned");
        return 1;
    }
    size_t need = 0;
    if (cv_text_line_index_bytes(len, max_lines, &need)) return 1;
    if (!cv_workspace_ok("cv_parse_tensor_text_dev", workspace_dev, workspace_bytes, need)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int64_t *line_end = nullptr;
    if (cv_text_line_index(text_dev, len, max_lines, workspace_dev, info_dev, &line_end, st)) return 1;
    const int shift = (int)((uintptr_t)text_dev & 15);
    const uint4 *gran = (const uint4 *)(text_dev - shift);
    if (len > 0 && max_lines > 0) {
        const int64_t blocks = (max_lines + PARSE_WAVES - 1) / PARSE_WAVES;
        hipLaunchKernelGGL(tp_parse_rows, dim3((int)(blocks < PARSE_GRID ? blocks : PARSE_GRID)), dim3(PARSE_WAVES * WAVE), 0, st,
                           gran, shift, line_end, info_dev, x_dev, meta_dev, status_dev);
    }
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_text_gather_rows(const float *x_dev, const int64_t *index_dev, int64_t nrows, float *out_dev, void *stream)
{
    if (nrows < 0) { cv_set_error("cv_text_gather_rows: negative row count"); return 1; }
    if (nrows == 0) return 0;
    if (!x_dev || !index_dev || !out_dev) { cv_set_error("cv_text_gather_rows: null argument"); return 1; }
    if (((uintptr_t)x_dev & 15) || ((uintptr_t)out_dev & 15) || ((uintptr_t)index_dev & 7)) {
        cv_set_error("cv_text_gather_rows: the tensors must be 16-byte, the index list 8-byte aligned");
        return 1;
    }
    const int64_t blocks = (nrows * (NV / 4) + 255) / 256;
    hipLaunchKernelGGL(tp_gather_rows, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const float4 *)x_dev, index_dev, nrows, (float4 *)out_dev);
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_text_find_newline_dev(const char *text_dev, int64_t len, const int64_t *from, int k, int64_t *out_dev, void *stream)
{
    if (k < 0 || k > CV_TEXT_FIND_MAX || len < 0) {
        cv_set_error("cv_text_find_newline_dev: %d queries / len %lld out of range (0 .. %d queries)", k, (long long)len, CV_TEXT_FIND_MAX);
        return 1;
    }
    if (k == 0) return 0;
    if (!from || !out_dev || (!text_dev && len > 0)) { cv_set_error("cv_text_find_newline_dev: null argument"); return 1; }
    if ((uintptr_t)out_dev & 7) { cv_set_error("cv_text_find_newline_dev: out_dev must be 8-byte aligned"); return 1; }
    hipStream_t st = (hipStream_t)stream;
    find_queries q;
    int64_t first = len;
    for (int i = 0; i < CV_TEXT_FIND_MAX; i++) {
        q.from[i] = i < k ? (from[i] < 0 ? 0 : from[i]) : len;
        if (q.from[i] < first) first = q.from[i];
    }
    hipLaunchKernelGGL(tp_find_begin, dim3(1), dim3(CV_TEXT_FIND_MAX), 0, st, out_dev, k, len);
    if (first < len) {
        const int shift = (int)((uintptr_t)text_dev & 15);
        const int64_t ntiles = (shift + len + TILE - 1) / TILE;
        hipLaunchKernelGGL(tp_find_newline, dim3((int)(ntiles < FIND_GRID ? ntiles : FIND_GRID)), dim3(TILE_THREADS), 0, st,
                           (const uint4 *)(text_dev - shift), shift, len, q, k, out_dev);
    }
    CV_HIP(hipGetLastError());
    return 0;
}

extern "C" int cv_text_gather_tokens(const char *text_dev, const int64_t *meta_dev, const int64_t *index_dev, int64_t nrows,
                                     uint8_t *bytes_dev, int64_t bytes_cap, int64_t *meta_out_dev, void *stream)
{
    if (nrows < 0 || bytes_cap < 0) { cv_set_error("cv_text_gather_tokens: negative row count or capacity"); return 1; }
    if (nrows == 0) return 0;
    if (!text_dev || !meta_dev || !index_dev || !bytes_dev || !meta_out_dev) { cv_set_error("cv_text_gather_tokens: null argument"); return 1; }
    if (((uintptr_t)meta_dev & 7) || ((uintptr_t)index_dev & 7) || ((uintptr_t)meta_out_dev & 7)) {
        cv_set_error("cv_text_gather_tokens: meta and the index list must be 8-byte aligned");
        return 1;
    }
    hipLaunchKernelGGL(tp_token_offsets, dim3(1), dim3(TOKEN_THREADS), 0, (hipStream_t)stream, meta_dev, index_dev, nrows, meta_out_dev);
    const int64_t blocks = (nrows + 255) / 256;
    hipLaunchKernelGGL(tp_token_copy, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t *)text_dev, meta_dev, index_dev, nrows, (const int64_t *)meta_out_dev, bytes_dev, bytes_cap);
    CV_HIP(hipGetLastError());
    return 0;
}
