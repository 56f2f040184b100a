// cv_gzip_dev.hip -- an ORDINARY gzip stream (one member, blocks of unknown position, a 32 KiB window that chains
// everything) inflated on the device in two passes, the scheme of pugz / rapidgzip:
//
//   gzip_find      one wave per guess (guesses evenly spaced through the compressed bytes): scans bit offsets forward,
//                  64 per step, every lane the full header test of cvg::header_at, first hit by ballot.
//   gzip_decode    one wave per chunk (a chunk = from one found start to the next), lanes cooperating as in
//                  bgzf_inflate: lane 0 decodes into a queue of copy commands, the wave runs the queue.  The window in
//                  front of a chunk is unknown, so the output is 16-bit symbols: a byte or a marker "byte j of the
//                  32 KiB in front of this chunk".  Run twice: WRITE = false counts (length, end bit, how it ended),
//                  the caller checks the chain (chunk k ends exactly where chunk k + 1 was found), places the chunks
//                  by an exclusive scan, and WRITE = true writes with cap = the counted length.
//   gzip_tails     ONE workgroup, chunk after chunk: the last 32 KiB of every chunk (all of a shorter one) resolved
//                  into the final text -- after it the 32 KiB in front of every chunk are final.
//   gzip_rest      all other symbols, in parallel.
//   gzip_crc       the CRC-32 state of every 1 KiB piece of the text (pieces aligned to the END, started from 0); the
//                  caller folds them.
//
// The lanes of a decoding wave talk through global memory and LDS with wave_sync() between steps, exactly as
// cv_inflate_dev.hip explains.  LDS per workgroup of four waves: 4 * sizeof(cvi::state) = 30 KB.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_gzip_core.hpp"

void cv_set_error(const char *fmt, ...);

namespace {

constexpr int WAVES = 4;
constexpr int GRID = 4096;
constexpr int TAIL_THREADS = 1024;

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(WAVES * cvi::LANES) void gzip_find(const uint8_t *comp, int64_t nbytes, int64_t first_bit, int64_t spacing_bits,
                                                                int64_t guesses, int64_t *found)
{
    const int wave = threadIdx.x / cvi::LANES, lane = threadIdx.x % cvi::LANES;
    const int64_t end_all = nbytes * 8;
    for (int64_t g = (int64_t)blockIdx.x * WAVES + wave; g < guesses; g += (int64_t)gridDim.x * WAVES) {
        int64_t lo = first_bit + g * spacing_bits + (g == 0 ? 1 : 0), hi = first_bit + (g + 1) * spacing_bits;
        if (hi > end_all) hi = end_all;
        int64_t hit = -1;
        for (; lo < hi && hit < 0; lo += cvi::LANES) {
            const int64_t bit = lo + lane;
            const bool ok = bit < hi && cvg::header_at(comp, (uint64_t)nbytes, (uint64_t)bit);
            const uint64_t mask = __ballot(ok);
            if (mask) hit = lo + (int64_t)__builtin_ctzll(mask);
        }
        if (lane == 0) found[g] = hit;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(WAVES * cvi::LANES) void gzip_decode(const uint8_t *comp, int64_t nbytes, const int64_t *table, int64_t chunks,
                                                                  uint16_t *sym, int64_t sym_cap, int64_t *result)
{
    __shared__ cvi::state states[WAVES];
    __shared__ int32_t hows[WAVES];
    const int wave = threadIdx.x / cvi::LANES, lane = threadIdx.x % cvi::LANES;
    cvi::state &S = states[wave];
    for (int64_t c = (int64_t)blockIdx.x * WAVES + wave; c < chunks; c += (int64_t)gridDim.x * WAVES) {
        const int64_t start = table[6 * c], end = table[6 * c + 1], off = table[6 * c + 2], cap64 = table[6 * c + 3], hist = table[6 * c + 4];
        int64_t *res = result + 4 * c;
        // a row that does not describe a chunk inside the buffers is not touched
        bool sane = start >= 0 && start < nbytes * 8 && hist >= 0 && (end < 0 || end >= start);
        if (WRITE) sane = sane && off >= 0 && cap64 >= 0 && cap64 <= (int64_t)cvg::OUT_MAX && off + cap64 <= sym_cap;
        if (!sane) {
            if (lane == 0) { res[0] = 0; res[1] = start; res[2] = cvg::BAD; res[3] = 0; }
            continue;
        }
        const int64_t base = start >> 3;
        const uint8_t *data = comp + base;
        const uint32_t len = (uint32_t)(nbytes - base);
        const int64_t rel_end = end < 0 ? -1 : end - base * 8;
        const uint32_t cap = WRITE ? (uint32_t)cap64 : cvg::OUT_MAX;
        const uint32_t h = hist > (int64_t)cvg::WSIZE ? cvg::WSIZE : (uint32_t)hist;
        uint16_t *out = WRITE ? sym + off : nullptr;
        if (lane == 0) { cvg::chunk_begin(S); hows[wave] = cvg::BAD; }
        wave_sync();
        cvi::window(S, data, len, lane, cvi::LANES);
        wave_sync();
        if (lane == 0) {
            cvi::window_loaded(S, len);
            if (!cvg::chunk_skip(S, (int)(start & 7))) S.what = cvi::W_BAD;
        }
        wave_sync();
        int what = __builtin_amdgcn_readfirstlane(S.what);
        while (what != cvi::W_BAD && what != cvi::W_DONE) {
            if (cvi::short_of_input(S, len, cvi::HEADER_NEED)) {                 // (the same answer in every lane)
                cvi::window(S, data, len, lane, cvi::LANES);
                wave_sync();
                if (lane == 0) cvi::window_loaded(S, len);
                wave_sync();
            }
            if (lane == 0) cvg::chunk_step(S, len, rel_end, cap, h, &hows[wave]);
            wave_sync();
            what = __builtin_amdgcn_readfirstlane(S.what);
            if (what == cvi::W_BAD) break;
            if (WRITE) {
                const int nq = __builtin_amdgcn_readfirstlane(S.nq);
                for (int q = 0; q < nq; q++) {
                    cvg::chunk_run(S, q, data, out, lane, cvi::LANES);
                    wave_sync();
                }
            }
            if (what == cvi::W_FILL) {
                cvi::fill(S, 0, lane, cvi::LANES);
                wave_sync();
                cvi::fill(S, 1, lane, cvi::LANES);
                wave_sync();
            }
        }
        if (lane == 0) {
            res[0] = (int64_t)S.out;
            res[1] = base * 8 + cvg::bit_at(S);
            res[2] = what == cvi::W_DONE ? hows[wave] : cvg::BAD;
            res[3] = 0;
        }
        wave_sync();
    }
}

// off[0 .. chunks]: where each chunk's symbols / text start; text[-hist, 0) = what exists in front of the first chunk
__global__ __launch_bounds__(TAIL_THREADS) void gzip_tails(const uint16_t *sym, const int64_t *off, int64_t chunks, int64_t hist, uint8_t *text,
                                                           int32_t *bad)
{
    int32_t mine = 0;
    for (int64_t c = 0; c < chunks; c++) {
        const int64_t lo = off[c], hi = off[c + 1];
        const int64_t from = hi - lo > (int64_t)cvg::WSIZE ? hi - (int64_t)cvg::WSIZE : lo;
        for (int64_t i = from + threadIdx.x; i < hi; i += TAIL_THREADS) text[i] = cvg::resolve(sym[i], text + lo, hist + lo, &mine);
        __syncthreads();                                                     // (the next chunk reads these bytes)
    }
    if (mine) atomicOr(bad, 1);
}

__global__ __launch_bounds__(256) void gzip_rest(const uint16_t *sym, const int64_t *off, int64_t chunks, int64_t hist, uint8_t *text, int32_t *bad)
{
    const int64_t total = off[chunks];
    int32_t mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t a = 0, b = chunks;                                           // the chunk of symbol i: off[a] <= i < off[a + 1]
        while (b - a > 1) {
            const int64_t m = (a + b) >> 1;
            if (off[m] <= i) a = m; else b = m;
        }
        const int64_t lo = off[a], hi = off[a + 1];
        const int64_t from = hi - lo > (int64_t)cvg::WSIZE ? hi - (int64_t)cvg::WSIZE : lo;
        if (i >= from) continue;                                             // (gzip_tails wrote it; others read it now)
        text[i] = cvg::resolve(sym[i], text + lo, hist + lo, &mine);
    }
    if (mine) atomicOr(bad, 1);
}

__global__ __launch_bounds__(256) void gzip_crc(const uint8_t *text, int64_t n, int64_t pieces, uint32_t *part)
{
    __shared__ uint32_t byte_table[256];
    byte_table[threadIdx.x] = cvi::crc_byte_table((uint32_t)threadIdx.x);
    __syncthreads();
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pieces; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t hi = n - (pieces - 1 - p) * cvi::CRC_CHUNK, lo = hi > cvi::CRC_CHUNK ? hi - cvi::CRC_CHUNK : 0;
        uint32_t s = 0;
        for (int64_t i = lo; i < hi; i++) s = byte_table[(s ^ text[i]) & 0xff] ^ (s >> 8);
        part[p] = s;
    }
}

int launched(const char *who)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cv_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return 1; }
    return 0;
}

inline int grid_for(int64_t items, int per_block)
{
    const int64_t blocks = (items + per_block - 1) / per_block;
    return (int)(blocks < 1 ? 1 : blocks < GRID ? blocks : GRID);
}

}  // namespace

extern "C" int cv_gzip_header_at(const uint8_t *src, int64_t n, int64_t bit)
{
    if (!src || n < 0 || bit < 0) return 0;
    return cvg::header_at(src, (uint64_t)n, (uint64_t)bit) ? 1 : 0;
}

extern "C" int cv_gzip_chunk_host(const uint8_t *src, int64_t n, int64_t start_bit, int64_t end_bit, uint16_t *sym, int64_t cap,
                                  int64_t hist, int64_t *symbols, int64_t *ended)
{
    if (!src || n < 0 || cap < 0 || hist < 0 || !symbols || !ended) return cvg::BAD;
    uint32_t got = 0;
    const int how = cvg::chunk_host(src, (uint64_t)n, start_bit, end_bit, sym, (uint32_t)(cap > (int64_t)cvg::OUT_MAX ? cvg::OUT_MAX : cap),
                                    (uint32_t)(hist > (int64_t)cvg::WSIZE ? cvg::WSIZE : hist), &got, ended);
    *symbols = got;
    return how;
}

extern "C" int cv_gzip_find_dev(const uint8_t *comp_dev, int64_t nbytes, int64_t first_bit, int64_t spacing_bytes, int64_t guesses,
                                int64_t *found_dev, void *stream)
{
    if (nbytes < 0 || nbytes > 0x7fffffff || first_bit < 0 || spacing_bytes < 1 || guesses < 0) {
        cv_set_error("cv_gzip_find_dev: bad size, offset or spacing");
        return 1;
    }
    if (guesses == 0) return 0;
    if (!comp_dev || !found_dev) { cv_set_error("cv_gzip_find_dev: null argument"); return 1; }
    hipLaunchKernelGGL(gzip_find, dim3(grid_for(guesses, WAVES)), dim3(WAVES * cvi::LANES), 0, (hipStream_t)stream, comp_dev, nbytes,
                       first_bit, spacing_bytes * 8, guesses, found_dev);
    return launched("cv_gzip_find_dev");
}

extern "C" int cv_gzip_decode_dev(const uint8_t *comp_dev, int64_t nbytes, const int64_t *table_dev, int64_t chunks, uint16_t *sym_dev,
                                  int64_t sym_cap, int64_t *result_dev, void *stream)
{
    if (nbytes < 0 || nbytes > 0x7fffffff || chunks < 0 || sym_cap < 0) { cv_set_error("cv_gzip_decode_dev: bad size or count"); return 1; }
    if (chunks == 0) return 0;
    if (!comp_dev || !table_dev || !result_dev) { cv_set_error("cv_gzip_decode_dev: null argument"); return 1; }
    if (((uintptr_t)table_dev | (uintptr_t)result_dev) & 7) { cv_set_error("cv_gzip_decode_dev: tables must be 8-byte aligned"); return 1; }
    const dim3 grid(grid_for(chunks, WAVES)), block(WAVES * cvi::LANES);
    if (sym_dev)
        hipLaunchKernelGGL(gzip_decode<true>, grid, block, 0, (hipStream_t)stream, comp_dev, nbytes, table_dev, chunks, sym_dev, sym_cap, result_dev);
    else
        hipLaunchKernelGGL(gzip_decode<false>, grid, block, 0, (hipStream_t)stream, comp_dev, nbytes, table_dev, chunks, sym_dev, sym_cap, result_dev);
    return launched("cv_gzip_decode_dev");
}

extern "C" int cv_gzip_resolve_dev(const uint16_t *sym_dev, const int64_t *off_dev, int64_t chunks, int64_t total, int64_t hist,
                                   uint8_t *text_dev, int32_t *bad_dev, void *stream)
{
    if (chunks < 0 || total < 0 || hist < 0 || hist > (int64_t)cvg::WSIZE) { cv_set_error("cv_gzip_resolve_dev: bad count or window"); return 1; }
    if (chunks == 0 || total == 0) return 0;
    if (!sym_dev || !off_dev || !text_dev || !bad_dev) { cv_set_error("cv_gzip_resolve_dev: null argument"); return 1; }
    hipLaunchKernelGGL(gzip_tails, dim3(1), dim3(TAIL_THREADS), 0, (hipStream_t)stream, sym_dev, off_dev, chunks, hist, text_dev, bad_dev);
    if (launched("cv_gzip_resolve_dev")) return 1;
    hipLaunchKernelGGL(gzip_rest, dim3(grid_for(total, 256 * 8)), dim3(256), 0, (hipStream_t)stream, sym_dev, off_dev, chunks, hist, text_dev, bad_dev);
    return launched("cv_gzip_resolve_dev");
}

extern "C" int cv_gzip_crc_dev(const uint8_t *text_dev, int64_t n, uint32_t *part_dev, void *stream)
{
    if (n < 0) { cv_set_error("cv_gzip_crc_dev: negative length"); return 1; }
    if (n == 0) return 0;
    if (!text_dev || !part_dev) { cv_set_error("cv_gzip_crc_dev: null argument"); return 1; }
    const int64_t pieces = (n + cvi::CRC_CHUNK - 1) / cvi::CRC_CHUNK;
    hipLaunchKernelGGL(gzip_crc, dim3(grid_for(pieces, 256)), dim3(256), 0, (hipStream_t)stream, text_dev, n, pieces, part_dev);
    return launched("cv_gzip_crc_dev");
}
