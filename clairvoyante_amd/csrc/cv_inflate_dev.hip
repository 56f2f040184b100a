// cv_inflate_dev.hip -- BGZF members inflated on the device: compressed bytes in HBM -> the slab of text that
// cv_parse_tensor_text_dev takes.  A BGZF file (bgzip / htslib) is a series of independent gzip members of at most
// 64 KiB each way whose headers state the compressed size, so thousands of members are decoded at once.
//
//   bgzf_inflate   one wave per member, INFLATE_WAVES waves per workgroup.  The decode core is cv_inflate_core.hpp (the
//                  same text the host tests run under sanitizers): lane 0 decodes symbols into a queue of copy commands
//                  in LDS, the wave runs the queue 64 bytes per step, every lane then takes the CRC-32 of one 1 KiB
//                  chunk and lane 0 folds the chunk states.  status = OK only for a valid stream of exactly ISIZE bytes
//                  with the trailer's CRC-32; everything else is HOST and the caller decodes that member itself.
//
// Output goes straight to HBM and back-references are read from there, so the lanes of a wave talk through global
// memory.  What keeps program order across lanes: every command and every table pass is followed by wave_sync() -- a
// wavefront-scope release fence, a wave barrier, a wavefront-scope acquire fence.  The vector memory operations of one
// wave are performed in order by the hardware, so at this scope the fences cost no instruction; what they do is forbid
// the compiler to move a later command's loads above an earlier command's stores.  An LDS window was the alternative:
// 64 KiB per wave would leave two waves per CU, against the 30 KB per workgroup of four waves used here.
//
// LDS per wave: 10-bit literal/length table 2 KiB, 8-bit distance table 0.5 KiB, canonical bookkeeping 1.1 KiB, command
// queue and literal bytes 1.3 KiB, input window 2 KiB (sizeof(cvi::state)); longer codes walk the canonical code
// instead of second-level tables.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_inflate_core.hpp"

void cv_set_error(const char *fmt, ...);

namespace {

constexpr int INFLATE_WAVES = 4;
constexpr int INFLATE_GRID = 4096;

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(INFLATE_WAVES * cvi::LANES) void bgzf_inflate(const uint8_t *comp, const int64_t *table, int64_t members,
                                                                           uint8_t *text, int64_t text_cap, uint8_t *status,
                                                                           const cvi::crc_consts C)
{
    __shared__ cvi::state states[INFLATE_WAVES];
    __shared__ uint32_t byte_table[256];
    __shared__ uint32_t part[INFLATE_WAVES][cvi::LANES];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) byte_table[i] = cvi::crc_byte_table((uint32_t)i);
    __syncthreads();
    const int wave = threadIdx.x / cvi::LANES, lane = threadIdx.x % cvi::LANES;
    cvi::state &S = states[wave];
    const int64_t data0 = table[0], out0 = table[2];
    for (int64_t m = (int64_t)blockIdx.x * INFLATE_WAVES + wave; m < members; m += (int64_t)gridDim.x * INFLATE_WAVES) {
        const int64_t off = table[4 * m] - data0, clen = table[4 * m + 1], oat = table[4 * m + 2] - out0;
        const uint32_t isize = (uint32_t)((uint64_t)table[4 * m + 3] >> 32), want_crc = (uint32_t)table[4 * m + 3];
        // a row that does not describe a member inside the buffers is not touched
        if (off < 0 || clen < 0 || clen > (int64_t)cvi::MEMBER_MAX || isize > cvi::MEMBER_MAX || oat < 0 || oat + (int64_t)isize > text_cap) {
            if (lane == 0) status[m] = CV_BGZF_HOST;
            continue;
        }
        const uint8_t *data = comp + off;
        uint8_t *out = text + oat;
        if (lane == 0) cvi::begin(S);
        wave_sync();
        int what;
        do {
            if (cvi::short_of_input(S, (uint32_t)clen, cvi::HEADER_NEED)) {      // (the same answer in every lane)
                cvi::window(S, data, (uint32_t)clen, lane, cvi::LANES);
                wave_sync();
                if (lane == 0) cvi::window_loaded(S, (uint32_t)clen);
                wave_sync();
            }
            if (lane == 0) cvi::step(S, (uint32_t)clen, isize);
            wave_sync();
            what = __builtin_amdgcn_readfirstlane(S.what);
            if (what == cvi::W_BAD) break;
            const int nq = __builtin_amdgcn_readfirstlane(S.nq);
            for (int q = 0; q < nq; q++) {
                cvi::run(S, q, data, out, lane, cvi::LANES);
                wave_sync();
            }
            if (what == cvi::W_FILL) {
                cvi::fill(S, 0, lane, cvi::LANES);
                wave_sync();
                cvi::fill(S, 1, lane, cvi::LANES);
                wave_sync();
            }
        } while (what != cvi::W_DONE);
        bool ok = what == cvi::W_DONE;
        if (ok) {
            part[wave][lane] = cvi::crc_chunk(out, isize, lane, byte_table);
            wave_sync();
            if (lane == 0) ok = cvi::crc_fold(part[wave], isize, C) == want_crc;
        }
        if (lane == 0) status[m] = ok ? CV_BGZF_OK : CV_BGZF_HOST;
        wave_sync();
    }
}

inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const uint8_t *p) { return rd16(p) | (rd16(p + 2) << 16); }

}  // namespace

extern "C" int cv_bgzf_scan(const uint8_t *src, int64_t n, int64_t max_members, int64_t *table, int64_t *members,
                            int64_t *inflated_bytes)
{
    if (!src || n < 0 || max_members < 0 || (max_members > 0 && !table) || !members || !inflated_bytes) {
        cv_set_error("cv_bgzf_scan: null or negative argument");
        return -1;
    }
    int64_t p = 0, m = 0, out = 0;
    while (p < n) {
        if (src[p] == 0) {                                   // zero padding behind the last member
            for (int64_t q = p; q < n; q++)
                if (src[q]) return 1;
            break;
        }
        // (the header logic of bgzf_block_size in cv_bam.cpp, on a whole file: what is short here is truncated)
        if (n - p < 18 || src[p] != 0x1f || src[p + 1] != 0x8b || src[p + 2] != 8 || src[p + 3] != 4) return 1;
        const int64_t xlen = rd16(src + p + 10);
        if (n - p < 12 + xlen + 8) return 1;
        int64_t at = 12, bsize = -1;
        while (at + 4 <= 12 + xlen) {
            const int64_t slen = rd16(src + p + at + 2);
            if (src[p + at] == 'B' && src[p + at + 1] == 'C' && slen == 2) {
                if (at + 6 > 12 + xlen) return 1;
                bsize = (int64_t)rd16(src + p + at + 4) + 1;
            }
            at += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || bsize > n - p) return 1;
        const uint32_t crc = rd32(src + p + bsize - 8), isize = rd32(src + p + bsize - 4);
        if (isize > 65536) return 1;
        if (m < max_members) {
            table[4 * m] = p + 12 + xlen;
            table[4 * m + 1] = bsize - 12 - xlen - 8;
            table[4 * m + 2] = out;
            table[4 * m + 3] = (int64_t)(((uint64_t)isize << 32) | crc);
        }
        m++; out += isize; p += bsize;
    }
    if (m == 0) return 1;
    *members = m;
    *inflated_bytes = out;
    return 0;
}

extern "C" int cv_inflate_bgzf_dev(const uint8_t *comp_dev, const int64_t *table_dev, int64_t members, uint8_t *text_dev,
                                   int64_t text_cap, uint8_t *status_dev, void *stream)
{
    if (members < 0 || text_cap < 0) { cv_set_error("cv_inflate_bgzf_dev: negative member count or capacity"); return 1; }
    if (members == 0) return 0;
    if (!comp_dev || !table_dev || !text_dev || !status_dev) { cv_set_error("cv_inflate_bgzf_dev: null argument"); return 1; }
    if ((uintptr_t)table_dev & 7) { cv_set_error("cv_inflate_bgzf_dev: the table must be 8-byte aligned"); return 1; }
    static const cvi::crc_consts C = [] { cvi::crc_consts c; cvi::make_crc_consts(&c); return c; }();
    const int64_t blocks = (members + INFLATE_WAVES - 1) / INFLATE_WAVES;
    hipLaunchKernelGGL(bgzf_inflate, dim3((int)(blocks < INFLATE_GRID ? blocks : INFLATE_GRID)), dim3(INFLATE_WAVES * cvi::LANES), 0,
                       (hipStream_t)stream, comp_dev, table_dev, members, text_dev, text_cap, status_dev, C);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cv_set_error("cv_inflate_bgzf_dev: launch failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
