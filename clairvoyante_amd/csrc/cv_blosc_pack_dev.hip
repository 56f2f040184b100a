// cv_blosc_pack_dev.hip -- the X blocks of a `.bin` training set packed on the device: the rows of a resident set in HBM
// -> c-blosc 1.x chunks (the multi-block layout of cv_blosc_compress_lz4_blocks: byte shuffle, blocks split into byte
// planes, one LZ4 block per plane) in one slab.  What crosses to the host is the compressed form, not 2 112 bytes per
// candidate.  A chunk is pickle head | 500 rows | pickle tail; the envelope is the same for every chunk of a call.
//
//   pack_encode     one wave (one workgroup) per stream, over all chunks of the call.  The encode core is
//                   cv_lz4enc_core.hpp (the same text the host tests run under sanitizers): the hash table and the step's
//                   window lie in LDS, 17 KiB per wave, so nine waves share a CU's 160 KiB.  The stream's bytes are read
//                   where they lie (envelope and rows, shuffled on the fly); the LZ4 block goes to the stream's slot of
//                   the scratch; a stream that does not get smaller is recorded with its own length and stored raw later.
//   pack_layout     one workgroup per chunk: the running sum of 4 + length over the chunk's streams in c-blosc order
//                   (block by block, plane by plane) -> where each stream lies in its chunk, and the chunk's total.  A
//                   chunk that does not get smaller than 16 + nbytes is HOST and takes no room in the slab.
//   pack_offsets    one workgroup: the running sum of the totals over the chunks -> chunk_off[chunks + 1].
//   pack_assemble   one workgroup per stream: header and bstarts (by the first stream of the chunk / of each block), the
//                   length word, the stream's bytes from its slot or, stored, from the source.  Plain byte stores.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>
#include <string.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_lz4enc_core.hpp"

void cv_set_error(const char *fmt, ...);

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int COPY_THREADS = 256;
constexpr int64_t MAX_GRID = 1 << 20;
static_assert(cve::ST_OK == CV_BLOSC_OK && cve::ST_HOST == CV_BLOSC_HOST, "the status words of the header and of the core");

struct envelope {
    const uint8_t *head, *tail;
    uint32_t head_len, tail_len;
};

// the workspace: envelope | lens u32[streams] | at u32[streams] | totals i64[chunks] | slots
struct workspace {
    int64_t env_at, lens_at, at_at, totals_at, slots_at, bytes;
};

workspace lay_out(int64_t chunks, const cve::geometry &g)
{
    workspace w;
    const int64_t streams = chunks * (int64_t)g.streams;
    w.env_at = 0;
    w.lens_at = 2 * (int64_t)cve::ENVELOPE_MAX;
    w.at_at = w.lens_at + ((4 * streams + 15) & ~(int64_t)15);
    w.totals_at = w.at_at + ((4 * streams + 15) & ~(int64_t)15);
    w.slots_at = w.totals_at + ((8 * chunks + 15) & ~(int64_t)15);
    w.bytes = w.slots_at + streams * (int64_t)g.slot;
    return w;
}

__device__ __forceinline__ uint32_t source_of(const cve::geometry &g, const envelope &env, const uint8_t *data, int64_t data_bytes,
                                              int64_t m, cve::source &src, int64_t *chunk, uint32_t *block, bool *first)
{
    const int64_t c = m / g.streams;
    const uint32_t s = (uint32_t)(m - c * g.streams);
    src.head = env.head; src.tail = env.tail; src.head_len = env.head_len; src.tail_len = env.tail_len;
    src.data = data + c * data_bytes; src.data_len = (uint32_t)data_bytes;
    *chunk = c;
    return cve::stream_source(g, s, src, block, first);
}

__global__ __launch_bounds__(cve::LANES) void pack_encode(cve::geometry g, envelope env, const uint8_t *data, int64_t data_bytes,
                                                          int64_t streams, uint8_t *slots, uint32_t *lens)
{
    __shared__ cve::state S;
    const int lane = threadIdx.x;
    for (int64_t m = blockIdx.x; m < streams; m += gridDim.x) {
        cve::source src;
        int64_t c; uint32_t b; bool f;
        const uint32_t n = source_of(g, env, data, data_bytes, m, src, &c, &b, &f);
        // the slot holds g.slot >= n bytes; the core writes at most n - 1 of them
        uint32_t len = n <= g.slot ? cve::encode(S, src, n, slots + m * (int64_t)g.slot, n - 1, lane) : 0;
        if (len == 0) len = n;
        if (lane == 0) lens[m] = len;
        __syncthreads();
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void pack_layout(cve::geometry g, const uint32_t *lens, uint32_t *at, int64_t *totals, int32_t *status)
{
    typedef hipcub::BlockScan<uint32_t, SCAN_THREADS> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const int64_t c = blockIdx.x, m0 = c * (int64_t)g.streams;
    uint32_t running = 16 + 4 * g.nblocks;         // (a chunk that counts stays below 16 + nbytes < 2^31; a sum that wraps
    bool over = false;                              //  is caught here)
    for (uint32_t lo = 0; lo < g.streams; lo += SCAN_THREADS) {
        const uint32_t s = lo + threadIdx.x;
        const uint32_t v = s < g.streams ? 4 + lens[m0 + s] : 0;
        uint32_t excl, sum;
        Scan(tmp).ExclusiveSum(v, excl, sum);
        if (s < g.streams) at[m0 + s] = running + excl;
        if (sum > 0x7fffffffu - running) over = true;
        running += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool ok = !over && running < 16 + g.nbytes;
        status[c] = ok ? CV_BLOSC_OK : CV_BLOSC_HOST;
        totals[c] = ok ? (int64_t)running : 0;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void pack_offsets(const int64_t *totals, int64_t chunks, int64_t *chunk_off)
{
    typedef hipcub::BlockScan<int64_t, SCAN_THREADS> Scan;
    __shared__ typename Scan::TempStorage tmp;
    int64_t running = 0;
    for (int64_t lo = 0; lo < chunks; lo += SCAN_THREADS) {
        const int64_t c = lo + threadIdx.x;
        const int64_t v = c < chunks ? totals[c] : 0;
        int64_t excl, sum;
        Scan(tmp).ExclusiveSum(v, excl, sum);
        if (c < chunks) chunk_off[c] = running + excl;
        running += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) chunk_off[chunks] = running;
}

__global__ __launch_bounds__(COPY_THREADS) void pack_assemble(cve::geometry g, envelope env, const uint8_t *data, int64_t data_bytes,
                                                              int64_t streams, const uint8_t *slots, const uint32_t *lens, const uint32_t *at,
                                                              const int64_t *totals, const int64_t *chunk_off, const int32_t *status,
                                                              uint8_t *out, int64_t out_cap)
{
    for (int64_t m = blockIdx.x; m < streams; m += gridDim.x) {
        cve::source src;
        int64_t c; uint32_t b; bool f;
        const uint32_t n = source_of(g, env, data, data_bytes, m, src, &c, &b, &f);
        if (status[c] != CV_BLOSC_OK) continue;
        const int64_t total = totals[c], base = chunk_off[c];
        const uint32_t o = at[m], len = lens[m];
        // a stream that does not lie inside its chunk, or a chunk outside the slab, is not written
        if (base < 0 || total < 16 || base > out_cap - total || len > n || (int64_t)o + 4 + len > total) continue;
        uint8_t *dst = out + base;
        if (threadIdx.x == 0) {
            if (m == c * (int64_t)g.streams) cve::put_header(g, (uint32_t)total, dst);
            if (f) cve::put32(dst + 16 + 4 * b, o);
            cve::put32(dst + o, len);
        }
        uint8_t *body = dst + o + 4;
        if (len == n) {
            for (uint32_t k = threadIdx.x; k < n; k += COPY_THREADS) body[k] = cve::byte(src, k);
        } else {
            const uint8_t *slot = slots + m * (int64_t)g.slot;
            for (uint32_t k = threadIdx.x; k < len; k += COPY_THREADS) body[k] = slot[k];
        }
    }
}

bool geometry_for(int64_t chunk_nbytes, int typesize, int64_t blocksize, cve::geometry &g, const char *who)
{
    if (typesize != 4) { cv_set_error("%s: only typesize 4 is packed on the device", who); return false; }
    if (!cve::make_geometry(chunk_nbytes, typesize, blocksize, g)) {
        cv_set_error("%s: not a chunk for the device (fewer than 64 bytes, or a stream of more than %u bytes)", who, cve::STREAM_CAP);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int64_t cv_blosc_pack_stream_cap(void) { return (int64_t)cve::STREAM_CAP; }

extern "C" int cv_blosc_pack_workspace(int64_t chunks, int64_t chunk_nbytes, int typesize, int64_t blocksize, int64_t *scratch_bytes,
                                       int64_t *out_bound)
{
    if (chunks < 0 || chunks > 65535 || !scratch_bytes || !out_bound) { cv_set_error("cv_blosc_pack_workspace: bad argument"); return 1; }
    cve::geometry g;
    if (!geometry_for(chunk_nbytes, typesize, blocksize, g, "cv_blosc_pack_workspace")) return 1;
    *scratch_bytes = lay_out(chunks, g).bytes;
    *out_bound = chunks * (16 + chunk_nbytes);
    return 0;
}

extern "C" int cv_blosc_pack_dev(const uint8_t *data_dev, int64_t chunks, int64_t data_bytes_per_chunk, const uint8_t *head, int64_t head_len,
                                 const uint8_t *tail, int64_t tail_len, int typesize, int64_t blocksize, uint8_t *out_dev, int64_t out_cap,
                                 int64_t *chunk_off_dev, int32_t *status_dev, uint8_t *workspace_dev, int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_blosc_pack_dev";
    if (chunks < 0 || chunks > 65535 || data_bytes_per_chunk < 0 || head_len < 0 || tail_len < 0 || head_len > (int64_t)cve::ENVELOPE_MAX ||
        tail_len > (int64_t)cve::ENVELOPE_MAX || (head_len && !head) || (tail_len && !tail)) {
        cv_set_error("%s: bad count, size or envelope", who);
        return 1;
    }
    if (!chunk_off_dev || ((uintptr_t)chunk_off_dev & 7) || ((uintptr_t)workspace_dev & 15)) { cv_set_error("%s: null or misaligned table", who); return 1; }
    hipStream_t st = (hipStream_t)stream;
    if (chunks == 0) {
        if (hipMemsetAsync(chunk_off_dev, 0, 8, st) != hipSuccess) { cv_set_error("%s: memset failed", who); return 1; }
        return 0;
    }
    cve::geometry g;
    const int64_t nbytes = head_len + data_bytes_per_chunk + tail_len;
    if (!geometry_for(nbytes, typesize, blocksize, g, who)) return 1;
    const workspace w = lay_out(chunks, g);
    if (!data_dev || !out_dev || !status_dev || !workspace_dev || workspace_bytes < w.bytes || out_cap < chunks * (16 + nbytes)) {
        cv_set_error("%s: null argument, or a workspace / output smaller than cv_blosc_pack_workspace says", who);
        return 1;
    }
    uint8_t *ws = workspace_dev;
    envelope env;
    env.head = ws + w.env_at; env.tail = ws + w.env_at + cve::ENVELOPE_MAX; env.head_len = (uint32_t)head_len; env.tail_len = (uint32_t)tail_len;
    // (the envelope is pageable host memory: these two copies return once it has been staged)
    if ((head_len && hipMemcpyAsync(ws + w.env_at, head, (size_t)head_len, hipMemcpyHostToDevice, st) != hipSuccess) ||
        (tail_len && hipMemcpyAsync(ws + w.env_at + cve::ENVELOPE_MAX, tail, (size_t)tail_len, hipMemcpyHostToDevice, st) != hipSuccess)) {
        cv_set_error("%s: copying the envelope failed", who);
        return 1;
    }
    uint32_t *lens = (uint32_t *)(ws + w.lens_at), *at = (uint32_t *)(ws + w.at_at);
    int64_t *totals = (int64_t *)(ws + w.totals_at);
    uint8_t *slots = ws + w.slots_at;
    const int64_t streams = chunks * (int64_t)g.streams;
    const unsigned grid = (unsigned)(streams < MAX_GRID ? streams : MAX_GRID);
    hipLaunchKernelGGL(pack_encode, dim3(grid), dim3(cve::LANES), 0, st, g, env, data_dev, data_bytes_per_chunk, streams, slots, lens);
    hipLaunchKernelGGL(pack_layout, dim3((unsigned)chunks), dim3(SCAN_THREADS), 0, st, g, lens, at, totals, status_dev);
    hipLaunchKernelGGL(pack_offsets, dim3(1), dim3(SCAN_THREADS), 0, st, totals, chunks, chunk_off_dev);
    hipLaunchKernelGGL(pack_assemble, dim3(grid), dim3(COPY_THREADS), 0, st, g, env, data_dev, data_bytes_per_chunk, streams, slots, lens, at,
                       totals, chunk_off_dev, status_dev, out_dev, out_cap);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cv_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return 1; }
    return 0;
}

// One phase alone, for tools/gpu_bin_pack_probe.py: 0 encode, 1 layout and offsets, 2 assemble -- the same launches as
// cv_blosc_pack_dev, which must have run once on these buffers (the envelope lies in the workspace).
extern "C" int cv_blosc_pack_phase_dev(int phase, const uint8_t *data_dev, int64_t chunks, int64_t data_bytes_per_chunk, int64_t head_len,
                                       int64_t tail_len, int typesize, int64_t blocksize, uint8_t *out_dev, int64_t out_cap,
                                       int64_t *chunk_off_dev, int32_t *status_dev, uint8_t *workspace_dev, int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_blosc_pack_phase_dev";
    cve::geometry g;
    const int64_t nbytes = head_len + data_bytes_per_chunk + tail_len;
    if (chunks <= 0 || chunks > 65535 || head_len < 0 || tail_len < 0 || head_len > (int64_t)cve::ENVELOPE_MAX || tail_len > (int64_t)cve::ENVELOPE_MAX ||
        data_bytes_per_chunk < 0) {
        cv_set_error("%s: bad count or size", who);
        return 1;
    }
    if (!geometry_for(nbytes, typesize, blocksize, g, who)) return 1;
    const workspace w = lay_out(chunks, g);
    if (!data_dev || !out_dev || !status_dev || !chunk_off_dev || !workspace_dev || workspace_bytes < w.bytes || out_cap < chunks * (16 + nbytes) ||
        ((uintptr_t)chunk_off_dev & 7) || ((uintptr_t)workspace_dev & 15)) {
        cv_set_error("%s: null, misaligned or too small a buffer", who);
        return 1;
    }
    uint8_t *ws = workspace_dev;
    envelope env;
    env.head = ws + w.env_at; env.tail = ws + w.env_at + cve::ENVELOPE_MAX; env.head_len = (uint32_t)head_len; env.tail_len = (uint32_t)tail_len;
    uint32_t *lens = (uint32_t *)(ws + w.lens_at), *at = (uint32_t *)(ws + w.at_at);
    int64_t *totals = (int64_t *)(ws + w.totals_at);
    uint8_t *slots = ws + w.slots_at;
    const int64_t streams = chunks * (int64_t)g.streams;
    const unsigned grid = (unsigned)(streams < MAX_GRID ? streams : MAX_GRID);
    hipStream_t st = (hipStream_t)stream;
    if (phase == 0) {
        hipLaunchKernelGGL(pack_encode, dim3(grid), dim3(cve::LANES), 0, st, g, env, data_dev, data_bytes_per_chunk, streams, slots, lens);
    } else if (phase == 1) {
        hipLaunchKernelGGL(pack_layout, dim3((unsigned)chunks), dim3(SCAN_THREADS), 0, st, g, lens, at, totals, status_dev);
        hipLaunchKernelGGL(pack_offsets, dim3(1), dim3(SCAN_THREADS), 0, st, totals, chunks, chunk_off_dev);
    } else if (phase == 2) {
        hipLaunchKernelGGL(pack_assemble, dim3(grid), dim3(COPY_THREADS), 0, st, g, env, data_dev, data_bytes_per_chunk, streams, slots, lens, at,
                           totals, chunk_off_dev, status_dev, out_dev, out_cap);
    } else {
        cv_set_error("%s: phase must be 0, 1 or 2", who);
        return 1;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cv_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return 1; }
    return 0;
}

// The same chunks written by the host form of the core from host memory: byte for byte what cv_blosc_pack_dev writes
// (for the tests and the probe).  out: chunks back to back, chunk_off[chunks + 1], status[chunks].
extern "C" int cv_blosc_pack_host_form(const uint8_t *data, int64_t chunks, int64_t data_bytes_per_chunk, const uint8_t *head, int64_t head_len,
                                       const uint8_t *tail, int64_t tail_len, int typesize, int64_t blocksize, uint8_t *out, int64_t out_cap,
                                       int64_t *chunk_off, int32_t *status)
{
    const char *who = "cv_blosc_pack_host_form";
    if (chunks < 0 || data_bytes_per_chunk < 0 || head_len < 0 || tail_len < 0 || head_len > (int64_t)cve::ENVELOPE_MAX ||
        tail_len > (int64_t)cve::ENVELOPE_MAX || !chunk_off || (chunks && (!data || !out || !status)) || (head_len && !head) || (tail_len && !tail)) {
        cv_set_error("%s: bad argument", who);
        return 1;
    }
    chunk_off[0] = 0;
    if (chunks == 0) return 0;
    cve::geometry g;
    const int64_t nbytes = head_len + data_bytes_per_chunk + tail_len;
    if (!geometry_for(nbytes, typesize, blocksize, g, who)) return 1;
    if (out_cap < chunks * (16 + nbytes)) { cv_set_error("%s: output smaller than cv_blosc_pack_workspace says", who); return 1; }
    for (int64_t c = 0; c < chunks; c++) {
        const uint32_t total = cve::pack_chunk_host(g, head, (uint32_t)head_len, data + c * data_bytes_per_chunk, (uint32_t)data_bytes_per_chunk,
                                                    tail, (uint32_t)tail_len, out + chunk_off[c]);
        status[c] = total ? CV_BLOSC_OK : CV_BLOSC_HOST;
        chunk_off[c + 1] = chunk_off[c] + total;
    }
    return 0;
}
