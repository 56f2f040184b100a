// cv_blosc_dev.hip -- the blocks of a `.bin` training set decoded on the device: c-blosc 1.x chunks (LZ4 / LZ4HC streams,
// byte shuffle) in HBM -> the ndarray data of every chunk, side by side, where the batch is wanted.  What crosses to the
// device is the compressed file (a fourteenth of the candidates for X), not 2 112 bytes per candidate.
//
//   cv_blosc_plan     host: walks the chunk headers, bstarts and per-split length words with the checks of
//                     cv_blosc_decompress and writes one row per LZ4 stream and one per chunk.  A chunk the host decoder
//                     would refuse, or one that is not byte-shuffled LZ4, is marked "not for the device".
//   blosc_decode      one wave per stream row, DECODE_WAVES waves per workgroup.  The decode core is cv_lz4_core.hpp (the
//                     same text the host tests run under sanitizers): lane 0 walks sequences into a queue of copy
//                     commands in LDS, the wave runs the queue 64 bytes per step.  The stream goes to a byte-plane scratch
//                     in HBM, not to its strided final place: a match must read the plane back.  A stored split and a
//                     memcpy'd chunk are plain copies.
//   blosc_unpack      per chunk: unshuffles the first 1 KiB into LDS, finds the pickled ndarray's data there
//                     (cvl::find_array_payload: a short last block has another header length than a full one, and the
//                     offset is in general no multiple of the item size), then gathers the payload from the planes
//                     -- four bytes per thread, each plane read coalesced -- into dst + i * block_bytes.
//
// Lanes of a wave talk through global memory as in cv_inflate_dev.hip: every command is followed by wave_sync() -- a
// wavefront-scope release fence, a wave barrier, a wavefront-scope acquire fence -- which keeps the compiler from
// moving a later command's loads above an earlier command's stores; the hardware performs the vector memory operations
// of one wave in order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_lz4_core.hpp"

void cv_set_error(const char *fmt, ...);

namespace {

constexpr int DECODE_WAVES = 4;
constexpr int DECODE_GRID = 8192;
constexpr int UNPACK_THREADS = 256;
constexpr int UNPACK_BYTES = UNPACK_THREADS * 4 * 16;     // payload bytes per workgroup: 16 words per thread
constexpr int SROW = CV_BLOSC_STREAM_ROW, CROW = CV_BLOSC_CHUNK_ROW;
static_assert(SROW == cvl::STREAM_ROW && CROW == cvl::CHUNK_ROW, "the rows of the header and of the core");

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(DECODE_WAVES * cvl::LANES) void blosc_decode(const uint8_t *comp, int64_t comp_bytes, const int64_t *rows,
                                                                         int64_t streams, uint8_t *scratch, int64_t scratch_bytes,
                                                                         uint8_t *status)
{
    __shared__ cvl::state states[DECODE_WAVES];
    const int wave = threadIdx.x / cvl::LANES, lane = threadIdx.x % cvl::LANES;
    cvl::state &S = states[wave];
    for (int64_t m = (int64_t)blockIdx.x * DECODE_WAVES + wave; m < streams; m += (int64_t)gridDim.x * DECODE_WAVES) {
        const int64_t off = rows[SROW * m], cb64 = rows[SROW * m + 1], oat = rows[SROW * m + 2], ne64 = rows[SROW * m + 3];
        const int64_t stored = rows[SROW * m + 4];
        // a row that does not describe a stream inside the buffers is not touched
        if (off < 0 || cb64 < 0 || cb64 > (int64_t)cvl::STREAM_MAX || off > comp_bytes - cb64 || oat < 0 || ne64 < 0 ||
            ne64 > (int64_t)cvl::STREAM_MAX || oat > scratch_bytes - ne64 || (stored && cb64 != ne64)) {
            if (lane == 0) status[m] = CV_BLOSC_HOST;
            continue;
        }
        const uint8_t *data = comp + off;
        uint8_t *out = scratch + oat;
        const uint32_t cb = (uint32_t)cb64, neblock = (uint32_t)ne64;
        if (stored) {
            for (uint32_t k = (uint32_t)lane; k < neblock; k += cvl::LANES) out[k] = data[k];
            if (lane == 0) status[m] = CV_BLOSC_OK;
            continue;
        }
        if (lane == 0) cvl::begin(S);
        wave_sync();
        int what;
        do {
            if (__builtin_amdgcn_readfirstlane(S.refill)) {
                cvl::window(S, data, cb, lane, cvl::LANES);
                wave_sync();
                if (lane == 0) cvl::window_loaded(S, cb);
                wave_sync();
            }
            if (lane == 0) cvl::step(S, cb, neblock);
            wave_sync();
            what = __builtin_amdgcn_readfirstlane(S.what);
            if (what == cvl::W_BAD) break;
            const int nq = __builtin_amdgcn_readfirstlane(S.nq);
            for (int q = 0; q < nq; q++) {
                cvl::run(S, q, data, out, lane, cvl::LANES);
                wave_sync();
            }
        } while (what != cvl::W_DONE);
        if (lane == 0) status[m] = what == cvl::W_DONE ? CV_BLOSC_OK : CV_BLOSC_HOST;
        wave_sync();
    }
}

__global__ __launch_bounds__(UNPACK_THREADS) void blosc_unpack(const int64_t *crow, int64_t chunks, const uint8_t *stream_status,
                                                              int64_t streams, const uint8_t *scratch, int64_t scratch_bytes,
                                                              uint8_t *dst, int64_t block_bytes, int64_t *lens, int32_t *status)
{
    __shared__ uint8_t head[1024];
    __shared__ int64_t pay[2];
    __shared__ int found;
    const int64_t c = blockIdx.y;
    const int64_t *row = crow + CROW * c;
    const int64_t ts64 = row[0], shuf = row[1], nb64 = row[2], bsz64 = row[3], s0 = row[4], ns = row[5], sat = row[6], refused = row[7];
    const bool first = blockIdx.x == 0;
    // a row that does not describe a chunk inside the buffers goes to the host
    bool bad = refused != 0 || nb64 < 0 || nb64 > (int64_t)cvl::STREAM_MAX || bsz64 <= 0 || bsz64 > (int64_t)cvl::STREAM_MAX ||
               (ts64 != 1 && ts64 != 4 && ts64 != 8) || sat < 0 || sat > scratch_bytes - nb64 || s0 < 0 || ns < 0 || s0 > streams - ns;
    if (bad) {
        if (first && threadIdx.x == 0) { status[c] = 1; lens[c] = 0; }
        return;
    }
    const uint32_t nbytes = (uint32_t)nb64, blocksize = (uint32_t)bsz64, ts = (uint32_t)ts64;
    const bool shuffled = shuf != 0 && ts > 1;
    const uint8_t *sc = scratch + sat;
    if (first) {                                                       // (one workgroup per chunk reports)
        int host = 0;
        for (int64_t s = threadIdx.x; s < ns; s += UNPACK_THREADS) host |= stream_status[s0 + s] != CV_BLOSC_OK;
        if (__syncthreads_or(host)) {
            if (threadIdx.x == 0) { status[c] = 1; lens[c] = 0; }
            return;
        }
    }
    const uint32_t hn = nbytes < 1024u ? nbytes : 1024u;
    for (uint32_t r = threadIdx.x; r < hn; r += UNPACK_THREADS) head[r] = cvl::plane_byte(sc, r, nbytes, blocksize, ts, shuffled);
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t off = 0, L = 0;
        found = cvl::find_array_payload(head, (int64_t)nbytes, &off, &L) ? 1 : 0;
        pay[0] = off; pay[1] = L;
    }
    __syncthreads();
    const int64_t off = pay[0], L = pay[1];
    if (!found) {
        // an empty trailing block pickles an array without a data object worth finding: a tiny stream is accepted
        if (first && threadIdx.x == 0) { status[c] = (c == chunks - 1 && nbytes < 512u) ? 0 : 2; lens[c] = 0; }
        return;
    }
    if ((c < chunks - 1 && L != block_bytes) || L > block_bytes) {
        if (first && threadIdx.x == 0) { status[c] = 2; lens[c] = 0; }
        return;
    }
    // find_array_payload vouches for off + L <= nbytes; L <= block_bytes keeps the chunk inside its own place
    uint8_t *out = dst + (size_t)c * (size_t)block_bytes;
    const int64_t lo = (int64_t)blockIdx.x * UNPACK_BYTES, hi = lo + UNPACK_BYTES < L ? lo + UNPACK_BYTES : L;
    const bool words = (((uintptr_t)out) & 3) == 0;
    for (int64_t p = lo + (int64_t)threadIdx.x * 4; p < hi; p += UNPACK_THREADS * 4) {
        const uint32_t r = (uint32_t)(off + p);
        if (words && p + 4 <= hi) {
            uint32_t v = 0;
            for (int k = 0; k < 4; k++) v |= (uint32_t)cvl::plane_byte(sc, r + k, nbytes, blocksize, ts, shuffled) << (8 * k);
            *(uint32_t *)(out + p) = v;
        } else {
            for (int k = 0; k < 4 && p + k < hi; k++) out[p + k] = cvl::plane_byte(sc, r + k, nbytes, blocksize, ts, shuffled);
        }
    }
    if (first && threadIdx.x == 0) { status[c] = 0; lens[c] = L; }
}

}  // namespace

extern "C" int cv_blosc_plan(const uint8_t *const *chunks, const int64_t *clens, int64_t n, int64_t max_nbytes, int64_t max_streams,
                             int64_t *stream_rows, int64_t *chunk_rows, int64_t *streams, int64_t *comp_bytes, int64_t *scratch_bytes)
{
    if (n < 0 || max_streams < 0 || max_nbytes < 0 || ((!chunks || !clens || !chunk_rows) && n > 0) || (!stream_rows && max_streams > 0) ||
        !streams || !comp_bytes || !scratch_bytes) {
        cv_set_error("cv_blosc_plan: null or negative argument");
        return -1;
    }
    int64_t ns = 0, comp = 0, scratch = 0;
    int refused = 0;
    for (int64_t i = 0; i < n; i++) {
        int64_t *crow = chunk_rows + CV_BLOSC_CHUNK_ROW * i;
        int64_t got = 0;
        if (clens[i] >= 0 && cvl::plan_chunk(chunks[i], clens[i], comp, scratch, max_nbytes, ns, max_streams, stream_rows, crow, &got)) {
            crow[8] = comp; crow[9] = clens[i];
            ns += got;
            comp += (clens[i] + 15) & ~(int64_t)15;
            scratch += (crow[2] + 15) & ~(int64_t)15;
        } else {
            for (int k = 0; k < CV_BLOSC_CHUNK_ROW; k++) crow[k] = 0;
            crow[7] = 1;
            refused++;
        }
    }
    *streams = ns; *comp_bytes = comp; *scratch_bytes = scratch;
    return refused;
}

extern "C" int cv_blosc_decode_dev(const uint8_t *comp_dev, int64_t comp_bytes, const int64_t *stream_rows_dev, int64_t streams,
                                   uint8_t *scratch_dev, int64_t scratch_bytes, uint8_t *status_dev, void *stream)
{
    if (streams < 0 || comp_bytes < 0 || scratch_bytes < 0) { cv_set_error("cv_blosc_decode_dev: negative count or size"); return 1; }
    if (streams == 0) return 0;
    if (!comp_dev || !stream_rows_dev || !scratch_dev || !status_dev) { cv_set_error("cv_blosc_decode_dev: null argument"); return 1; }
    if ((uintptr_t)stream_rows_dev & 7) { cv_set_error("cv_blosc_decode_dev: the table must be 8-byte aligned"); return 1; }
    const int64_t blocks = (streams + DECODE_WAVES - 1) / DECODE_WAVES;
    hipLaunchKernelGGL(blosc_decode, dim3((int)(blocks < DECODE_GRID ? blocks : DECODE_GRID)), dim3(DECODE_WAVES * cvl::LANES), 0,
                       (hipStream_t)stream, comp_dev, comp_bytes, stream_rows_dev, streams, scratch_dev, scratch_bytes, status_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cv_set_error("cv_blosc_decode_dev: launch failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int cv_blosc_unpack_dev(const int64_t *chunk_rows_dev, int64_t chunks, const uint8_t *stream_status_dev, int64_t streams,
                                   const uint8_t *scratch_dev, int64_t scratch_bytes, uint8_t *dst_dev, int64_t block_bytes,
                                   int64_t *lens_dev, int32_t *status_dev, void *stream)
{
    if (chunks < 0 || streams < 0 || scratch_bytes < 0 || block_bytes < 0) { cv_set_error("cv_blosc_unpack_dev: negative count or size"); return 1; }
    if (chunks == 0) return 0;
    if (chunks > 65535) { cv_set_error("cv_blosc_unpack_dev: at most 65535 chunks per call"); return 1; }
    if (!chunk_rows_dev || !dst_dev || !lens_dev || !status_dev || (streams > 0 && (!stream_status_dev || !scratch_dev))) {
        cv_set_error("cv_blosc_unpack_dev: null argument");
        return 1;
    }
    if (((uintptr_t)chunk_rows_dev | (uintptr_t)lens_dev) & 7) { cv_set_error("cv_blosc_unpack_dev: tables must be 8-byte aligned"); return 1; }
    int64_t slices = (block_bytes + UNPACK_BYTES - 1) / UNPACK_BYTES;
    if (slices < 1) slices = 1;
    if (slices > 0x7fffffff) { cv_set_error("cv_blosc_unpack_dev: block_bytes too large"); return 1; }
    hipLaunchKernelGGL(blosc_unpack, dim3((unsigned)slices, (unsigned)chunks), dim3(UNPACK_THREADS), 0, (hipStream_t)stream, chunk_rows_dev,
                       chunks, stream_status_dev, streams, scratch_dev, scratch_bytes, dst_dev, block_bytes, lens_dev, status_dev);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { cv_set_error("cv_blosc_unpack_dev: launch failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
