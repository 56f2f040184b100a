// cv_lz4_core.hpp -- the decode core of the .bin block reader on the device (cv_blosc_dev.hip): one LZ4 block stream of
// a c-blosc chunk decoded by one wave, and the rule that finds the ndarray's data inside the unpickled-to-be block.
// Written like cv_inflate_core.hpp, so that the SAME text also compiles for the host: tests/native/lz4_core_driver.cpp
// runs it under AddressSanitizer / UBSan over damaged chunks before any damaged chunk is given to the GPU.
//
// One stream (cb bytes of LZ4 block data, neblock bytes of output, both known from the chunk's tables):
//   window()    all lanes: the next WIN bytes of the stream into LDS, from where the decoding lane reads tokens, length
//               extensions and offsets (a byte read from HBM by one lane costs a memory round trip each)
//   step()      ONE lane: walks sequences into a queue of copy commands (a literal run, a match).  It can stop for a new
//               window at any byte, a length field of a thousand extension bytes included, and goes on where it stopped
//   run()       all lanes: the queued commands, one after the other, LANES bytes per step.  A literal run reads the
//               stream itself; a match whose distance is shorter than its length reads  out[dst - dist + k % dist]:
//               every source byte of a command lies in front of the command's first output byte, so the lanes of one
//               command never depend on each other (a run of one byte of 262 124 bytes is one command)
// The host form runs the same functions with the lane loop written out (LANES "lanes" one after the other).
//
// Safety rules, checked here and nowhere else: every iteration of step() consumes input, moves on to the next field of
// the sequence or ends; input reads stay inside data[0, cb) (the decoder reads the window only); a command is queued
// only after its output range [dst, dst + n) has been checked against [0, neblock) and its source against [0, dst) /
// data[0, cb), so run() needs no checks of its own; the stream must consume exactly cb bytes and produce exactly
// neblock, ending on a sequence of literals only that holds at least one; offset 0 and offsets in front of the output
// are errors.  This is stricter than lz4_decompress of cv_hostio.cpp (which also takes a stream that ends behind a
// match): whatever this core does not vouch for goes back to the host decoder.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVL_FN __host__ __device__ inline
#else
#define CVL_FN inline
#endif

namespace cvl {

constexpr int LANES = 64;
constexpr int QCAP = 64;                 // commands per batch
constexpr int WIN = 2048;                // bytes of input in the window
constexpr uint32_t STREAM_MAX = 0x7fffff00u;
constexpr int STREAM_ROW = 5, CHUNK_ROW = 10;   // int64 words per row of the plan (CV_BLOSC_STREAM_ROW / CV_BLOSC_CHUNK_ROW)

enum : int { K_LIT = 0, K_MATCH = 1 };
enum : int { W_RUN = 0, W_DONE = 1, W_BAD = 2 };                 // what step() asks the wave to do next
enum : int { P_TOKEN = 0, P_LITLEN = 1, P_LITS = 2, P_OFFSET = 3, P_MLEN = 4, P_MATCH = 5 };

struct state {
    uint32_t q_dst[QCAP], q_src[QCAP], q_len[QCAP];   // src: offset in the stream (literals) / distance (match)
    uint8_t q_kind[QCAP];
    uint8_t win[WIN];                    // data[win_lo, win_hi)
    uint32_t win_lo, win_hi;
    int32_t nq, what, refill;            // refill: the decoder wants a window from `pos` on before it goes on
    // ---- the decoder (one lane's)
    uint32_t pos, out;
    uint32_t token, acc, off;
    int32_t phase;
};

CVL_FN void begin(state &S)
{
    S.pos = 0; S.out = 0; S.token = 0; S.acc = 0; S.off = 0; S.phase = P_TOKEN; S.nq = 0; S.what = W_RUN;
    S.win_lo = 0; S.win_hi = 0; S.refill = 1;
}

// all lanes: the window from the decoder's position on (a barrier of the caller's in front and behind)
CVL_FN void window(state &S, const uint8_t *data, uint32_t cb, int lane, int nlanes)
{
    const uint32_t lo = S.pos < cb ? S.pos : cb, n = cb - lo < (uint32_t)WIN ? cb - lo : (uint32_t)WIN;
    for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) S.win[i] = data[lo + i];
}

// ONE lane, after window() and a barrier
CVL_FN void window_loaded(state &S, uint32_t cb)
{
    const uint32_t lo = S.pos < cb ? S.pos : cb;
    S.win_lo = lo; S.win_hi = cb - lo < (uint32_t)WIN ? cb : lo + (uint32_t)WIN;
    S.refill = 0;
}

// `need` bytes from pos on lie in the window?  (the caller has checked them against cb)
CVL_FN bool in_window(const state &S, uint32_t need) { return S.pos >= S.win_lo && S.pos + need <= S.win_hi; }

CVL_FN void push(state &S, int kind, uint32_t src, uint32_t n)
{
    S.q_kind[S.nq] = (uint8_t)kind; S.q_dst[S.nq] = S.out; S.q_src[S.nq] = src; S.q_len[S.nq] = n;
    S.nq++;
    S.out += n;
}

// ONE lane: go on until the queue holds a batch or a new window is needed (W_RUN; S.refill says which), the stream
// has ended (W_DONE; the queue may hold a last batch) or is not one this core vouches for (W_BAD).
CVL_FN int step(state &S, uint32_t cb, uint32_t neblock)
{
    S.nq = 0;
    for (;;) {
        switch (S.phase) {
        case P_TOKEN:
            if (S.pos >= cb) return S.what = W_BAD;                  // ended behind a match, or an empty stream
            if (!in_window(S, 1)) { S.refill = 1; return S.what = W_RUN; }
            S.token = S.win[S.pos++ - S.win_lo];
            S.acc = S.token >> 4;
            S.phase = S.acc == 15 ? P_LITLEN : P_LITS;
            break;
        case P_LITLEN:
        case P_MLEN: {
            if (S.pos >= cb) return S.what = W_BAD;
            if (!in_window(S, 1)) { S.refill = 1; return S.what = W_RUN; }
            const uint32_t b = S.win[S.pos++ - S.win_lo];
            S.acc += b;
            if (S.acc > neblock) return S.what = W_BAD;              // (no length may pass the output; keeps acc small)
            if (b != 255) S.phase = S.phase == P_LITLEN ? P_LITS : P_MATCH;
            break;
        }
        case P_LITS:
            if (S.acc > cb - S.pos || S.acc > neblock - S.out) return S.what = W_BAD;
            if (S.acc) {
                if (S.nq >= QCAP) return S.what = W_RUN;
                push(S, K_LIT, S.pos, S.acc);
                S.pos += S.acc;
            }
            if (S.pos == cb) {                                       // the last sequence: literals only
                if (S.out != neblock || S.acc == 0) return S.what = W_BAD;
                return S.what = W_DONE;
            }
            S.phase = P_OFFSET;
            break;
        case P_OFFSET:
            if (cb - S.pos < 2) return S.what = W_BAD;
            if (!in_window(S, 2)) { S.refill = 1; return S.what = W_RUN; }
            S.off = (uint32_t)S.win[S.pos - S.win_lo] | ((uint32_t)S.win[S.pos + 1 - S.win_lo] << 8);
            S.pos += 2;
            if (S.off == 0 || S.off > S.out) return S.what = W_BAD;
            S.acc = S.token & 15;
            S.phase = S.acc == 15 ? P_MLEN : P_MATCH;
            break;
        default: {                                                   // P_MATCH
            const uint32_t ml = S.acc + 4;
            if (ml > neblock - S.out) return S.what = W_BAD;
            if (S.nq >= QCAP) return S.what = W_RUN;
            push(S, K_MATCH, S.off, ml);
            S.phase = P_TOKEN;
            break;
        }
        }
    }
}

// all lanes: command q of the batch
CVL_FN void run(const state &S, int q, const uint8_t *data, uint8_t *out, int lane, int nlanes)
{
    const uint32_t dst = S.q_dst[q], src = S.q_src[q], n = S.q_len[q];
    if (S.q_kind[q] == K_LIT) {
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) out[dst + k] = data[src + k];
    } else if (src >= n) {
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) out[dst + k] = out[dst - src + k];
    } else if (src == 1) {
        const uint8_t b = out[dst - 1];
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) out[dst + k] = b;
    } else {
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) out[dst + k] = out[dst - src + k % src];
    }
}

inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// The raw data of ONE pickled ndarray inside a decompressed block (see cv_hostio.cpp): the bytes object found by its
// opcode + length in the first 1 KiB -- BINBYTES 'B' (u32) / BINBYTES8 0x8e / BYTEARRAY8 0x96 (u64) of protocols 3-5,
// BINSTRING 'T' of Python 2's protocol 2 -- that holds at least 16 bytes and ends less than 256 bytes in front of the
// end of the stream.  `head` = the first min(n, 1024) bytes of the stream, n = the length of the whole stream.
CVL_FN bool find_array_payload(const uint8_t *head, int64_t n, int64_t *off, int64_t *len)
{
    const int64_t hn = n < 1024 ? n : 1024;
    for (int64_t i = 0; i + 9 < hn; i++) {
        int64_t L = -1, h = 0;
        const uint8_t op = head[i];
        if (op == 'B' || op == 'T') {
            L = (int64_t)((uint32_t)head[i + 1] | ((uint32_t)head[i + 2] << 8) | ((uint32_t)head[i + 3] << 16) | ((uint32_t)head[i + 4] << 24));
            h = 5;
        } else if (op == 0x8e || op == 0x96) {
            uint64_t v = 0;
            for (int k = 7; k >= 0; k--) v = (v << 8) | head[i + 1 + k];
            if (v < (1ull << 40)) L = (int64_t)v;
            h = 9;
        }
        if (L < 0) continue;
        const int64_t endp = i + h + L;
        if (endp <= n && n - endp < 256 && L >= 16) { *off = i + h; *len = L; return true; }
    }
    return false;
}

// byte r of chunk's decompressed stream, from the plane scratch (r < nbytes)
CVL_FN uint8_t plane_byte(const uint8_t *sc, uint32_t r, uint32_t nbytes, uint32_t blocksize, uint32_t ts, bool shuffled)
{
    if (!shuffled) return sc[r];
    const uint32_t b = r / blocksize, rb = r - b * blocksize;
    const uint32_t left = nbytes - b * blocksize, bsize = left < blocksize ? left : blocksize;
    const uint32_t ne = bsize / ts;
    const uint8_t *blk = sc + (size_t)b * blocksize;
    if (rb >= ne * ts) return blk[rb];                                 // the bytes behind the last whole element
    const uint32_t i = rb / ts, j = rb - i * ts;
    return blk[(size_t)j * ne + i];
}

inline int32_t rdi32(const uint8_t *p) { return (int32_t)rd32(p); }

// ONE chunk's header, bstarts and per-split length words, with the checks of cv_blosc_decompress -> one row per stream
// (offset in the slab, cb, offset in the scratch, neblock, stored) and the chunk's row; false = not for the device
// (nothing written that counts).  comp_off / scratch_off: where the chunk and its planes will lie.
inline bool plan_chunk(const uint8_t *chunk, int64_t clen, int64_t comp_off, int64_t scratch_off, int64_t max_nbytes, int64_t first_stream,
                int64_t max_streams, int64_t *srows, int64_t *crow, int64_t *nstreams)
{
    if (!chunk || clen < 16) return false;
    const int flags = chunk[2], typesize = chunk[3] ? chunk[3] : 1;
    const int32_t nbytes = rdi32(chunk + 4), blocksize = rdi32(chunk + 8), cbytes = rdi32(chunk + 12);
    if (chunk[0] != 2) return false;
    if (nbytes < 0 || nbytes > max_nbytes || cbytes > clen || blocksize <= 0) return false;
    if (typesize != 1 && typesize != 4 && typesize != 8) return false;
    int64_t ns = 0;
    auto put = [&](int64_t off, int64_t cb, int64_t oat, int64_t ne, int64_t stored) -> bool {
        if (first_stream + ns >= max_streams) return false;
        int64_t *r = srows + STREAM_ROW * (first_stream + ns);
        r[0] = comp_off + off; r[1] = cb; r[2] = scratch_off + oat; r[3] = ne; r[4] = stored;
        ns++;
        return true;
    };
    bool shuffle = false;
    if (nbytes == 0) {
        // nothing to decode
    } else if (flags & 0x2) {                               // memcpy'd: one stored stream, never shuffled
        if (clen < 16 + (int64_t)nbytes) return false;
        if (!put(16, nbytes, 0, nbytes, 1)) return false;
    } else {
        if (flags & 0x4) return false;                      // bit shuffle
        if (((flags & 0xe0) >> 5) != 1) return false;       // not LZ4 / LZ4HC
        shuffle = (flags & 0x1) && typesize > 1;
        const bool dont_split = (flags & 0x10) != 0;
        const int64_t nblocks = ((int64_t)nbytes + blocksize - 1) / blocksize;
        if (16 + 4 * nblocks > clen) return false;
        const int64_t data0 = 16 + 4 * nblocks;
        for (int64_t b = 0; b < nblocks; b++) {
            int32_t bsize = blocksize;
            bool leftover = false;
            if (b == nblocks - 1 && nbytes % blocksize) { bsize = nbytes % blocksize; leftover = true; }
            int nsplits = 1;
            if (!dont_split && typesize <= 16 && blocksize / typesize >= 128 && !leftover) nsplits = typesize;
            if (bsize % nsplits) return false;              // (the host decoder leaves the rest of such a block unwritten)
            const int32_t neblock = bsize / nsplits;
            int64_t ip = rdi32(chunk + 16 + 4 * b);
            if (ip < data0) return false;
            for (int s = 0; s < nsplits; s++) {
                if (ip + 4 > clen) return false;
                const int32_t cb = rdi32(chunk + ip); ip += 4;
                if (cb < 0 || ip + cb > clen) return false;
                if (!put(ip, cb, b * (int64_t)blocksize + (int64_t)s * neblock, neblock, cb == neblock)) return false;
                ip += cb;
            }
        }
    }
    crow[0] = typesize; crow[1] = shuffle ? 1 : 0; crow[2] = nbytes; crow[3] = blocksize; crow[4] = first_stream; crow[5] = ns;
    crow[6] = scratch_off; crow[7] = 0;
    *nstreams = ns;
    return true;
}


#if !defined(__HIP_DEVICE_COMPILE__)
// The host form: one stream, the lane loops written out.  -> true = OK (out[0, neblock) written).
inline bool lz4_stream_host(const uint8_t *data, uint32_t cb, uint8_t *out, uint32_t neblock)
{
    if (cb > STREAM_MAX || neblock > STREAM_MAX) return false;
    state S;
    begin(S);
    for (;;) {
        if (S.refill) {
            for (int lane = 0; lane < LANES; lane++) window(S, data, cb, lane, LANES);
            window_loaded(S, cb);
        }
        const int what = step(S, cb, neblock);
        if (what == W_BAD) return false;
        for (int q = 0; q < S.nq; q++)
            for (int lane = 0; lane < LANES; lane++) run(S, q, data, out, lane, LANES);
        if (what == W_DONE) return true;
    }
}
#endif

}  // namespace cvl
