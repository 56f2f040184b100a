// cv_inflate_core.hpp -- the raw-DEFLATE (RFC 1951) decode core of the BGZF reader on the device (cv_inflate_dev.hip),
// written so that the SAME text also compiles for the host: tests/native/bgzf_core_driver.cpp runs it under
// AddressSanitizer / UBSan over damaged members before any damaged member is given to the GPU.
//
// One member (<= 64 KiB of DEFLATE data, <= 64 KiB of output, both sizes known from the BGZF header / trailer) is
// decoded by one wave:
//   window()    all lanes: the next WIN bytes of the DEFLATE data into LDS, from where the decoding lane reads them (a
//               byte read from HBM by one lane costs a memory round trip each)
//   step()      ONE lane: reads block headers, builds the canonical-Huffman bookkeeping (codes per length, symbols in
//               code order), decodes symbols into a queue of copy commands (a run of literals, a match, a stored block)
//   fill()      all lanes: the first-level lookup tables (10 bits literal/length, 8 bits distance) from that bookkeeping;
//               codes longer than the table walk the canonical code bit by bit (at most 15 steps)
//   run()       all lanes: the queued commands, one after the other, LANES bytes per step.  A match whose distance is
//               shorter than its length reads  out[dst - dist + k % dist]: every source byte of a command lies in front
//               of the command's first output byte, so the lanes of one command never depend on each other
//   crc         every lane the CRC-32 state of one 1 KiB chunk (chunks are aligned to the END of the member, so all but
//               the first are whole), folded with the constant GF(2) operator "1024 zero bytes follow"
// The host form runs the same functions with the lane loop written out (LANES "lanes" one after the other).
//
// Safety rules, checked here and nowhere else: every loop iteration consumes at least one input bit or ends; input
// reads stay inside data[0, len) (the decoder reads the window only, and stops for a new one while the bytes ahead
// still cover the longest thing it reads in one go: HEADER_NEED at a block header, SYMBOL_NEED inside a block); a
// command is queued only after its output range [dst, dst + n) has been checked against [0, isize) and its source
// against [0, dst) / data[0, len); so run() needs no checks of its own.
// Strictness follows zlib (an incomplete code is an error unless it is a single one-bit code, 286 / 287 and distance
// codes 30 / 31 are errors): whatever this core does not vouch for goes back to the host decoder.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVI_FN __host__ __device__ inline
#else
#define CVI_FN inline
#endif

namespace cvi {

constexpr int LANES = 64;
constexpr int LBITS = 10, DBITS = 8, MAXBITS = 15;
constexpr int NLIT = 288, NDIST = 32;
constexpr int QCAP = 64;                 // commands per batch
constexpr int LITCAP = 512;              // literal bytes per batch
constexpr int WIN = 2048;                // bytes of input in the window
constexpr uint32_t HEADER_NEED = 640;    // a dynamic header: 14 + 19 * 3 + 316 * (7 + 7) bits, and the refill's 8 bytes
constexpr uint32_t SYMBOL_NEED = 16;     // a length / distance pair with its extra bits: 48 bits, and two refills
constexpr int CRC_CHUNK = 1024;          // LANES * CRC_CHUNK = 65536 = the largest member
constexpr uint32_t MEMBER_MAX = 65536;

enum : int { K_LIT = 0, K_MATCH = 1, K_STORED = 2 };
enum : int { W_RUN = 0, W_FILL = 1, W_DONE = 2, W_BAD = 3 };     // what step() asks the wave to do next

struct state {
    // ---- tables
    uint16_t lit[1 << LBITS];            // (symbol << 4) | code length; 0 = not here: walk the canonical code
    uint16_t dist[1 << DBITS];
    uint16_t sorted[NLIT + NDIST];       // symbols in code order (literal/length, then distance)
    uint16_t count[2][MAXBITS + 1];      // codes of each length
    uint16_t start[2][MAXBITS + 1];      // index in `sorted` of the first code of each length
    uint16_t first[2][MAXBITS + 1];      // its code
    uint8_t lens[NLIT + NDIST];
    // ---- the batch
    uint32_t q_dst[QCAP], q_src[QCAP];   // src: offset in `lits` / distance / offset in the DEFLATE data
    uint16_t q_len[QCAP];
    uint8_t q_kind[QCAP];
    uint8_t lits[LITCAP];
    uint8_t win[WIN];                    // data[win_lo, win_hi)
    uint32_t win_lo, win_hi;
    int32_t nq, what;
    // ---- the decoder (one lane's)
    uint64_t buf;
    int32_t cnt;
    uint32_t pos, out;
    int32_t in_block, last;              // in_block: 0 = at a block header, 1 = inside a Huffman block
};

struct crc_consts {
    uint32_t shift[32];                  // column i = the CRC state 1 << i after CRC_CHUNK zero bytes
};

CVI_FN uint32_t crc_byte_table(uint32_t i)
{
    for (int k = 0; k < 8; k++) i = (i & 1) ? 0xEDB88320u ^ (i >> 1) : i >> 1;
    return i;
}

inline void make_crc_consts(crc_consts *c)
{
    uint32_t t[256];
    for (uint32_t i = 0; i < 256; i++) t[i] = crc_byte_table(i);
    for (int b = 0; b < 32; b++) {
        uint32_t s = 1u << b;
        for (int k = 0; k < CRC_CHUNK; k++) s = t[s & 0xff] ^ (s >> 8);
        c->shift[b] = s;
    }
}

CVI_FN void refill(state &S)
{
    while (S.cnt <= 56 && S.pos < S.win_hi) { S.buf |= (uint64_t)S.win[S.pos++ - S.win_lo] << S.cnt; S.cnt += 8; }
}

// the decoder must not go on with the window it has: fewer than `need` bytes ahead, and the data goes on behind it
CVI_FN bool short_of_input(const state &S, uint32_t len, uint32_t need) { return S.win_hi < len && S.pos + need > S.win_hi; }

// all lanes: the window from the decoder's position on (a barrier of the caller's in front and behind)
CVI_FN void window(state &S, const uint8_t *data, uint32_t len, int lane, int nlanes)
{
    const uint32_t lo = S.pos < len ? S.pos : len, n = len - lo < (uint32_t)WIN ? len - lo : (uint32_t)WIN;
    for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) S.win[i] = data[lo + i];
}

// ONE lane, after window() and a barrier
CVI_FN void window_loaded(state &S, uint32_t len)
{
    const uint32_t lo = S.pos < len ? S.pos : len;
    S.win_lo = lo; S.win_hi = len - lo < (uint32_t)WIN ? len : lo + (uint32_t)WIN;
    S.pos = lo;
}

CVI_FN void drop(state &S, int k) { S.buf >>= k; S.cnt -= k; }

// k <= 16 bits; false when the input has run out
CVI_FN bool take(state &S, int k, uint32_t *v)
{
    if (S.cnt < k) return false;
    *v = (uint32_t)S.buf & ((1u << k) - 1);
    drop(S, k);
    return true;
}

// one symbol of code `which` (0 literal/length, 1 distance); -1 = invalid code or input exhausted.  The caller has
// refilled: at least 15 bits are in the buffer unless the input ends.
CVI_FN int symbol(state &S, int which)
{
    const uint32_t e = which ? S.dist[S.buf & ((1u << DBITS) - 1)] : S.lit[S.buf & ((1u << LBITS) - 1)];
    const int l = (int)(e & 15);
    if (l) {
        if (l > S.cnt) return -1;
        drop(S, l);
        return (int)(e >> 4);
    }
    const uint16_t *count = S.count[which];
    int code = 0, first = 0, index = 0;
    uint64_t v = S.buf;
    for (int n = 1; n <= MAXBITS; n++) {
        code |= (int)(v & 1); v >>= 1;
        const int c = count[n];
        if (code - c < first) {
            if (n > S.cnt) return -1;
            drop(S, n);
            return S.sorted[(which ? NLIT : 0) + index + (code - first)];
        }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return -1;
}

// code lengths -> count / start / first / sorted of code `which`.  false: over-subscribed, or incomplete in a way
// zlib rejects.
CVI_FN bool bookkeeping(state &S, int which, int n)
{
    const uint8_t *lens = S.lens + (which ? NLIT : 0);
    uint16_t *count = S.count[which], *start = S.start[which], *first = S.first[which];
    for (int l = 0; l <= MAXBITS; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[lens[s]]++;
    count[0] = 0;
    int left = 1, max = 0;
    uint32_t code = 0, at = 0;
    for (int l = 1; l <= MAXBITS; l++) {
        left = left * 2 - count[l];
        if (left < 0) return false;
        if (count[l]) max = l;
        code = (code + count[l - 1]) << 1;
        first[l] = (uint16_t)code;
        start[l] = (uint16_t)at;
        at += count[l];
    }
    if (left > 0 && max > 1) return false;
    uint16_t next[MAXBITS + 1];
    for (int l = 1; l <= MAXBITS; l++) next[l] = start[l];
    uint16_t *sorted = S.sorted + (which ? NLIT : 0);
    for (int s = 0; s < n; s++)
        if (lens[s]) sorted[next[lens[s]]++] = (uint16_t)s;
    return true;
}

// all lanes: the first-level tables from the bookkeeping.  Two passes with a barrier of the caller's between them
// (pass 0 clears, pass 1 writes): different lanes write the same entries.
CVI_FN void fill(state &S, int pass, int lane, int nlanes)
{
    if (pass == 0) {
        for (int i = lane; i < (1 << LBITS); i += nlanes) S.lit[i] = 0;
        for (int i = lane; i < (1 << DBITS); i += nlanes) S.dist[i] = 0;
        return;
    }
    for (int which = 0; which < 2; which++) {
        const int tbits = which ? DBITS : LBITS;
        uint16_t *tab = which ? S.dist : S.lit;
        const uint16_t *sorted = S.sorted + (which ? NLIT : 0);
        const uint8_t *lens = S.lens + (which ? NLIT : 0);
        int total = 0;
        for (int l = 1; l <= tbits; l++) total += S.count[which][l];       // (codes up to tbits come first in `sorted`)
        for (int j = lane; j < total; j += nlanes) {
            const int s = sorted[j], l = lens[s];
            uint32_t code = (uint32_t)S.first[which][l] + (uint32_t)(j - S.start[which][l]), rev = 0;
            for (int k = 0; k < l; k++) { rev = (rev << 1) | (code & 1); code >>= 1; }
            const uint16_t e = (uint16_t)((s << 4) | l);
            for (uint32_t i = rev; i < (1u << tbits); i += 1u << l) tab[i] = e;
        }
    }
}

CVI_FN void begin(state &S)
{
    S.buf = 0; S.cnt = 0; S.pos = 0; S.out = 0; S.in_block = 0; S.last = 0; S.nq = 0; S.what = W_RUN;
    S.win_lo = 0; S.win_hi = 0;
}

CVI_FN bool push(state &S, int kind, uint32_t src, uint32_t n)
{
    S.q_kind[S.nq] = (uint8_t)kind; S.q_dst[S.nq] = S.out; S.q_src[S.nq] = src; S.q_len[S.nq] = (uint16_t)n;
    S.nq++;
    S.out += n;
    return true;
}

// the header of a dynamic block: code lengths into S.lens; false = malformed
CVI_FN bool dynamic_header(state &S)
{
    const uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v;
    refill(S);
    if (!take(S, 14, &v)) return false;
    const int hlit = (int)(v & 31) + 257, hdist = (int)((v >> 5) & 31) + 1, hclen = (int)((v >> 10) & 15) + 4;
    if (hlit > 286 || hdist > 30) return false;
    // the code-length code borrows the distance slots of the state while it is needed
    uint8_t *cl = S.lens + NLIT;
    for (int i = 0; i < 19; i++) cl[i] = 0;
    for (int i = 0; i < hclen; i++) {
        refill(S);
        if (!take(S, 3, &v)) return false;
        cl[ORDER[i]] = (uint8_t)v;
    }
    if (!bookkeeping(S, 1, 19)) return false;
    {   // (zlib takes no incomplete code-length code at all)
        int left = 1;
        for (int l = 1; l <= 7; l++) left = left * 2 - S.count[1][l];
        bool any = false;
        for (int l = 1; l <= 7; l++) any = any || S.count[1][l];
        if (any && left > 0) return false;
    }
    for (int i = 0; i < (1 << DBITS); i++) S.dist[i] = 0;              // (all of it through the canonical walk)
    uint8_t all[286 + 30];
    const int total = hlit + hdist;
    int i = 0;
    while (i < total) {
        refill(S);
        const int sym = symbol(S, 1);
        if (sym < 0) return false;
        if (sym < 16) { all[i++] = (uint8_t)sym; continue; }
        int rep; uint8_t fillv = 0;
        if (sym == 16) {
            if (i == 0) return false;
            fillv = all[i - 1];
            if (!take(S, 2, &v)) return false;
            rep = 3 + (int)v;
        } else if (sym == 17) {
            if (!take(S, 3, &v)) return false;
            rep = 3 + (int)v;
        } else {
            if (!take(S, 7, &v)) return false;
            rep = 11 + (int)v;
        }
        if (i + rep > total) return false;
        while (rep--) all[i++] = fillv;
    }
    if (all[256] == 0) return false;                                    // no end-of-block code
    for (int s = 0; s < NLIT + NDIST; s++) S.lens[s] = 0;
    for (int s = 0; s < hlit; s++) S.lens[s] = all[s];
    for (int s = 0; s < hdist; s++) S.lens[NLIT + s] = all[hlit + s];
    return bookkeeping(S, 0, NLIT) && bookkeeping(S, 1, NDIST);
}

// ONE lane: go on until the queue holds a batch (W_RUN), the tables must be filled (W_FILL), the stream has ended
// (W_DONE; the queue may hold a last batch) or is not one this core vouches for (W_BAD).
CVI_FN int step(state &S, uint32_t len, uint32_t isize)
{
    const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    S.nq = 0;
    uint32_t nlits = 0, run = 0;          // literal bytes of this batch; of them in the run that is still open
    uint32_t v;
    for (;;) {
        if (!S.in_block) {
            if (run) { push(S, K_LIT, nlits - run, run); run = 0; }
            if (S.last) {
                // the stream ends here: all of the output, and nothing but padding bits and whole unread bytes? (the
                // DEFLATE data of a BGZF member ends at the byte the last block ends in)
                if (S.out != isize || S.pos != len || S.cnt >= 8) return S.what = W_BAD;
                return S.what = W_DONE;
            }
            if (S.nq >= QCAP - 1 || short_of_input(S, len, HEADER_NEED)) return S.what = W_RUN;
            refill(S);
            if (!take(S, 3, &v)) return S.what = W_BAD;
            S.last = (int32_t)(v & 1);
            const int type = (int)(v >> 1);
            if (type == 0) {                                             // stored: 3 header bits, then byte-aligned
                drop(S, S.cnt & 7);
                refill(S);
                uint32_t a, b;
                if (!take(S, 16, &a) || !take(S, 16, &b)) return S.what = W_BAD;
                if ((a ^ b) != 0xffffu) return S.what = W_BAD;
                const uint32_t at = S.pos - (uint32_t)(S.cnt >> 3);      // first byte not yet consumed
                if (a > len - at || a > isize - S.out) return S.what = W_BAD;
                if (a) push(S, K_STORED, at, a);
                S.pos = at + a; S.buf = 0; S.cnt = 0;               // (behind the window, perhaps: nothing is read there)
                continue;
            }
            if (type == 3) return S.what = W_BAD;
            if (type == 1) {
                int s = 0;
                for (; s < 144; s++) S.lens[s] = 8;
                for (; s < 256; s++) S.lens[s] = 9;
                for (; s < 280; s++) S.lens[s] = 7;
                for (; s < 288; s++) S.lens[s] = 8;
                for (s = 0; s < 32; s++) S.lens[NLIT + s] = 5;
                if (!bookkeeping(S, 0, NLIT) || !bookkeeping(S, 1, NDIST)) return S.what = W_BAD;
            } else if (!dynamic_header(S)) {
                return S.what = W_BAD;
            }
            S.in_block = 1;
            return S.what = W_FILL;                                      // (the queue is run first, then the tables filled)
        }
        if (S.nq >= QCAP - 1 || nlits >= LITCAP || short_of_input(S, len, SYMBOL_NEED)) {
            if (run) push(S, K_LIT, nlits - run, run);
            return S.what = W_RUN;
        }
        refill(S);
        const int sym = symbol(S, 0);
        if (sym < 0) return S.what = W_BAD;
        if (sym < 256) {
            if (S.out + run >= isize) return S.what = W_BAD;
            S.lits[nlits++] = (uint8_t)sym; run++;
            continue;
        }
        if (run) { push(S, K_LIT, nlits - run, run); run = 0; }
        if (sym == 256) { S.in_block = 0; continue; }
        if (sym > 285) return S.what = W_BAD;
        if (!take(S, LEN_EXTRA[sym - 257], &v)) return S.what = W_BAD;
        const uint32_t n = LEN_BASE[sym - 257] + v;
        refill(S);
        const int ds = symbol(S, 1);
        if (ds < 0 || ds > 29) return S.what = W_BAD;
        if (!take(S, DIST_EXTRA[ds], &v)) return S.what = W_BAD;
        const uint32_t d = DIST_BASE[ds] + v;
        if (d > S.out || n > isize - S.out) return S.what = W_BAD;
        push(S, K_MATCH, d, n);
    }
}

// all lanes: command q of the batch
CVI_FN void run(const state &S, int q, const uint8_t *data, uint8_t *out, int lane, int nlanes)
{
    const uint32_t dst = S.q_dst[q], src = S.q_src[q], n = S.q_len[q];
    const int kind = S.q_kind[q];
    if (kind == K_LIT) {
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) out[dst + k] = S.lits[src + k];
    } else if (kind == K_STORED) {
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

// lane `lane`'s chunk of the member's CRC: the state after its bytes, started from 0xffffffff by the lane that holds
// the first byte and from 0 by the others (so the states combine linearly); lanes without a chunk give 0
CVI_FN uint32_t crc_chunk(const uint8_t *out, uint32_t isize, int lane, const uint32_t *byte_table)
{
    const uint32_t nchunks = (isize + CRC_CHUNK - 1) / CRC_CHUNK;
    if ((uint32_t)lane >= nchunks) return 0;
    const uint32_t head = isize - (nchunks - 1) * CRC_CHUNK;             // bytes of the first chunk, 1 .. CRC_CHUNK
    const uint32_t lo = lane ? head + (uint32_t)(lane - 1) * CRC_CHUNK : 0, hi = lane ? lo + CRC_CHUNK : head;
    uint32_t s = lane ? 0u : 0xffffffffu;
    for (uint32_t i = lo; i < hi; i++) s = byte_table[(s ^ out[i]) & 0xff] ^ (s >> 8);
    return s;
}

// ONE lane: the member's CRC-32 from the chunk states part[0 .. chunks)
CVI_FN uint32_t crc_fold(const uint32_t *part, uint32_t isize, const crc_consts &C)
{
    const uint32_t nchunks = (isize + CRC_CHUNK - 1) / CRC_CHUNK;
    if (nchunks == 0) return 0;
    uint32_t acc = part[0];
    for (uint32_t c = 1; c < nchunks; c++) {
        uint32_t moved = 0;
        for (int b = 0; b < 32; b++) moved ^= ((acc >> b) & 1) ? C.shift[b] : 0u;
        acc = moved ^ part[c];
    }
    return ~acc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The host form: one member, the lane loops written out.  -> true = OK (out[0, isize) written, its CRC-32 is `crc`).
inline bool inflate_member_host(const uint8_t *data, uint32_t len, uint8_t *out, uint32_t isize, uint32_t crc)
{
    if (isize > MEMBER_MAX || len > MEMBER_MAX) return false;
    static const crc_consts C = [] { crc_consts c; make_crc_consts(&c); return c; }();
    state S;
    begin(S);
    for (;;) {
        if (short_of_input(S, len, HEADER_NEED)) {
            for (int lane = 0; lane < LANES; lane++) window(S, data, len, lane, LANES);
            window_loaded(S, len);
        }
        const int what = step(S, len, isize);
        if (what == W_BAD) return false;
        for (int q = 0; q < S.nq; q++)
            for (int lane = 0; lane < LANES; lane++) run(S, q, data, out, lane, LANES);
        if (what == W_FILL)
            for (int pass = 0; pass < 2; pass++)
                for (int lane = 0; lane < LANES; lane++) fill(S, pass, lane, LANES);
        if (what == W_DONE) break;
    }
    uint32_t table[256], part[LANES];
    for (uint32_t i = 0; i < 256; i++) table[i] = crc_byte_table(i);
    for (int lane = 0; lane < LANES; lane++) part[lane] = crc_chunk(out, isize, lane, table);
    return crc_fold(part, isize, C) == crc;
}
#endif

}  // namespace cvi
