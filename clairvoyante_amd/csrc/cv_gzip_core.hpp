// cv_gzip_core.hpp -- the decode core of the ORDINARY gzip reader on the device (cv_gzip_dev.hip): one DEFLATE stream of
// any length, cut into chunks at block starts that were FOUND, not stated.  A sibling of cv_inflate_core.hpp (whose
// tables, window and queue it uses), and like it one text for host and device: tests/test_gzip_core_host.py runs it
// under AddressSanitizer / UBSan over damaged streams.
//
//   header_at()   is there a non-final dynamic-Huffman block header at this BIT offset?  BFINAL = 0, BTYPE = 2,
//                 HLIT <= 29, HDIST <= 29, a complete code-length code, lengths that decode and fill HLIT + HDIST
//                 exactly, a code for symbol 256, a complete literal/length code and a complete distance code.  (zlib
//                 also takes a single one-bit code; the deflate side never writes one, and a header this test misses
//                 only leaves its block to the chunk in front.)  It proves nothing: a chunk start is trusted only
//                 because the chunk in front, decoded from a trusted start, ENDS there (the caller's chain rule).
//   chunk_begin() / chunk_step() / chunk_run()
//                 a chunk = the blocks from a start bit to an end bit (or to BFINAL), of all three types, decoded with
//                 an UNKNOWN window into 16-bit symbols: a byte, or MARK | j = "byte j of the 32 KiB in front of this
//                 chunk".  A match that reaches in front of the chunk yields markers, a match that copies markers copies
//                 them, so one look-up per symbol resolves the chunk once the window is known.
//                 how: LANDED = at a block header exactly at the end bit; FINAL = the block with BFINAL ended; PASSED =
//                 went over the end bit (the end, or the start, is not a true block start); BAD = not a stream this core
//                 vouches for, input exhausted, or more output than `cap`.
//
// Safety rules as in cv_inflate_core.hpp: every iteration consumes input or ends; input reads stay inside data[0, len);
// a command is queued only after [dst, dst + n) has been checked against [0, cap) and its distance against 32 768 and
// against dst + hist (hist = bytes that exist in front of the chunk), so chunk_run() needs no checks of its own.  With
// cap = the length a counting pass found, the writing pass cannot overrun whatever the compression ratio.
#pragma once
#include "cv_inflate_core.hpp"

namespace cvg {

using cvi::state;

constexpr uint32_t WSIZE = 32768;
constexpr uint16_t MARK = 0x8000;
constexpr uint32_t OUT_MAX = 1u << 30;            // symbols of one chunk (a counting pass states no smaller cap)
enum : int { LANDED = 1, FINAL = 2, PASSED = 3, BAD = 4 };

// ---- the header test ------------------------------------------------------------------------------------------------
struct bits {
    const uint8_t *d;
    uint64_t pos, end;                   // in bits
};

// k <= 16 bits at the reader's position; false past the end
CVI_FN bool get(bits &B, int k, uint32_t *v)
{
    if (B.pos + (uint64_t)k > B.end) return false;
    const uint64_t by = B.pos >> 3, last = (B.end - 1) >> 3;
    uint32_t w = B.d[by];
    if (by + 1 <= last) w |= (uint32_t)B.d[by + 1] << 8;
    if (by + 2 <= last) w |= (uint32_t)B.d[by + 2] << 16;
    *v = (w >> (B.pos & 7)) & ((1u << k) - 1);
    B.pos += (uint64_t)k;
    return true;
}

// Kraft sum of n code lengths in units of 2^-15; 1 << 15 = complete
CVI_FN uint32_t kraft(const uint8_t *lens, int n)
{
    uint32_t s = 0;
    for (int i = 0; i < n; i++)
        if (lens[i]) s += 1u << (15 - lens[i]);
    return s;
}

// the 57 bits from `bit` on (zeros behind the end): eight independent byte loads, no look at what they hold in between
CVI_FN uint64_t peek(const uint8_t *data, uint64_t nbytes, uint64_t bit)
{
    const uint64_t by = bit >> 3;
    uint64_t w = 0;
    if (by + 8 <= nbytes) {
        for (int i = 0; i < 8; i++) w |= (uint64_t)data[by + i] << (8 * i);
    } else {
        for (int i = 0; by + i < nbytes; i++) w |= (uint64_t)data[by + i] << (8 * i);
    }
    return w >> (bit & 7);
}

CVI_FN bool header_at(const uint8_t *data, uint64_t nbytes, uint64_t bit)
{
    const uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    // the 17 bits nearly every offset fails on, and the code-length code's lengths, from two peeks
    if (bit + 17 > nbytes * 8) return false;
    const uint64_t head = peek(data, nbytes, bit);
    if ((head & 7) != 4) return false;                                   // BFINAL 0, BTYPE 2
    uint32_t v = (uint32_t)(head >> 3) & 0x3fff;
    const int hlit = (int)(v & 31) + 257, hdist = (int)((v >> 5) & 31) + 1, hclen = (int)((v >> 10) & 15) + 4;
    if (hlit > 286 || hdist > 30) return false;
    if (bit + 17 + 3 * (uint64_t)hclen > nbytes * 8) return false;
    uint64_t three = peek(data, nbytes, bit + 17);                       // (19 * 3 = 57 bits at the most)
    uint8_t cl[19];
    for (int i = 0; i < 19; i++) cl[i] = 0;
    for (int i = 0; i < hclen; i++) { cl[ORDER[i]] = (uint8_t)(three & 7); three >>= 3; }
    if (kraft(cl, 19) != 1u << 15) return false;
    bits B = {data, bit + 17 + 3 * (uint64_t)hclen, nbytes * 8};
    // the canonical code-length code: codes per length, first code and first index of each length, symbols in order
    uint8_t count[8], sorted[19];
    for (int l = 0; l < 8; l++) count[l] = 0;
    for (int i = 0; i < 19; i++) count[cl[i]]++;
    count[0] = 0;
    {
        uint8_t next[8];
        int at = 0;
        for (int l = 1; l < 8; l++) { next[l] = (uint8_t)at; at += count[l]; }
        for (int i = 0; i < 19; i++)
            if (cl[i]) sorted[next[cl[i]]++] = (uint8_t)i;
    }
    uint8_t all[286 + 30];
    const int total = hlit + hdist;
    int i = 0;
    while (i < total) {
        int code = 0, first = 0, index = 0, sym = -1;
        for (int n = 1; n <= 7; n++) {
            if (!get(B, 1, &v)) return false;
            code |= (int)v;
            const int c = count[n];
            if (code - c < first) { sym = sorted[index + (code - first)]; break; }
            index += c; first += c; first <<= 1; code <<= 1;
        }
        if (sym < 0) return false;
        if (sym < 16) { all[i++] = (uint8_t)sym; continue; }
        int rep; uint8_t fillv = 0;
        if (sym == 16) {
            if (i == 0) return false;
            fillv = all[i - 1];
            if (!get(B, 2, &v)) return false;
            rep = 3 + (int)v;
        } else if (sym == 17) {
            if (!get(B, 3, &v)) return false;
            rep = 3 + (int)v;
        } else {
            if (!get(B, 7, &v)) return false;
            rep = 11 + (int)v;
        }
        if (i + rep > total) return false;
        while (rep--) all[i++] = fillv;
    }
    if (all[256] == 0) return false;
    return kraft(all, hlit) == 1u << 15 && kraft(all + hlit, hdist) == 1u << 15;
}

// ---- a chunk --------------------------------------------------------------------------------------------------------
// ONE lane.  The chunk's data starts `skip` (0..7) bits into data[0]; after it window() / window_loaded() as usual.
CVI_FN void chunk_begin(state &S) { cvi::begin(S); }

// ONE lane, once, after the first window: drops the bits in front of the start
CVI_FN bool chunk_skip(state &S, int skip)
{
    cvi::refill(S);
    if (S.cnt < skip) return false;
    cvi::drop(S, skip);
    return true;
}

CVI_FN int64_t bit_at(const state &S) { return (int64_t)S.pos * 8 - S.cnt; }

// ONE lane: as cvi::step().  end_bit: relative to data[0], < 0 = none (the chunk ends at BFINAL).  W_DONE: *how says
// how; W_BAD: *how = BAD.  The queue may hold a last batch in both cases only for W_DONE.
CVI_FN int chunk_step(state &S, uint32_t len, int64_t end_bit, uint32_t cap, uint32_t hist, int32_t *how)
{
    const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    S.nq = 0;
    uint32_t nlits = 0, run = 0;
    uint32_t v;
    *how = BAD;
    for (;;) {
        if (!S.in_block) {
            if (run) { cvi::push(S, cvi::K_LIT, nlits - run, run); run = 0; }
            if (S.last) { *how = FINAL; return S.what = cvi::W_DONE; }
            if (end_bit >= 0 && bit_at(S) >= end_bit) {
                *how = bit_at(S) == end_bit ? LANDED : PASSED;
                return S.what = cvi::W_DONE;
            }
            if (S.nq >= cvi::QCAP - 1 || cvi::short_of_input(S, len, cvi::HEADER_NEED)) return S.what = cvi::W_RUN;
            cvi::refill(S);
            if (!cvi::take(S, 3, &v)) return S.what = cvi::W_BAD;
            S.last = (int32_t)(v & 1);
            const int type = (int)(v >> 1);
            if (type == 0) {
                cvi::drop(S, S.cnt & 7);
                cvi::refill(S);
                uint32_t a, b;
                if (!cvi::take(S, 16, &a) || !cvi::take(S, 16, &b)) return S.what = cvi::W_BAD;
                if ((a ^ b) != 0xffffu) return S.what = cvi::W_BAD;
                const uint32_t at = S.pos - (uint32_t)(S.cnt >> 3);
                if (a > len - at || a > cap - S.out) return S.what = cvi::W_BAD;
                if (a) cvi::push(S, cvi::K_STORED, at, a);
                S.pos = at + a; S.buf = 0; S.cnt = 0;
                continue;
            }
            if (type == 3) return S.what = cvi::W_BAD;
            if (type == 1) {
                int s = 0;
                for (; s < 144; s++) S.lens[s] = 8;
                for (; s < 256; s++) S.lens[s] = 9;
                for (; s < 280; s++) S.lens[s] = 7;
                for (; s < 288; s++) S.lens[s] = 8;
                for (s = 0; s < 32; s++) S.lens[cvi::NLIT + s] = 5;
                if (!cvi::bookkeeping(S, 0, cvi::NLIT) || !cvi::bookkeeping(S, 1, cvi::NDIST)) return S.what = cvi::W_BAD;
            } else if (!cvi::dynamic_header(S)) {
                return S.what = cvi::W_BAD;
            }
            S.in_block = 1;
            return S.what = cvi::W_FILL;
        }
        if (end_bit >= 0 && bit_at(S) > end_bit) {                       // a block that straddles the end: not a chain
            if (run) cvi::push(S, cvi::K_LIT, nlits - run, run);
            *how = PASSED;
            return S.what = cvi::W_DONE;
        }
        if (S.nq >= cvi::QCAP - 1 || nlits >= (uint32_t)cvi::LITCAP || cvi::short_of_input(S, len, cvi::SYMBOL_NEED)) {
            if (run) cvi::push(S, cvi::K_LIT, nlits - run, run);
            return S.what = cvi::W_RUN;
        }
        cvi::refill(S);
        const int sym = cvi::symbol(S, 0);
        if (sym < 0) return S.what = cvi::W_BAD;
        if (sym < 256) {
            if (S.out + run >= cap) return S.what = cvi::W_BAD;
            S.lits[nlits++] = (uint8_t)sym; run++;
            continue;
        }
        if (run) { cvi::push(S, cvi::K_LIT, nlits - run, run); run = 0; }
        if (sym == 256) { S.in_block = 0; continue; }
        if (sym > 285) return S.what = cvi::W_BAD;
        if (!cvi::take(S, LEN_EXTRA[sym - 257], &v)) return S.what = cvi::W_BAD;
        const uint32_t n = LEN_BASE[sym - 257] + v;
        cvi::refill(S);
        const int ds = cvi::symbol(S, 1);
        if (ds < 0 || ds > 29) return S.what = cvi::W_BAD;
        if (!cvi::take(S, DIST_EXTRA[ds], &v)) return S.what = cvi::W_BAD;
        const uint32_t d = DIST_BASE[ds] + v;
        if (d > WSIZE || (d > S.out && d - S.out > hist) || n > cap - S.out) return S.what = cvi::W_BAD;
        cvi::push(S, cvi::K_MATCH, d, n);
    }
}

// all lanes: command q of the batch into the chunk's symbols
CVI_FN void chunk_run(const state &S, int q, const uint8_t *data, uint16_t *out, int lane, int nlanes)
{
    const uint32_t dst = S.q_dst[q], src = S.q_src[q], n = S.q_len[q];
    const int kind = S.q_kind[q];
    if (kind == cvi::K_LIT) {
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) out[dst + k] = S.lits[src + k];
    } else if (kind == cvi::K_STORED) {
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) out[dst + k] = data[src + k];
    } else {
        for (uint32_t k = (uint32_t)lane; k < n; k += (uint32_t)nlanes) {
            const int64_t at = (int64_t)dst - (int64_t)src + (int64_t)(src >= n ? k : k % src);
            out[dst + k] = at < 0 ? (uint16_t)(MARK | (uint32_t)((int64_t)WSIZE + at)) : out[at];
        }
    }
}

// one symbol with the window known: `before` = the text in front of the chunk, before[-1] its last byte.  *bad is set
// for a marker that reaches in front of the `hist` bytes that exist there.
CVI_FN uint8_t resolve(uint16_t sym, const uint8_t *before, int64_t hist, int32_t *bad)
{
    if (!(sym & MARK)) return (uint8_t)sym;
    const int64_t back = (int64_t)WSIZE - (int64_t)(sym & (MARK - 1));  // 1 .. 32768
    if (back > hist) { *bad = 1; return 0; }
    return before[-back];
}

// The host form: one chunk, the lane loops written out.  data[0, len), the chunk starts at start_bit and ends at
// end_bit (< 0: at BFINAL), both relative to data[0].  out: room for `cap` symbols, or null to count only.
// -> how; *n symbols, *ended = the bit the chunk ended at.
inline int chunk_host(const uint8_t *data, uint64_t len64, int64_t start_bit, int64_t end_bit, uint16_t *out, uint32_t cap,
                      uint32_t hist, uint32_t *n, int64_t *ended)
{
    *n = 0; *ended = start_bit;
    if (start_bit < 0 || (uint64_t)start_bit >= len64 * 8) return BAD;
    const uint64_t base = (uint64_t)start_bit >> 3;
    if (len64 - base > 0x7fffffffu) return BAD;
    const uint32_t len = (uint32_t)(len64 - base);
    const uint8_t *d = data + base;
    const int64_t rel_end = end_bit < 0 ? -1 : end_bit - (int64_t)base * 8;
    if (!out) cap = OUT_MAX;
    state S;
    chunk_begin(S);
    bool first = true;
    int32_t how = BAD;
    for (;;) {
        if (first || cvi::short_of_input(S, len, cvi::HEADER_NEED)) {
            for (int lane = 0; lane < cvi::LANES; lane++) cvi::window(S, d, len, lane, cvi::LANES);
            cvi::window_loaded(S, len);
            if (first && !chunk_skip(S, (int)(start_bit & 7))) return BAD;
            first = false;
        }
        const int what = chunk_step(S, len, rel_end, cap, hist, &how);
        if (what == cvi::W_BAD) return BAD;
        if (out)
            for (int q = 0; q < S.nq; q++)
                for (int lane = 0; lane < cvi::LANES; lane++) chunk_run(S, q, d, out, lane, cvi::LANES);
        if (what == cvi::W_FILL)
            for (int pass = 0; pass < 2; pass++)
                for (int lane = 0; lane < cvi::LANES; lane++) cvi::fill(S, pass, lane, cvi::LANES);
        if (what == cvi::W_DONE) break;
    }
    *n = S.out;
    *ended = (int64_t)base * 8 + bit_at(S);
    return how;
}

}  // namespace cvg
