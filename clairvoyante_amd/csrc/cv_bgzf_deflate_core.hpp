// cv_bgzf_deflate_core.hpp -- one BGZF member (<= 65 280 input bytes) compressed by one workgroup: the 18-byte header of
// utils_v2.BgzfWriter.member, ONE final DEFLATE block (RFC 1951: the smallest of stored, fixed and dynamic Huffman), the
// CRC-32 / ISIZE trailer.  The SAME text compiles for the device (cv_bgzf_deflate_dev.hip) and for the host
// (cv_bgzf_deflate_host_form, tests/native/bgzf_deflate_driver.cpp under ASan / UBSan): member() is a list of phases, a
// phase is what every one of THREADS "threads" does between two barriers (CVD_ALL: on the device the statement and
// __syncthreads(), on the host the loop over tid written out).  Nothing a phase reads is written in the same phase except
// through a max, an OR or a sum, so the bytes depend on no timing and both forms write the same member.
//
// The encoder is position-parallel, not the one-sequence-at-a-time walk of the LZ4 packer (4.6.1):
//   load      the text into LDS (zeros behind it, so that four-byte compares may read past the end), tables cleared
//   match     tiles of THREADS positions, in order.  Every position of a tile at once: the candidate of a hash table of
//             three-byte prefixes that holds positions of EARLIER tiles only (entry = the largest position + 1, an atomic
//             max), plus the distances 1, 2, 3, 4 and 8 the table cannot know inside a tile (distance 1 and 4 are the
//             "0.0 0.0 ..." runs of tensor rows).  The longest wins, the nearer on a tie; no candidate beyond 32 768 bytes;
//             a three-byte match further than 4 096 back stays a literal (it costs more than it saves).  The verdict of a
//             position is one word in the caller's workspace: a literal byte, or length and distance.  Then the tile's
//             own positions enter the table.
//   parse     greedy, i -> i + max(1, length[i]): the lengths as 16-bit steps fill the LDS the text and the hash table
//             no longer need, ONE lane chases through them (no global memory in that loop) and sets a bit per chosen
//             position.
//   count     every chosen position adds to the literal/length and distance histograms (LDS atomic adds)
//   codes     ranks in parallel, then one lane per alphabet: Huffman by two queues over the sorted leaves, depths, the
//             lengths limited to 15 (7 for the code-length code) by moving codes down until the Kraft sum is exactly 1;
//             an alphabet with fewer than two used symbols gets a second one, so every code is complete.  The RLE of the
//             lengths (16 / 17 / 18), its code, the three costs, the choice.
//   emit      tiles again: code and extra bits of a chosen position in one 64-bit word, its bit count prefix-summed over
//             the tile (scan256), the word ORed into an LDS image of the block; the image, header and trailer go to the
//             member's slot.  A stored block copies the text from where it came.
//   crc       cvi::crc_chunk / cvi::crc_fold of the inflater (64 pieces of 1 KiB), on a wave the codes phase leaves idle
#pragma once
#include <stdint.h>
#include <string.h>
#include "cv_inflate_core.hpp"

#define CVD_FN CVI_FN

#if defined(__HIP_DEVICE_COMPILE__)
#define CVD_ALL(...) do { const int tid = (int)threadIdx.x; __VA_ARGS__; __syncthreads(); } while (0)
#define CVD_MAX(p, v) atomicMax((p), (v))
#define CVD_ADD(p, v) atomicAdd((p), (v))
#define CVD_OR(p, v) atomicOr((p), (v))
#else
#define CVD_ALL(...) do { for (int tid = 0; tid < cvd::THREADS; ++tid) { __VA_ARGS__; } } while (0)
#define CVD_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define CVD_ADD(p, v) (*(p) += (v))
#define CVD_OR(p, v) (*(p) |= (v))
#endif

namespace cvd {

constexpr int THREADS = 256;                  // the workgroup, and the positions of one tile
constexpr uint32_t BLOCK_MAX = 65280, SLOT = 65536, WINDOW = 32768, TOO_FAR = 4096;
constexpr uint32_t MIN_MATCH = 3, MAX_MATCH = 258;
constexpr int HASH_BITS = 14;
constexpr int NLIT = 286, NDIST = 30, NCL = 19, LIT_LIMIT = 15, CL_LIMIT = 7;
constexpr uint32_t MEMBER_AT = 14;            // the member starts here in its slot: its DEFLATE data is then 4-byte aligned
constexpr uint32_t HEAD = 18, TAIL = 8;
constexpr uint32_t OUT_WORDS = (BLOCK_MAX + 5) / 4 + 4;
constexpr uint32_t MATCH = 0x80000000u;       // a verdict: MATCH | (length - 3) << 16 | (distance - 1), or the literal byte
enum : int { B_STORED = 0, B_FIXED = 1, B_DYNAMIC = 2 };

static_assert(MEMBER_AT + HEAD + 5 + BLOCK_MAX + TAIL <= SLOT, "a stored member fits its slot");

struct tree_scratch {
    uint32_t weight[2 * NLIT];
    uint16_t parent[2 * NLIT];               // later: the depth
    uint16_t order[NLIT];                    // the used symbols, lightest first
    uint16_t count[16], next[16];
};

struct state {
    union {
        struct { uint8_t text[65536]; uint32_t hash[1 << HASH_BITS]; } m;
        uint16_t step[65536];
        uint32_t out[OUT_WORDS];
    } u;
    uint32_t chosen[2048];                   // one bit per position
    uint32_t freq[NLIT + NDIST], wt[NLIT + NDIST];
    uint16_t code[NLIT + NDIST];             // bit-reversed, as DEFLATE sends them
    uint8_t len[NLIT + NDIST + 4];
    uint32_t clfreq[NCL];
    uint16_t clcode[NCL];
    uint8_t cllen[NCL + 1];
    uint16_t rle[NLIT + NDIST];              // symbol | extra << 8
    tree_scratch ts[2];
    uint64_t bits[THREADS];
    uint32_t scan[THREADS], wsum[THREADS / 64], total;
    uint32_t crc_table[256], crc_part[cvi::LANES];
    uint32_t base[2], nused[2];
    int32_t hlit, hdist, hclen, nrle, kind;
    uint32_t head_bits, body_bytes, crc, size;
};
static_assert(sizeof(state) <= 160 * 1024, "one workgroup per CU: the state is the CU's LDS");

CVD_FN uint32_t log2u(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

// length 3 .. 258 -> index of its code (symbol 257 + index), extra bits and their value
CVD_FN void len_code(uint32_t len, uint32_t *idx, uint32_t *eb, uint32_t *ev)
{
    const uint32_t l = len - 3;
    if (l < 8) { *idx = l; *eb = 0; *ev = 0; return; }
    if (len == 258) { *idx = 28; *eb = 0; *ev = 0; return; }
    const uint32_t e = log2u(l) - 2;
    *idx = 4 * e + 4 + ((l >> e) & 3); *eb = e; *ev = l & ((1u << e) - 1);
}

// distance 1 .. 32 768 -> its code, extra bits and their value
CVD_FN void dist_code(uint32_t dist, uint32_t *idx, uint32_t *eb, uint32_t *ev)
{
    const uint32_t d = dist - 1;
    if (d < 4) { *idx = d; *eb = 0; *ev = 0; return; }
    const uint32_t k = log2u(d), e = k - 1;
    *idx = 2 * k + ((d >> e) & 1); *eb = e; *ev = d & ((1u << e) - 1);
}

CVD_FN uint32_t len_extra(uint32_t idx) { return idx < 8 || idx == 28 ? 0 : (idx - 4) / 4; }
CVD_FN uint32_t dist_extra(uint32_t idx) { return idx < 4 ? 0 : (idx - 2) / 2; }
CVD_FN uint32_t fixed_len(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

CVD_FN uint32_t reverse_bits(uint32_t c, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t k = 0; k < n; k++) r |= ((c >> k) & 1) << (n - 1 - k);
    return r;
}

CVD_FN uint32_t load32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// bytes text[a ...] and text[b ...] share, at most maxl (b < a; four readable bytes lie behind every compared one)
CVD_FN uint32_t match_len(const uint8_t *t, uint32_t a, uint32_t b, uint32_t maxl)
{
    uint32_t l = 0;
    while (l + 4 <= maxl) {
        const uint32_t x = load32(t + a + l) ^ load32(t + b + l);
        if (x) return l + ((uint32_t)__builtin_ctz(x) >> 3);
        l += 4;
    }
    while (l < maxl && t[a + l] == t[b + l]) l++;
    return l;
}

CVD_FN uint32_t hash3(const uint8_t *t, uint32_t i) { return ((load32(t + i) & 0xffffffu) * 2654435761u) >> (32 - HASH_BITS); }

// the verdict of position i: the table holds positions of earlier tiles only
CVD_FN uint32_t find_match(const state &S, uint32_t i, uint32_t n)
{
    const uint8_t *t = S.u.m.text;
    const uint32_t maxl = n - i < MAX_MATCH ? n - i : MAX_MATCH;
    if (maxl < MIN_MATCH) return t[i];
    uint32_t best = 0, dist = 0;
    const uint32_t close_by[5] = {1, 2, 3, 4, 8};
    for (int k = 0; k < 5 && best < maxl; k++) {
        const uint32_t d = close_by[k];
        if (d > i || t[i] != t[i - d]) continue;
        const uint32_t l = match_len(t, i, i - d, maxl);
        if (l > best) { best = l; dist = d; }
    }
    const uint32_t c = S.u.m.hash[hash3(t, i)];
    if (c && best < maxl) {
        const uint32_t d = i - (c - 1);
        if (d <= WINDOW) {
            const uint32_t l = match_len(t, i, c - 1, maxl);
            if (l > best) { best = l; dist = d; }
        }
    }
    if (best < MIN_MATCH || (best == MIN_MATCH && dist > TOO_FAR)) return t[i];
    return MATCH | (best - MIN_MATCH) << 16 | (dist - 1);
}

// ONE lane: code lengths of at most `limit` bits for the m >= 2 symbols T.order[0, m) (lightest first) -> len[], the
// others 0; T.count[d] = codes of d bits.  Two queues: the sorted leaves and the inner nodes, which are made in ascending
// weight.  A tree deeper than the limit is cut off there and codes are moved one bit down until the Kraft sum is 1.
CVD_FN void build_lengths(const uint32_t *wt, int nsym, int m, int limit, uint8_t *len, tree_scratch &T)
{
    for (int s = 0; s < nsym; s++) len[s] = 0;
    for (int k = 0; k < m; k++) T.weight[k] = wt[T.order[k]];
    int a = 0, b = m;
    for (int nx = m; nx <= 2 * m - 2; nx++) {
        uint32_t w = 0;
        for (int pick = 0; pick < 2; pick++) {
            const int x = a < m && (b >= nx || T.weight[a] <= T.weight[b]) ? a++ : b++;
            w += T.weight[x];
            T.parent[x] = (uint16_t)nx;
        }
        T.weight[nx] = w;
    }
    T.parent[2 * m - 2] = 0;
    for (int k = 2 * m - 3; k >= 0; k--) T.parent[k] = (uint16_t)(T.parent[T.parent[k]] + 1);
    for (int d = 0; d < 16; d++) T.count[d] = 0;
    uint32_t kraft = 0;
    for (int k = 0; k < m; k++) {
        const int d = T.parent[k] < limit ? T.parent[k] : limit;
        T.count[d]++;
        kraft += 1u << (limit - d);
    }
    while (kraft > (1u << limit)) {
        T.count[limit]--;
        for (int d = limit - 1; d > 0; d--)
            if (T.count[d]) { T.count[d]--; T.count[d + 1] += 2; break; }
        kraft--;
    }
    int k = 0;
    for (int d = limit; d > 0; d--)
        for (int c = 0; c < T.count[d]; c++) len[T.order[k++]] = (uint8_t)d;
}

// ONE lane: the canonical codes of len[] (T.count from build_lengths), bit-reversed
CVD_FN void assign_codes(const uint8_t *len, int nsym, uint16_t *code, tree_scratch &T)
{
    uint32_t c = 0;
    T.next[0] = 0;
    for (int d = 1; d < 16; d++) { c = (c + T.count[d - 1]) << 1; T.next[d] = (uint16_t)c; }
    for (int s = 0; s < nsym; s++) code[s] = len[s] ? (uint16_t)reverse_bits(T.next[len[s]]++, len[s]) : 0;
}

// ONE lane: the used symbols of wt[0, nsym) into T.order, lightest first, the lower symbol first among equals -> how many
CVD_FN int sort_used(const uint32_t *wt, int nsym, tree_scratch &T)
{
    int m = 0;
    for (int s = 0; s < nsym; s++) {
        if (!wt[s]) continue;
        int k = m++;
        for (; k > 0 && wt[T.order[k - 1]] > wt[s]; k--) T.order[k] = T.order[k - 1];
        T.order[k] = (uint16_t)s;
    }
    return m;
}

// every lane: the place of symbol s among the used ones of its alphabet wt[0, nsym) (sort_used's order, as a rank)
CVD_FN void rank_symbol(const uint32_t *wt, int nsym, int s, tree_scratch &T)
{
    const uint32_t w = wt[s];
    if (!w) return;
    int r = 0;
    for (int o = 0; o < nsym; o++) r += wt[o] && (wt[o] < w || (wt[o] == w && o < s));
    T.order[r] = (uint16_t)s;
}

// ONE lane: an alphabet with fewer than two used symbols gets symbol 0 (or 1) beside it, weight 1
CVD_FN void two_at_least(uint32_t *wt, uint32_t *nused)
{
    for (int s = 0; *nused < 2; s++)
        if (!wt[s]) { wt[s] = 1; ++*nused; }
}

CVD_FN uint32_t seq_len(const state &S, int j) { return j < S.hlit ? S.len[j] : S.len[NLIT + j - S.hlit]; }

CVD_FN void rle_put(state &S, uint32_t sym, uint32_t extra)
{
    S.rle[S.nrle++] = (uint16_t)(sym | extra << 8);
    S.clfreq[sym]++;
}

// ONE lane: bits [at, at + n) of the image (n <= 32; nobody else writes yet)
CVD_FN uint32_t put_bits(state &S, uint32_t at, uint32_t v, uint32_t n)
{
    const uint64_t x = (uint64_t)v << (at & 31);
    S.u.out[at >> 5] |= (uint32_t)x;
    if (x >> 32) S.u.out[(at >> 5) + 1] |= (uint32_t)(x >> 32);
    return at + n;
}

// every lane: the (at most 48) bits of v ORed in at `at`
CVD_FN void or_bits(state &S, uint32_t at, uint64_t v)
{
    if (!v) return;
    const uint32_t w = at >> 5, sh = at & 31;
    const uint64_t x = v << sh;
    const uint32_t lo = (uint32_t)x, mid = (uint32_t)(x >> 32), hi = sh ? (uint32_t)(v >> (64 - sh)) : 0;
    if (lo) CVD_OR(&S.u.out[w], lo);
    if (mid) CVD_OR(&S.u.out[w + 1], mid);
    if (hi) CVD_OR(&S.u.out[w + 2], hi);
}

CVD_FN bool is_chosen(const state &S, uint32_t i) { return (S.chosen[i >> 5] >> (i & 31)) & 1; }

// ONE lane, after the codes of both alphabets: the header's RLE and its code, the costs, the choice, the header's bits
CVD_FN void choose_and_head(state &S, uint32_t n)
{
    S.hlit = NLIT; S.hdist = NDIST;
    while (S.hlit > 257 && !S.len[S.hlit - 1]) S.hlit--;
    while (S.hdist > 1 && !S.len[NLIT + S.hdist - 1]) S.hdist--;
    for (int s = 0; s < NCL; s++) S.clfreq[s] = 0;
    S.nrle = 0;
    const int tot = S.hlit + S.hdist;
    for (int j = 0; j < tot;) {
        const uint32_t v = seq_len(S, j);
        int run = 1;
        while (j + run < tot && seq_len(S, j + run) == v) run++;
        j += run;
        if (v == 0) {
            while (run >= 11) { const int r = run < 138 ? run : 138; rle_put(S, 18, (uint32_t)(r - 11)); run -= r; }
            if (run >= 3) { rle_put(S, 17, (uint32_t)(run - 3)); run = 0; }
        } else {
            rle_put(S, v, 0); run--;
            while (run >= 3) { const int r = run < 6 ? run : 6; rle_put(S, 16, (uint32_t)(r - 3)); run -= r; }
        }
        while (run-- > 0) rle_put(S, v, 0);
    }
    tree_scratch &T = S.ts[0];
    uint32_t clwt[NCL], used = 0;
    for (int s = 0; s < NCL; s++) { clwt[s] = S.clfreq[s]; used += clwt[s] != 0; }
    two_at_least(clwt, &used);
    build_lengths(clwt, NCL, sort_used(clwt, NCL, T), CL_LIMIT, S.cllen, T);
    assign_codes(S.cllen, NCL, S.clcode, T);
    const uint8_t order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    S.hclen = NCL;
    while (S.hclen > 4 && !S.cllen[order[S.hclen - 1]]) S.hclen--;
    uint32_t dyn = 3 + 14 + 3 * (uint32_t)S.hclen, fix = 3;
    for (int s = 0; s < NCL; s++) dyn += S.clfreq[s] * (S.cllen[s] + (s == 16 ? 2u : s == 17 ? 3u : s == 18 ? 7u : 0u));
    const uint32_t head = dyn;
    for (uint32_t s = 0; s < (uint32_t)NLIT; s++) {
        const uint32_t e = s > 256 ? len_extra(s - 257) : 0;
        dyn += S.freq[s] * (S.len[s] + e);
        fix += S.freq[s] * (fixed_len(s) + e);
    }
    for (uint32_t s = 0; s < (uint32_t)NDIST; s++) {
        dyn += S.freq[NLIT + s] * (S.len[NLIT + s] + dist_extra(s));
        fix += S.freq[NLIT + s] * (5 + dist_extra(s));
    }
    const uint32_t dyn_bytes = (dyn + 7) / 8, fix_bytes = (fix + 7) / 8, stored_bytes = n + 5;
    S.kind = dyn_bytes < fix_bytes && dyn_bytes < stored_bytes ? B_DYNAMIC : fix_bytes < stored_bytes ? B_FIXED : B_STORED;
    S.body_bytes = S.kind == B_DYNAMIC ? dyn_bytes : S.kind == B_FIXED ? fix_bytes : stored_bytes;
    if (S.kind == B_FIXED) {
        for (uint32_t s = 0; s < (uint32_t)NLIT; s++) {
            S.len[s] = (uint8_t)fixed_len(s);
            const uint32_t c = s < 144 ? 0x30 + s : s < 256 ? 0x190 + s - 144 : s < 280 ? s - 256 : 0xc0 + s - 280;
            S.code[s] = (uint16_t)reverse_bits(c, S.len[s]);
        }
        for (uint32_t s = 0; s < (uint32_t)NDIST; s++) { S.len[NLIT + s] = 5; S.code[NLIT + s] = (uint16_t)reverse_bits(s, 5); }
        S.head_bits = put_bits(S, 0, 3, 3);
    } else if (S.kind == B_DYNAMIC) {
        uint32_t at = put_bits(S, 0, 5, 3);
        at = put_bits(S, at, (uint32_t)(S.hlit - 257), 5);
        at = put_bits(S, at, (uint32_t)(S.hdist - 1), 5);
        at = put_bits(S, at, (uint32_t)(S.hclen - 4), 4);
        for (int k = 0; k < S.hclen; k++) at = put_bits(S, at, S.cllen[order[k]], 3);
        for (int k = 0; k < S.nrle; k++) {
            const uint32_t s = S.rle[k] & 0xff, x = S.rle[k] >> 8;
            at = put_bits(S, at, S.clcode[s], S.cllen[s]);
            if (s >= 16) at = put_bits(S, at, x, s == 16 ? 2 : s == 17 ? 3 : 7);
        }
        S.head_bits = at;                        // == head
        (void)head;
    }
    S.base[0] = S.head_bits;
}

// every lane: the word and bit count of position i (nothing for a position the parse skips)
CVD_FN uint64_t symbol_bits(const state &S, uint32_t e, uint32_t *nbits)
{
    if (!(e & MATCH)) { *nbits = S.len[e & 0xff]; return S.code[e & 0xff]; }
    uint32_t li, le, lv, di, de, dv;
    len_code(((e >> 16) & 0xff) + MIN_MATCH, &li, &le, &lv);
    dist_code((e & 0xffff) + 1, &di, &de, &dv);
    uint64_t v = S.code[257 + li];
    uint32_t at = S.len[257 + li];
    v |= (uint64_t)lv << at; at += le;
    v |= (uint64_t)S.code[NLIT + di] << at; at += S.len[NLIT + di];
    v |= (uint64_t)dv << at; at += de;
    *nbits = at;
    return v;
}

// the exclusive sum of S.scan[0, THREADS) in place, the sum of all in S.total (called by all, between phases)
CVD_FN void scan256(state &S)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t v = S.scan[tid];
    uint32_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) S.wsum[w] = x;
    __syncthreads();
    uint32_t add = 0;
    for (int k = 0; k < w; k++) add += S.wsum[k];
    S.scan[tid] = add + x - v;
    if (tid == THREADS - 1) S.total = add + x;
    __syncthreads();
#else
    uint32_t run = 0;
    for (int t = 0; t < THREADS; t++) { const uint32_t v = S.scan[t]; S.scan[t] = run; run += v; }
    S.total = run;
#endif
}

CVD_FN void store16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
CVD_FN void store32(uint8_t *p, uint32_t v) { store16(p, v); store16(p + 2, v >> 16); }

// One member: src[0, n) -> the member at slot + MEMBER_AT (slot: SLOT bytes, 4-byte aligned); ent[0, n) = the caller's
// room for the verdicts.  Called by all THREADS (on the host: once).  S.size = the member's bytes, S.kind its block type.
CVD_FN void member(state &S, const uint8_t *src, uint32_t n, uint32_t *ent, uint8_t *slot, const cvi::crc_consts &C)
{
    const uint32_t tiles = (n + THREADS - 1) / THREADS;
    CVD_ALL({
        for (uint32_t i = (uint32_t)tid; i < n + 8; i += THREADS) S.u.m.text[i] = i < n ? src[i] : 0;
        for (uint32_t k = (uint32_t)tid; k < (1u << HASH_BITS); k += THREADS) S.u.m.hash[k] = 0;
        for (uint32_t k = (uint32_t)tid; k < 2048; k += THREADS) S.chosen[k] = 0;
        for (uint32_t k = (uint32_t)tid; k < (uint32_t)(NLIT + NDIST); k += THREADS) S.freq[k] = 0;
        S.crc_table[tid] = cvi::crc_byte_table((uint32_t)tid);
        if (tid < 2) S.nused[tid] = 0;
    });
    for (uint32_t t = 0; t < tiles; t++) {
        CVD_ALL({
            const uint32_t i = t * THREADS + (uint32_t)tid;
            if (i < n) ent[i] = find_match(S, i, n);
        });
        CVD_ALL({
            const uint32_t i = t * THREADS + (uint32_t)tid;
            if (i + MIN_MATCH <= n) CVD_MAX(&S.u.m.hash[hash3(S.u.m.text, i)], i + 1);
        });
    }
    // the CRC while the text is still here (the wave's lanes each take 1 KiB), before the steps take its place
    CVD_ALL({
        if (tid < cvi::LANES) S.crc_part[tid] = cvi::crc_chunk(S.u.m.text, n, tid, S.crc_table);
    });
    CVD_ALL({
        for (uint32_t i = (uint32_t)tid; i < n; i += THREADS) {
            const uint32_t e = ent[i];
            S.u.step[i] = (uint16_t)(e & MATCH ? ((e >> 16) & 0xff) + MIN_MATCH : 1);
        }
    });
    CVD_ALL({
        if (tid == 0) {
            uint32_t cur = 0, w = 0;
            for (uint32_t i = 0; i < n; i += S.u.step[i] ? S.u.step[i] : 1) {    // (a step is never 0: the loop ends whatever it reads)
                if (i >> 5 != cur) { S.chosen[cur] = w; w = 0; cur = i >> 5; }
                w |= 1u << (i & 31);
            }
            S.chosen[cur] = w;
            S.freq[256] = 1;
        }
        if (tid == 64) S.crc = cvi::crc_fold(S.crc_part, n, C);
    });
    CVD_ALL({
        for (uint32_t k = (uint32_t)tid; k < OUT_WORDS; k += THREADS) S.u.out[k] = 0;       // (the steps are done with)
        for (uint32_t i = (uint32_t)tid; i < n; i += THREADS) {
            if (!is_chosen(S, i)) continue;
            const uint32_t e = ent[i];
            if (!(e & MATCH)) { CVD_ADD(&S.freq[e & 0xff], 1u); continue; }
            uint32_t idx, eb, ev;
            len_code(((e >> 16) & 0xff) + MIN_MATCH, &idx, &eb, &ev);
            CVD_ADD(&S.freq[257 + idx], 1u);
            dist_code((e & 0xffff) + 1, &idx, &eb, &ev);
            CVD_ADD(&S.freq[NLIT + idx], 1u);
        }
    });
    CVD_ALL({
        for (int s = tid; s < NLIT + NDIST; s += THREADS) {
            S.wt[s] = S.freq[s];
            if (S.freq[s]) CVD_ADD(&S.nused[s < NLIT ? 0 : 1], 1u);
        }
    });
    CVD_ALL({
        if (tid == 0) two_at_least(S.wt, &S.nused[0]);
        if (tid == 64) two_at_least(S.wt + NLIT, &S.nused[1]);
    });
    CVD_ALL({
        for (int s = tid; s < NLIT + NDIST; s += THREADS) {
            if (s < NLIT) rank_symbol(S.wt, NLIT, s, S.ts[0]);
            else rank_symbol(S.wt + NLIT, NDIST, s - NLIT, S.ts[1]);
        }
    });
    CVD_ALL({
        if (tid == 0) {
            build_lengths(S.wt, NLIT, (int)S.nused[0], LIT_LIMIT, S.len, S.ts[0]);
            assign_codes(S.len, NLIT, S.code, S.ts[0]);
        }
        if (tid == 64) {
            build_lengths(S.wt + NLIT, NDIST, (int)S.nused[1], LIT_LIMIT, S.len + NLIT, S.ts[1]);
            assign_codes(S.len + NLIT, NDIST, S.code + NLIT, S.ts[1]);
        }
    });
    CVD_ALL({
        if (tid == 0) choose_and_head(S, n);
    });
    uint8_t *mem = slot + MEMBER_AT, *body = mem + HEAD;
    if (S.kind != B_STORED) {
        for (uint32_t t = 0; t < tiles; t++) {
            CVD_ALL({
                const uint32_t i = t * THREADS + (uint32_t)tid;
                uint32_t nb = 0;
                uint64_t v = 0;
                if (i < n && is_chosen(S, i)) v = symbol_bits(S, ent[i], &nb);
                S.bits[tid] = v;
                S.scan[tid] = nb;
            });
            scan256(S);
            CVD_ALL({
                or_bits(S, S.base[t & 1] + S.scan[tid], S.bits[tid]);
                if (tid == 0) S.base[(t + 1) & 1] = S.base[t & 1] + S.total;
            });
        }
        CVD_ALL({
            if (tid == 0) or_bits(S, S.base[tiles & 1], S.code[256]);
        });
        CVD_ALL({
            uint32_t *body32 = reinterpret_cast<uint32_t *>(body);
            const uint32_t words = S.body_bytes / 4;
            for (uint32_t k = (uint32_t)tid; k < words; k += THREADS) body32[k] = S.u.out[k];
            if (tid == 0)
                for (uint32_t k = words * 4; k < S.body_bytes; k++) body[k] = (uint8_t)(S.u.out[k >> 2] >> (8 * (k & 3)));
        });
    } else {
        CVD_ALL({
            if (tid == 0) { body[0] = 1; store16(body + 1, n); store16(body + 3, ~n); }
            for (uint32_t i = (uint32_t)tid; i < n; i += THREADS) body[5 + i] = src[i];
        });
    }
    CVD_ALL({
        if (tid == 0) {
            const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
            S.size = HEAD + S.body_bytes + TAIL;
            for (int k = 0; k < 16; k++) mem[k] = head[k];
            store16(mem + 16, S.size - 1);
            store32(body + S.body_bytes, S.crc);
            store32(body + S.body_bytes + 4, n);
        }
    });
}

// members of a text of `len` bytes cut every `block`: an empty text is one empty member
CVD_FN int64_t members_of(int64_t len, int64_t block) { return len <= 0 ? 1 : (len + block - 1) / block; }

// The host form: the members of text[0, len) back to back into out[0, out_cap) -- nothing of a member that does not fit
// --, sizes[k] the bytes of member k, info[8] = {bytes of all, members, stored, fixed, dynamic, 0 ...}
inline void deflate_host_form(const uint8_t *text, int64_t len, int64_t block, uint8_t *out, int64_t out_cap, int32_t *sizes, int64_t *info)
{
    static const cvi::crc_consts C = [] { cvi::crc_consts c; cvi::make_crc_consts(&c); return c; }();
    state *S = new state;
    uint32_t *ent = new uint32_t[BLOCK_MAX];
    uint8_t *slot = new uint8_t[SLOT];
    const int64_t members = members_of(len, block);
    for (int k = 0; k < 8; k++) info[k] = 0;
    info[1] = members;
    for (int64_t m = 0; m < members; m++) {
        const int64_t lo = m * block, n = len - lo < block ? len - lo : block;
        member(*S, text + lo, (uint32_t)(n < 0 ? 0 : n), ent, slot, C);
        sizes[m] = (int32_t)S->size;
        info[2 + S->kind]++;
        if ((int64_t)S->size <= out_cap - info[0]) memcpy(out + info[0], slot + MEMBER_AT, S->size);
        info[0] += S->size;
    }
    delete[] slot;
    delete[] ent;
    delete S;
}

}  // namespace cvd
