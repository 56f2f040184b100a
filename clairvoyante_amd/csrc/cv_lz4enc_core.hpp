// cv_lz4enc_core.hpp -- the encode core of the .bin block writer on the device (cv_blosc_pack_dev.hip): ONE stream of a
// c-blosc chunk -- a byte plane of a split block, or an unsplit block -- written as one LZ4 block by one wave, and the
// geometry of the chunk (which streams it has, where each stream's bytes come from, where they go).  Written like
// cv_lz4_core.hpp: the SAME text compiles for the device (64 lanes, a barrier behind every CVE_LANES group) and for the
// host (the lane loop written out), so tests/native/lz4enc_core_driver.cpp runs it under AddressSanitizer / UBSan and
// the kernel is held to the host form byte for byte.
//
// Nothing is materialised: byte i of a stream is read where it lies, through the chunk's virtual buffer
// head | data | tail (the pickle envelope around the rows in HBM) and c-blosc's shuffle rule (shuffle_bytes of
// cv_hostio.cpp: bsize / ts whole elements plane by plane, the remainder unshuffled behind them).
//
// One step of encode() takes the next 64 positions:
//   load     the bytes [pos - BACK, pos + 64 + 3) into the window in LDS
//   find     every lane hashes its 4 bytes, reads the position the table held BEFORE this step and checks it against the
//            stream; it also tries the distances 1..NEAR, which the table cannot know yet inside a step (distance 1 is
//            the zero runs of pileup planes).  The lowest lane with a verified match wins (an LDS atomic min)
//   insert   the lanes up to the winner put their positions into the table with an atomic max.  Positions behind the
//            winner are NOT inserted, so the table never holds a position at or behind the next step's: a candidate is
//            always strictly in front of the position it is offered to (and is checked to be)
//   extend   the wave compares 64 bytes at a time; of the winner's two candidates the longer match is taken
//   emit     token, length bytes, literals, offset: checked against the cap BEFORE anything is written
// Every value that steers the wave (the winner, where a match stops) is a min or a max over the lanes, so the result
// does not depend on lane timing: the device and the host form write the same bytes.
//
// What the output obeys (the STRICT decoder of cv_lz4_core.hpp takes it): the last sequence is literals only and holds
// at least the last 5 bytes; no match starts within the last 12 bytes; distances are 1..65 535 and never reach in front
// of the stream; a stream of fewer than 13 bytes is literals only.  encode() writes at most `cap` bytes; 0 = the block
// does not fit into cap bytes (the caller stores the stream raw).  Each step consumes input or ends.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVE_FN __host__ __device__ inline
#else
#define CVE_FN inline
#endif

// all lanes run the group, then meet; the host form runs the lanes one after the other
#if defined(__HIP_DEVICE_COMPILE__)
#define CVE_LANES(...) { const int lane = lane_; __VA_ARGS__ } __syncthreads();
#define CVE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define CVE_MIN(x, v) atomicMin(&(x), (uint32_t)(v))
#define CVE_MAX(x, v) atomicMax(&(x), (uint32_t)(v))
#else
#define CVE_LANES(...) for (int lane = 0; lane < LANES; lane++) { __VA_ARGS__ }
#define CVE_UNIFORM(x) ((uint32_t)(x))
#define CVE_MIN(x, v) do { if ((uint32_t)(v) < (x)) (x) = (uint32_t)(v); } while (0)
#define CVE_MAX(x, v) do { if ((uint32_t)(v) > (x)) (x) = (uint32_t)(v); } while (0)
#endif

namespace cve {

constexpr int LANES = 64;
constexpr int HASH_BITS = 12;
constexpr int HASH_SIZE = 1 << HASH_BITS;
constexpr uint32_t STREAM_CAP = 65535;   // bytes of a stream the core takes: every distance inside one fits 16 bits
constexpr uint32_t EXTEND = 1;           // bytes a lane compares per step of a match's extension
constexpr int BACK = 8, NEAR = 4;        // bytes of the window behind the step; distances tried inside the step
constexpr int WIN = BACK + LANES + 3;
constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t MAX_DISTANCE = 65535;
constexpr int32_t ST_OK = 1, ST_HOST = 2;           // per chunk (CV_BLOSC_OK / CV_BLOSC_HOST)
constexpr uint32_t ENVELOPE_MAX = 2048;             // bytes of head and of tail

// where a stream's bytes lie: the shuffled form of the block [base, base + bsize) of the virtual buffer, from `first` on
struct source {
    const uint8_t *head, *data, *tail;
    uint32_t head_len, data_len, tail_len;
    uint32_t base, ne, ts, first;
    int32_t plane;                       // >= 0: the stream is this byte plane of a split block (no division per byte)
};

CVE_FN uint8_t vbyte(const source &s, uint32_t vb)
{
    if (vb < s.head_len) return s.head[vb];
    vb -= s.head_len;
    if (vb < s.data_len) return s.data[vb];
    return s.tail[vb - s.data_len];
}

CVE_FN uint8_t byte(const source &s, uint32_t i)
{
    if (s.plane >= 0) return vbyte(s, s.base + i * s.ts + (uint32_t)s.plane);
    const uint32_t q = s.first + i;
    if (q < s.ne * s.ts) {
        const uint32_t j = q / s.ne;
        return vbyte(s, s.base + (q - j * s.ne) * s.ts + j);
    }
    return vbyte(s, s.base + q);
}

struct state {
    uint32_t table[HASH_SIZE];           // position + 1 of the latest insert per hash; 0 = none
    uint32_t cand[LANES];                // per lane: the table's position, verified, or NONE
    uint32_t winner, stop;
    uint16_t hash[LANES];                // per lane: its hash, 0xffff = the lane has no position to offer
    uint8_t near_[LANES];                // per lane: the smallest distance 1..NEAR that matches, 0 = none
    uint8_t win[WIN + 1];
};

CVE_FN uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HASH_BITS); }

// bytes of a length field behind its nibble
CVE_FN uint32_t length_bytes(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }

// the wave: how far the match of `mpos` against `cp` (< mpos) goes, 4 <= result <= maxml (the first 4 bytes are known)
CVE_FN uint32_t extend(state &S, const source &src, uint32_t mpos, uint32_t cp, uint32_t maxml, int lane_)
{
    (void)lane_;
    uint32_t ml = 4;
    for (;;) {
        CVE_LANES(if (lane == 0) S.stop = NONE;)
        CVE_LANES(
            for (uint32_t k = ml + EXTEND * (uint32_t)lane, e = k + EXTEND; k < e; k++)
                if (k >= maxml || byte(src, cp + k) != byte(src, mpos + k)) { CVE_MIN(S.stop, k); break; }
        )
        const uint32_t stop = CVE_UNIFORM(S.stop);
        if (stop != NONE) return stop < maxml ? stop : maxml;
        ml += EXTEND * LANES;
    }
}

// the wave: one sequence at out[op...] -- `litlen` literals from `anchor`, then a match (ml >= 4) or, ml == 0, nothing.
// The caller has checked the room.  -> the new op
CVE_FN uint32_t emit(const source &src, uint8_t *out, uint32_t op, uint32_t anchor, uint32_t litlen, uint32_t ml, uint32_t dist, int lane_)
{
    (void)lane_;
    const uint32_t nl = length_bytes(litlen), mcode = ml ? ml - 4 : 0, nm = ml ? length_bytes(mcode) : 0;
    const uint32_t lit_at = op + 1 + nl, off_at = lit_at + litlen, end = ml ? off_at + 2 + nm : off_at;
    CVE_LANES(
        if (lane == 0) {
            out[op] = (uint8_t)(((litlen < 15 ? litlen : 15) << 4) | (mcode < 15 ? mcode : 15));
            if (ml) { out[off_at] = (uint8_t)(dist & 255); out[off_at + 1] = (uint8_t)(dist >> 8); }
        }
        for (uint32_t j = (uint32_t)lane; j < nl; j += LANES) out[op + 1 + j] = j + 1 < nl ? 255 : (uint8_t)((litlen - 15) % 255);
        for (uint32_t j = (uint32_t)lane; j < nm; j += LANES) out[off_at + 2 + j] = j + 1 < nm ? 255 : (uint8_t)((mcode - 15) % 255);
        for (uint32_t k = (uint32_t)lane; k < litlen; k += LANES) out[lit_at + k] = byte(src, anchor + k);
    )
    return end;
}

// the wave: the stream src[0, n) as one LZ4 block into out[0, cap) -> its length, 0 = it does not fit (nothing of use
// written; never a byte at or behind out[cap]).  n <= STREAM_CAP.
CVE_FN uint32_t encode(state &S, const source &src, uint32_t n, uint8_t *out, uint32_t cap, int lane_)
{
    (void)lane_;
    if (n == 0 || n > STREAM_CAP) return 0;
    uint32_t op = 0, anchor = 0, pos = 0;
    const uint32_t mflimit = n >= 13 ? n - 12 : 0;          // no match starts at or behind it
    if (mflimit) { CVE_LANES(for (int i = lane; i < HASH_SIZE; i += LANES) S.table[i] = 0;) }
    while (pos < mflimit) {
        CVE_LANES(
            for (int k = lane; k < WIN; k += LANES) {
                const int64_t at = (int64_t)pos + k - BACK;
                S.win[k] = at >= 0 && at < (int64_t)n ? byte(src, (uint32_t)at) : 0;
            }
            if (lane == 0) S.winner = LANES;
        )
        CVE_LANES(
            const uint32_t my = pos + (uint32_t)lane;
            uint32_t c = NONE, d = 0, h = 0xffff;
            if (my < mflimit) {
                const uint8_t *w = S.win + BACK + lane;
                const uint32_t v = (uint32_t)w[0] | ((uint32_t)w[1] << 8) | ((uint32_t)w[2] << 16) | ((uint32_t)w[3] << 24);
                h = hash4(v);
                for (uint32_t dd = 1; dd <= (uint32_t)NEAR && dd <= my; dd++)
                    if (w[0] == *(w - dd) && w[1] == *(w + 1 - dd) && w[2] == *(w + 2 - dd) && w[3] == *(w + 3 - dd)) { d = dd; break; }
                const uint32_t t = S.table[h];
                if (t) {
                    const uint32_t cp = t - 1;              // strictly in front of `my`, or it is no candidate
                    if (cp < my && my - cp <= MAX_DISTANCE && byte(src, cp) == w[0] && byte(src, cp + 1) == w[1] &&
                        byte(src, cp + 2) == w[2] && byte(src, cp + 3) == w[3])
                        c = cp;
                }
                if (d || c != NONE) CVE_MIN(S.winner, lane);
            }
            S.cand[lane] = c; S.near_[lane] = (uint8_t)d; S.hash[lane] = (uint16_t)h;
        )
        const uint32_t wl = CVE_UNIFORM(S.winner);
        CVE_LANES(
            if ((uint32_t)lane <= wl && S.hash[lane] != 0xffff) CVE_MAX(S.table[S.hash[lane]], pos + (uint32_t)lane + 1);
        )
        if (wl >= (uint32_t)LANES) { pos += LANES; continue; }
        const uint32_t mpos = pos + wl, maxml = n - 5 - mpos;   // mpos < n - 12: maxml >= 8
        const uint32_t c = CVE_UNIFORM(S.cand[wl]), d = CVE_UNIFORM(S.near_[wl]);
        uint32_t ml = 0, dist = 0;
        if (d) { ml = extend(S, src, mpos, mpos - d, maxml, lane_); dist = d; }
        if (c != NONE && mpos - c != d) {
            const uint32_t m2 = extend(S, src, mpos, c, maxml, lane_);
            if (m2 > ml) { ml = m2; dist = mpos - c; }
        }
        const uint32_t litlen = mpos - anchor;
        const uint32_t need = 1 + length_bytes(litlen) + litlen + 2 + length_bytes(ml - 4);
        if (need > cap || op > cap - need) return 0;
        op = emit(src, out, op, anchor, litlen, ml, dist, lane_);
        pos = anchor = mpos + ml;
    }
    const uint32_t litlen = n - anchor;                         // >= 5, or all of a short stream
    const uint32_t need = 1 + length_bytes(litlen) + litlen;
    if (need > cap || op > cap - need) return 0;
    return emit(src, out, op, anchor, litlen, 0, 0, lane_);
}

// ---- the chunk ----------------------------------------------------------------------------
// c-blosc's cut of nbytes into blocks, by the rules of cv_blosc_compress_lz4_blocks: no block larger than the data, whole
// elements per block, a block of at least 128 elements that is not the leftover is split into ts planes.
struct geometry {
    uint32_t nbytes, ts, blocksize;      // (the blocksize the header names)
    uint32_t nfull, left, per_block;     // whole blocks, bytes of the leftover block, streams per whole block
    uint32_t nblocks, streams, slot;     // slot: bytes of the largest stream, rounded up to 16
};

// false = not a chunk the device writes (the host packs it)
CVE_FN bool make_geometry(int64_t nbytes, int64_t ts, int64_t blocksize, geometry &g)
{
    if (nbytes < 64 || nbytes > 0x7fffff00 || ts < 1 || ts > 16 || blocksize < ts || blocksize > 0x7fffff00) return false;
    if (blocksize > nbytes) blocksize = nbytes;
    if (blocksize > ts) blocksize = blocksize / ts * ts;
    g.nbytes = (uint32_t)nbytes; g.ts = (uint32_t)ts; g.blocksize = (uint32_t)blocksize;
    g.nfull = (uint32_t)(nbytes / blocksize); g.left = (uint32_t)(nbytes % blocksize);
    g.per_block = blocksize / ts >= 128 ? (uint32_t)ts : 1u;
    g.nblocks = g.nfull + (g.left ? 1u : 0u);
    const uint64_t streams = (uint64_t)g.nfull * g.per_block + (g.left ? 1u : 0u);
    if (streams > 0x7fffffffu) return false;
    g.streams = (uint32_t)streams;
    uint32_t big = g.blocksize / g.per_block;
    if (g.left > big) big = g.left;
    if (big > STREAM_CAP) return false;
    g.slot = (big + 15u) & ~15u;
    return true;
}

// stream s of the chunk: its source (the envelope and data pointers are the caller's), its length, its block and
// whether it is the first stream of that block
CVE_FN uint32_t stream_source(const geometry &g, uint32_t s, source &src, uint32_t *block, bool *first_of_block)
{
    const uint32_t split_streams = g.nfull * g.per_block;
    src.ts = g.ts; src.first = 0;
    if (s < split_streams) {
        const uint32_t b = s / g.per_block, p = s - b * g.per_block;
        *block = b; *first_of_block = p == 0;
        src.base = b * g.blocksize;
        src.ne = g.blocksize / g.ts;
        if (g.per_block == g.ts) { src.plane = (int32_t)p; return src.ne; }
        src.plane = -1;
        return g.blocksize;
    }
    *block = g.nfull; *first_of_block = true;
    src.base = g.nfull * g.blocksize;
    src.ne = g.left / g.ts;
    src.plane = -1;
    return g.left;
}

CVE_FN void put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// the 16-byte header of a chunk of `total` bytes
CVE_FN void put_header(const geometry &g, uint32_t total, uint8_t *dst)
{
    dst[0] = 2; dst[1] = 1; dst[2] = (uint8_t)((1 << 5) | (g.ts > 1 ? 1 : 0)); dst[3] = (uint8_t)g.ts;
    put32(dst + 4, g.nbytes); put32(dst + 8, g.blocksize); put32(dst + 12, total);
}

// The host form of one stream: encode() into a block of exactly cap bytes.
inline uint32_t encode_host(const source &src, uint32_t n, uint8_t *out, uint32_t cap)
{
    state *S = new state;
    const uint32_t c = encode(*S, src, n, out, cap, 0);
    delete S;
    return c;
}

// The host form of the chunk writer: head | data | tail of g.nbytes bytes -> the chunk the device writes, into
// out[0, g.nbytes + 16).  -> its length, 0 = HOST (the chunk does not shrink; nothing of use written).
inline uint32_t pack_chunk_host(const geometry &g, const uint8_t *head, uint32_t head_len, const uint8_t *data, uint32_t data_len,
                                const uint8_t *tail, uint32_t tail_len, uint8_t *out)
{
    if ((uint64_t)head_len + data_len + tail_len != g.nbytes) return 0;
    uint8_t **bufs = new uint8_t *[g.streams];
    uint32_t *lens = new uint32_t[g.streams];
    uint64_t total = 16 + 4 * (uint64_t)g.nblocks;
    for (uint32_t s = 0; s < g.streams; s++) {
        source src;
        src.head = head; src.data = data; src.tail = tail; src.head_len = head_len; src.data_len = data_len; src.tail_len = tail_len;
        uint32_t b; bool f;
        const uint32_t n = stream_source(g, s, src, &b, &f);
        bufs[s] = new uint8_t[n > 1 ? n - 1 : 1];       // (exactly the cap: one byte more is a sanitizer report)
        const uint32_t c = encode_host(src, n, bufs[s], n - 1);
        lens[s] = c ? c : n;
        total += 4 + lens[s];
    }
    const bool ok = total < 16 + (uint64_t)g.nbytes;
    if (ok) {
        put_header(g, (uint32_t)total, out);
        uint32_t op = 16 + 4 * g.nblocks;
        for (uint32_t s = 0; s < g.streams; s++) {
            source src;
            src.head = head; src.data = data; src.tail = tail; src.head_len = head_len; src.data_len = data_len; src.tail_len = tail_len;
            uint32_t b; bool f;
            const uint32_t n = stream_source(g, s, src, &b, &f);
            if (f) put32(out + 16 + 4 * b, op);
            put32(out + op, lens[s]);
            if (lens[s] == n) for (uint32_t k = 0; k < n; k++) out[op + 4 + k] = byte(src, k);
            else for (uint32_t k = 0; k < lens[s]; k++) out[op + 4 + k] = bufs[s][k];
            op += 4 + lens[s];
        }
    }
    for (uint32_t s = 0; s < g.streams; s++) delete[] bufs[s];
    delete[] bufs;
    delete[] lens;
    return ok ? (uint32_t)total : 0;
}

}  // namespace cve
