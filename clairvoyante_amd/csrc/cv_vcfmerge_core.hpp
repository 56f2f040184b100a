// cv_vcfmerge_core.hpp -- the arithmetic of the VCF merge (clairvoyante_amd/vcf_merge.py is the definition) once, for the
// kernels of cv_vcfmerge_dev.hip and for the host forms; compiles with g++ alone (tests/native/vcf_merge_driver.cpp).
//
//   reg2bin        the UCSC bin of [beg, end) that tabix uses
//   line_fields    one record line -> reflen, end, bin and the verdict: DEVICE, or HOST for a line only the definition
//                  answers (fewer than 8 tab-separated columns, the first two columns not "token TAB digits TAB", an END=
//                  key in INFO, an empty REF, POS < 1, end > 2^29, a line that does not end in a newline or is longer
//                  than LINE_CAP).  The byte rule (no '\r', printable ASCII) is the item line pass's, which ran before.
//   copy_record    the bytes of one record from the text, read as ALIGNED 16-byte granules and funnel-shifted, into a
//                  tile (LDS on the device) at any byte offset: dwords in the middle, bytes at the two ends
//   merge_host_form / windows_host_form   the whole of cv_vcf_merge_dev / cv_vcf_windows_dev on the CPU, the tile included
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#if defined(__HIPCC__)
#define CVM_HD __host__ __device__ inline
#else
#define CVM_HD inline
#endif

namespace cvm {

constexpr int64_t MAX_END = (int64_t)1 << 29;
constexpr int WINDOW_SHIFT = 14;
constexpr int LINE_CAP = 8192;
constexpr int POS_BITS = 40;                       // the sort key is rank << POS_BITS | POS
constexpr int MAX_RANKS = 1 << 20;
constexpr int STATUS_DEVICE = 1, STATUS_HOST = 2;
constexpr int LANES = 64;
constexpr int TILE_TEXT = 16 * 1024;               // bytes of 64 consecutive records that are assembled in one tile
constexpr int TILE_BYTES = TILE_TEXT + 32;         // ... standing at any phase, in whole granules
constexpr int64_t UNSET = INT64_MAX;

CVM_HD int32_t reg2bin(int64_t beg, int64_t end)
{
    const int64_t e = end - 1;
    if (beg >> 14 == e >> 14) return (int32_t)(4681 + (beg >> 14));
    if (beg >> 17 == e >> 17) return (int32_t)(585 + (beg >> 17));
    if (beg >> 20 == e >> 20) return (int32_t)(73 + (beg >> 20));
    if (beg >> 23 == e >> 23) return (int32_t)(9 + (beg >> 23));
    if (beg >> 26 == e >> 26) return (int32_t)(1 + (beg >> 26));
    return 0;
}

struct Fields {
    int32_t reflen, bin, verdict;
    int64_t end;
};

// s[0, len): one line with its newline; pos: its second column as the item pass read it
CVM_HD Fields line_fields(const char *s, int64_t len, int64_t pos)
{
    Fields f;
    f.reflen = 0; f.bin = 0; f.end = 0; f.verdict = STATUS_HOST;
    if (len < 2 || len > LINE_CAP || s[len - 1] != '\n') return f;
    const int64_t n = len - 1;                      // without the newline
    // the tabs: REF lies between the third and the fourth, INFO behind the seventh
    int tabs = 0;
    int64_t ref_at = -1, ref_end = -1, info_at = -1, info_end = n, tab1 = -1, tab2 = -1;
    for (int64_t i = 0; i < n && tabs < 8; ++i) {
        if (s[i] != '\t') continue;
        ++tabs;
        if (tabs == 1) tab1 = i;
        else if (tabs == 2) tab2 = i;
        else if (tabs == 3) ref_at = i + 1;
        else if (tabs == 4) ref_end = i;
        else if (tabs == 7) info_at = i + 1;
        else if (tabs == 8) info_end = i;
    }
    if (tabs < 7) return f;                         // fewer than 8 columns
    // the item pass cut its two tokens at blanks AND tabs: the definition splits at tabs alone
    if (tab1 < 1 || tab2 < tab1 + 2) return f;
    for (int64_t i = 0; i < tab2; ++i)
        if (s[i] == ' ') return f;
    for (int64_t i = tab1 + 1; i < tab2; ++i)
        if (s[i] < '0' || s[i] > '9') return f;
    for (int64_t i = info_at; i + 4 <= info_end; ++i)
        if ((i == info_at || s[i - 1] == ';') && s[i] == 'E' && s[i + 1] == 'N' && s[i + 2] == 'D' && s[i + 3] == '=') return f;
    const int64_t reflen = ref_end - ref_at;
    if (reflen < 1 || pos < 1 || pos > MAX_END) return f;
    const int64_t beg = pos - 1, end = beg + reflen;
    if (end > MAX_END) return f;
    f.reflen = (int32_t)reflen;
    f.end = end;
    f.bin = reg2bin(beg, end);
    f.verdict = STATUS_DEVICE;
    return f;
}

struct alignas(16) Granule { uint32_t x, y, z, w; };            // 16 bytes, as the device loads them (uint4)

// the text as aligned 16-byte granules, one held at a time: words are asked for in ascending order, so every granule is
// loaded once, and only a granule that holds a byte of the record is ever loaded
struct Source {
    const Granule *g;
    Granule cur;
    int64_t at;
    CVM_HD explicit Source(const void *text) : g((const Granule *)text), at(-1) { cur.x = cur.y = cur.z = cur.w = 0; }
    CVM_HD uint32_t word(int64_t a)                 // the a-th aligned dword of the text
    {
        if ((a >> 2) != at) { at = a >> 2; cur = g[at]; }
        const int k = (int)(a & 3);
        return k == 0 ? cur.x : k == 1 ? cur.y : k == 2 ? cur.z : cur.w;
    }
    // the (at most four) bytes at byte offset p, of which `avail` >= 1 belong to the record
    CVM_HD uint32_t bytes_at(int64_t p, int avail)
    {
        const int sh = (int)(p & 3) * 8;
        const uint32_t lo = word(p >> 2);
        if (sh == 0) return lo;
        const uint32_t hi = (int)(p & 3) + (avail < 4 ? avail : 4) > 4 ? word((p >> 2) + 1) : 0;
        return (lo >> sh) | (hi << (32 - sh));
    }
};

// text[s, s + len) -> tile[d, d + len); tile is 4-byte aligned, text 16-byte aligned and readable up to the end of the
// granule that holds its last byte
CVM_HD void copy_record(char *tile, int d, const void *text, int64_t s, int len)
{
    Source src(text);
    int head = (4 - (d & 3)) & 3;
    if (head > len) head = len;
    if (head) {
        const uint32_t w = src.bytes_at(s, head);
        for (int i = 0; i < head; ++i) tile[d + i] = (char)(w >> (8 * i));
    }
    const int nw = (len - head) >> 2;
    const int64_t p = s + head;
    uint32_t *out = (uint32_t *)(tile + d + head);
    const int sh = (int)(p & 3) * 8;
    const int64_t a = p >> 2;
    if (sh == 0) {
        for (int k = 0; k < nw; ++k) out[k] = src.word(a + k);
    } else if (nw) {
        uint32_t prev = src.word(a);
        for (int k = 0; k < nw; ++k) {
            const uint32_t nxt = src.word(a + k + 1);
            out[k] = (prev >> sh) | (nxt << (32 - sh));
            prev = nxt;
        }
    }
    const int tail = len - head - 4 * nw;
    if (tail) {
        const uint32_t w = src.bytes_at(p + 4 * (int64_t)nw, tail);
        for (int i = 0; i < tail; ++i) tile[d + head + 4 * nw + i] = (char)(w >> (8 * i));
    }
}

CVM_HD int bits_for(int64_t values)                 // bits that hold 0 .. values - 1
{
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < values) ++b;
    return b;
}

// cv_vcf_merge_dev on the CPU: the same per-line function, a stable sort, the tiles of 64 records through copy_record
inline void merge_host_form(const char *text, int64_t text_len, int64_t n, const int64_t *pos, const int32_t *run, const int64_t *off,
                            const int64_t *llen, const int32_t *run_rank, int64_t nruns, int32_t nrank, int32_t *srank,
                            int64_t *sbeg, int64_t *send, int64_t *ooff, char *out_text, int64_t out_cap, int64_t *chunks,
                            int64_t *stats, int64_t *info)
{
    std::vector<uint64_t> key((size_t)n);
    std::vector<int64_t> perm((size_t)n), end((size_t)n);
    std::vector<int32_t> bin((size_t)n);
    std::vector<char> good((size_t)n);
    int64_t host = 0;
    for (int64_t i = 0; i < n; ++i) {
        Fields f;
        f.verdict = STATUS_HOST; f.end = 0; f.bin = 0;
        int64_t rank = 0;
        const bool inside = off[i] >= 0 && llen[i] > 0 && off[i] + llen[i] <= text_len && run[i] >= 0 && run[i] < nruns;
        if (inside) {
            rank = run_rank[run[i]];
            if (rank >= 0 && rank < nrank) f = line_fields(text + off[i], llen[i], pos[i]); else rank = 0;
        }
        good[i] = f.verdict == STATUS_DEVICE;
        host += !good[i];
        key[i] = good[i] ? (uint64_t)rank << POS_BITS | (uint64_t)pos[i] : 0;
        end[i] = f.end; bin[i] = f.bin; perm[i] = i;
    }
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b) { return key[a] < key[b]; });
    std::vector<int32_t> sbin((size_t)n);
    ooff[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t j = perm[i];
        srank[i] = (int32_t)(key[j] >> POS_BITS);
        sbeg[i] = (int64_t)(key[j] & (((uint64_t)1 << POS_BITS) - 1)) - 1;
        send[i] = end[j]; sbin[i] = bin[j];
        ooff[i + 1] = ooff[i] + (good[j] ? llen[j] : 0);
    }
    // the text: tiles of 64 records, assembled at the phase the range has in the output
    std::vector<uint32_t> tile(TILE_BYTES / 4);
    for (int64_t r0 = 0; r0 < n; r0 += LANES) {
        const int64_t cnt = n - r0 < LANES ? n - r0 : LANES, start = ooff[r0], bytes = ooff[r0 + cnt] - start;
        if (start + bytes > out_cap || !out_text) continue;
        const int phase = (int)((uintptr_t)(out_text + start) & 15);
        for (int64_t r = r0; r < r0 + cnt; ++r) {
            const int64_t j = perm[r];
            if (!good[j]) continue;
            if (bytes <= TILE_TEXT) copy_record((char *)tile.data(), phase + (int)(ooff[r] - start), text, off[j], (int)llen[j]);
            else memcpy(out_text + ooff[r], text + off[j], (size_t)llen[j]);
        }
        if (bytes <= TILE_TEXT) memcpy(out_text + start, (char *)tile.data() + phase, (size_t)bytes);
    }
    // chunks: runs of equal (rank, bin), then sorted by (rank, bin), file order kept
    std::vector<int64_t> cr, cb, cu, ce;
    for (int64_t i = 0; i < n; ++i) {
        if (i == 0 || srank[i] != srank[i - 1] || sbin[i] != sbin[i - 1]) { cr.push_back(srank[i]); cb.push_back(sbin[i]); cu.push_back(ooff[i]); ce.push_back(0); }
        ce.back() = ooff[i + 1];
    }
    const int64_t nc = (int64_t)cr.size();
    std::vector<int64_t> order((size_t)nc);
    for (int64_t c = 0; c < nc; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return cr[a] != cr[b] ? cr[a] < cr[b] : cb[a] < cb[b]; });
    for (int64_t c = 0; c < nc; ++c) {
        const int64_t v = order[c];
        chunks[c] = cr[v]; chunks[n + c] = cb[v]; chunks[2 * n + c] = cu[v]; chunks[3 * n + c] = ce[v];
    }
    for (int64_t k = 0; k < 4 * (int64_t)nrank; ++k) stats[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = srank[i];
        if (r < 0 || r >= nrank) continue;
        if (stats[2 * nrank + r] == 0) stats[r] = ooff[i];
        stats[nrank + r] = ooff[i + 1];
        stats[2 * nrank + r] += 1;
        if (send[i] > stats[3 * nrank + r]) stats[3 * nrank + r] = send[i];
    }
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[0] = host; info[1] = nc; info[2] = ooff[n];
}

inline void windows_host_form(int64_t n, const int32_t *srank, const int64_t *sbeg, const int64_t *send, const int64_t *ooff,
                              int32_t nrank, const int64_t *win_off, int64_t *win, int64_t nwin)
{
    for (int64_t w = 0; w < nwin; ++w) win[w] = UNSET;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t r = srank[i];
        if (r < 0 || r >= nrank || sbeg[i] < 0 || send[i] <= sbeg[i]) continue;
        const int64_t base = win_off[r], cnt = win_off[r + 1] - base;
        for (int64_t w = sbeg[i] >> WINDOW_SHIFT; w <= (send[i] - 1) >> WINDOW_SHIFT; ++w)
            if (w < cnt && base + w >= 0 && base + w < nwin && ooff[i] < win[base + w]) win[base + w] = ooff[i];
    }
    for (int32_t r = 0; r < nrank; ++r) {
        int64_t lo = win_off[r], hi = win_off[r + 1];
        if (lo < 0) lo = 0;
        if (hi > nwin) hi = nwin;
        for (int64_t w = hi - 2; w >= lo; --w)
            if (win[w + 1] < win[w]) win[w] = win[w + 1];
    }
}

}  // namespace cvm
