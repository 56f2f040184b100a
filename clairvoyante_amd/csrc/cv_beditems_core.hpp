// cv_beditems_core.hpp -- what ChooseItemInBed / CountNumInBed / RandomSampling compute per line and per position
// (bed_items.py: choose_items_host, count_items_host, sample_positions_host are the definitions).  The SAME text compiles
// for the device (cv_beditems_dev.hip) and for the host (the *_host_form entry points; tests/native/bed_items_driver.cpp
// runs it under AddressSanitizer / UBSan over heap blocks of exactly the bytes it may touch).
//
//   lower_bound / upper_bound   the binary searches of every device reader over its sorted tables
//   stab          _Intervals.hit over one contig's sorted table: upper_bound(begin, pos) = k > 0 and emax[k - 1] > pos
//   copy_lane     one lane's share of a line copied by a wave of 64 lanes (see cv_beditems_dev.hip for the form)
//   sample_keep   "in an interval, when there are intervals, and u(pos) <= prob"
//   lines_host_form / keep_host_form   the two slab passes on the CPU, in the layout of the *_dev calls
//   copy_fits / copy_host_form         the bounds test of one copied line; the gather by given lengths on the CPU
#pragma once
#include <stdint.h>
#include "cv_draw_core.hpp"
#include "cv_truth_core.hpp"

namespace cvb {

constexpr int WAVE = 64;
constexpr int DRAW_RANDOM = 2;                                   // draws.RANDOM

// first slot of the sorted a[0, n) whose value is >= v
CVT_FN int64_t lower_bound(const uint64_t *a, int64_t n, uint64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// number of elements of the sorted a[0, n) that are <= v
CVT_FN int64_t upper_bound(const int64_t *a, int64_t n, int64_t v)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

CVT_FN bool stab(const int64_t *begin, const int64_t *emax, int64_t m, int64_t p)
{
    const int64_t u = upper_bound(begin, m, p);
    return u > 0 && emax[u - 1] > p;
}

// the verdict of one row of a slab: run -> BED contig id (-1: a contig the BED lacks) -> the stabbing test
CVT_FN bool keep_row(int64_t pos, int32_t run, const int32_t *run_ctg, int64_t nruns, int32_t nctg, const int64_t *bed_off,
                     const int64_t *bed_begin, const int64_t *bed_emax)
{
    if (run < 0 || run >= nruns) return false;
    const int32_t c = run_ctg[run];
    if (c < 0 || c >= nctg) return false;
    const int64_t lo = bed_off[c], m = bed_off[c + 1] - lo;
    return stab(bed_begin + lo, bed_emax + lo, m, pos);
}

CVT_FN bool sample_keep(uint64_t seed, uint32_t h, int64_t pos, double prob, int64_t nbed, const int64_t *bed_begin,
                        const int64_t *bed_emax)
{
    if (nbed > 0 && !stab(bed_begin, bed_emax, nbed, pos)) return false;
    return cv_draw(seed, DRAW_RANDOM, h, pos, 0) <= prob;
}

struct G16 { uint32_t w[4]; };

// Lane `lane` of a wave of WAVE lanes copies its share of src[0, n) to dst[0, n).  A line under 64 bytes is one byte per
// lane.  Otherwise: a byte head of up to 15 bytes brings dst to a 16-byte boundary; where src then sits on one too the
// body moves in 16-byte granules, else in 4-byte stores put together from four byte loads (dst is aligned, src is not); a
// byte tail of up to 15 bytes.  Every byte of dst[0, n) has exactly one writer and nothing outside src[0, n) is read.
CVT_FN void copy_lane(uint8_t *dst, const uint8_t *src, int64_t n, int lane)
{
    if (n < WAVE) {
        if (lane < n) dst[lane] = src[lane];
        return;
    }
    const int64_t head = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (lane < head) dst[lane] = src[lane];
    uint8_t *d = dst + head;
    const uint8_t *s = src + head;
    const int64_t body = n - head;
    int64_t done;
    if (((uintptr_t)s & 15) == 0) {
        const int64_t g = body >> 4;
        for (int64_t k = lane; k < g; k += WAVE) {
            G16 v;
            __builtin_memcpy(&v, __builtin_assume_aligned(s + 16 * k, 16), 16);
            __builtin_memcpy(__builtin_assume_aligned(d + 16 * k, 16), &v, 16);
        }
        done = g << 4;
    } else {
        const int64_t g = body >> 2;
        for (int64_t k = lane; k < g; k += WAVE) {
            const uint8_t *q = s + 4 * k;
            const uint32_t w = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
            __builtin_memcpy(__builtin_assume_aligned(d + 4 * k, 4), &w, 4);
        }
        done = g << 2;
    }
    for (int64_t k = done + lane; k < body; k += WAVE) d[k] = s[k];
}

// Host form of cv_item_lines_dev over text[0, len): the same outputs in the same layout (include/clairvoyante_amd.h)
inline void lines_host_form(const uint8_t *text, int64_t len, int64_t max_lines, int64_t *pos, int32_t *run, int64_t *off, int64_t *llen,
                            int64_t *tok, int64_t *info)
{
    int64_t lines = 0, rows = 0, host = 0, runs = 0, start = 0;
    int64_t prev_off = 0, prev_len = -1;                         // the contig token of the line before, when that was a ROW
    for (int64_t i = 0; i < len && lines < max_lines; ++i) {
        if (text[i] != '\n') continue;
        cvt::Line L;
        cvt::verdict(text + start, i - start, cvt::FMT_ITEM, nullptr, false, &L);
        if (L.status == cvt::ROW) {
            bool differs = prev_len != L.ctg_len;
            for (int k = 0; !differs && k < L.ctg_len; ++k) differs = text[prev_off + k] != text[start + L.ctg_off + k];
            if (differs) { tok[2 * runs] = start + L.ctg_off; tok[2 * runs + 1] = L.ctg_len; ++runs; }
            pos[rows] = L.pos;
            run[rows] = (int32_t)(runs - 1);
            off[rows] = start;
            llen[rows] = i + 1 - start;
            ++rows;
            prev_off = start + L.ctg_off; prev_len = L.ctg_len;
        } else {
            prev_len = -1;
            ++host;
        }
        ++lines;
        start = i + 1;
    }
    info[0] = start; info[1] = lines; info[2] = rows; info[3] = 0; info[4] = host; info[5] = runs; info[6] = 0; info[7] = 0;
}

// Host form of cv_items_keep_dev: the verdicts, the running sum of the kept lengths, the copy lane by lane
inline void keep_host_form(const uint8_t *text, int64_t len, int64_t n, const int64_t *pos, const int32_t *run, const int64_t *off,
                           const int64_t *llen, const int32_t *run_ctg, int64_t nruns, int32_t nctg, const int64_t *bed_off,
                           const int64_t *bed_begin, const int64_t *bed_emax, int want_text, uint8_t *out_text, int64_t out_cap,
                           int64_t *counts)
{
    int64_t kept = 0, bytes = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!keep_row(pos[i], run[i], run_ctg, nruns, nctg, bed_off, bed_begin, bed_emax)) continue;
        ++kept;
        if (!want_text) continue;
        if (off[i] >= 0 && llen[i] >= 0 && off[i] + llen[i] <= len && bytes + llen[i] <= out_cap)
            for (int lane = 0; lane < WAVE; ++lane) copy_lane(out_text + bytes, text + off[i], llen[i], lane);
        bytes += llen[i];
    }
    counts[0] = n; counts[1] = kept; counts[2] = bytes; counts[3] = 0;
}

// "m bytes at src offset s of a text of len bytes and at dst offset d of a room of cap bytes lie inside both", without a sum
// that could overflow on a caller's wrong length
CVT_FN bool copy_fits(int64_t s, int64_t m, int64_t len, int64_t d, int64_t cap)
{
    return m > 0 && m <= len && s >= 0 && s <= len - m && m <= cap && d >= 0 && d <= cap - m;
}

// Host form of cv_items_copy_dev: the running sum of the given lengths places the lines (0: the line is not kept; a negative
// length is the caller's error, never copied, and the sum takes it as the device's scan does), the copy lane by lane where
// the line lies inside the text and fits the room
inline void copy_host_form(const uint8_t *text, int64_t len, int64_t n, const int64_t *off, const int64_t *kept_len, uint8_t *out_text,
                           int64_t out_cap, int64_t *counts)
{
    uint64_t bytes = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t m = kept_len[i];
        if (copy_fits(off[i], m, len, (int64_t)bytes, out_cap))
            for (int lane = 0; lane < WAVE; ++lane) copy_lane(out_text + bytes, text + off[i], m, lane);
        bytes += (uint64_t)m;
    }
    counts[0] = 0; counts[1] = 0; counts[2] = (int64_t)bytes; counts[3] = 0;
}

}  // namespace cvb
