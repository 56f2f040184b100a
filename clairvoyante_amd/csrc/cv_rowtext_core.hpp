// cv_rowtext_core.hpp -- the arithmetic of one text tensor row (CreateTensor.py:52), as cv_format_tensor_row of
// cv_pileup.hip writes it: "<ctg> <centre> <seq>" and then " %0.1f" per value.  The SAME text compiles for the device
// (cv_rowtext_dev.hip: one wave per row, every lane a run of values) and for the host (tests/native/rowtext_core_driver.cpp
// runs it under AddressSanitizer / UBSan against snprintf), so the kernel is held to printf through this header.
//
// What it vouches for: a value v with v >= 0, v < 2^24 and v == (float)(int32_t)v -- the host formatter's own predicate for
// the branch that prints an integer and ".0".  Everything else (negative, fractional, 2^24 or more, NaN, infinite) is
// "%0.1f" of a double, which stays with the host: value_len() says 0 and the row goes back whole.  -0.0 passes the
// predicate and prints "0.0", as the host prints it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVR_FN __host__ __device__ inline
#else
#define CVR_FN inline
#endif

namespace cvr {

constexpr int FLANK = 16;
constexpr int WIDTH = 2 * FLANK + 1;
constexpr int NVALS = WIDTH * 16;                 // 528 values of a row
constexpr int LANES = 64;
constexpr int PER_LANE = (NVALS + LANES - 1) / LANES;    // 9: lane l formats the values [9 l, 9 l + 9) below NVALS
constexpr int MAX_VALUE = 11;                     // " 16777215.0"
constexpr int MAX_CTG = 255;                      // bytes of a contig name the device takes
constexpr int MAX_CENTRE = 19;                    // digits of an int64
constexpr int MAX_ROW = MAX_CTG + 1 + MAX_CENTRE + 1 + WIDTH + NVALS * MAX_VALUE + 1;     // 6 118 with the newline

// the host formatter's predicate; the order keeps the conversion defined (NaN fails the first comparison)
CVR_FN bool value_ok(float v) { return v >= 0.f && v < 16777216.f && v == (float)(int32_t)v; }

// decimal digits of u < 2^24 (1 .. 8)
CVR_FN int digits_u32(uint32_t u)
{
    return u < 10u ? 1 : u < 100u ? 2 : u < 1000u ? 3 : u < 10000u ? 4 : u < 100000u ? 5 : u < 1000000u ? 6 : u < 10000000u ? 7 : 8;
}

// bytes of " %0.1f" of v, or 0 when the device does not vouch for v
CVR_FN int value_len(float v) { return value_ok(v) ? 3 + digits_u32((uint32_t)(int32_t)v) : 0; }

// writes " <u>.0" of a value that passed value_ok(); nd = digits_u32(u) -> bytes written (nd + 3)
CVR_FN int value_write(char *dst, uint32_t u, int nd)
{
    dst[0] = ' ';
    for (int i = nd; i >= 1; --i) { dst[i] = (char)('0' + u % 10u); u /= 10u; }
    dst[nd + 1] = '.';
    dst[nd + 2] = '0';
    return nd + 3;
}

// decimal digits of a centre >= 1 (1 .. 19)
CVR_FN int digits_i64(int64_t c)
{
    int n = 1;
    while (c >= 10) { c /= 10; ++n; }
    return n;
}

CVR_FN void centre_write(char *dst, int64_t c, int nd)
{
    for (int i = nd - 1; i >= 0; --i) { dst[i] = (char)('0' + (int)(c % 10)); c /= 10; }
}

// the reference bytes of a row: what of [new_pos - 17, new_pos + 16) lies inside the window [0, ref_len)
// (new_pos = centre - ref_first0) -> *start, *len; fewer than 33 bytes where the window ends, none where it misses it
CVR_FN void seq_range(int64_t new_pos, int64_t ref_len, int64_t *start, int *len)
{
    const int64_t a = new_pos - (FLANK + 1) < 0 ? 0 : new_pos - (FLANK + 1);
    const int64_t b = new_pos > ref_len - FLANK ? ref_len : new_pos + FLANK;       // (no overflow at any centre)
    *start = a;
    *len = b > a ? (int)(b - a) : 0;
}

// bytes of "<ctg> <centre> <seq>", or 0 when the header is not the device's (centre < 1, a name above MAX_CTG)
CVR_FN int header_len(int ctg_len, int64_t centre, int64_t ref_first0, int64_t ref_len, int64_t *seq_start, int *seq_len)
{
    if (centre < 1 || ctg_len > MAX_CTG) return 0;
    seq_range(centre - ref_first0, ref_len, seq_start, seq_len);
    return ctg_len + 1 + digits_i64(centre) + 1 + *seq_len;
}

}  // namespace cvr
