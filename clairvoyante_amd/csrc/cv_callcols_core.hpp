// cv_callcols_core.hpp -- what callVarBam.region_tensors decides and builds per candidate centre between the pileup and the
// call loop: does the centre give a row, which reference window goes with it, how its coordinate is spelt -- the tokens of
// utils_v2.PosBatch.from_columns(ctg, centres_kept, seqs_kept).  The SAME text compiles for the device
// (cv_callcols_dev.hip) and for the host (cv_call_columns_host_form; tests/native/call_columns_driver.cpp runs it under
// AddressSanitizer / UBSan into heap blocks of exactly the bytes it may write).
//
// The definition (clairvoyante_amd/callVarBam.py, host route), with p = c - shift and ri = p - 1 = c - 1 - ref_first:
//   seq  = ref_seq[p - 17 : p + 16].upper() if p - 17 >= 0 else b""        -> ref[ri - 16 : min(ri + 17, ref_len)]
//   keep = touched and len(seq) > 16 and seq[16:17] in (b"A", b"C", b"G", b"T")
// len(seq) > 16 is ri < ref_len; bytes.upper() maps a..z and nothing else (a byte >= 0x80 stays as it is).  A kept row has
// ri >= 16, so with ref_first >= 0 (the entry points insist on it) its centre is >= 17 and "%d" of it is 2..10 bare digits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVK_FN __host__ __device__ inline
#else
#define CVK_FN inline
#endif

namespace cvk {

constexpr int FLANK = 16;
constexpr int WIDTH = 2 * FLANK + 1;
constexpr int MAX_DIGITS = 10;                    // a centre is an int32
constexpr int MAX_ROW_TEXT = MAX_DIGITS + WIDTH;  // 43: the text is at most ctg_len + 43 n bytes

// Python's bytes.upper() of one byte
CVK_FN unsigned upper(unsigned b) { return b >= 'a' && b <= 'z' ? b - 32u : b; }

struct Row {
    int keep;        // the centre gives a row
    int digits;      // of its coordinate (0 when not kept)
    int wlen;        // bytes of its window, 17 .. 33 (0 when not kept)
    int64_t w0;      // the window is ref[w0, w0 + wlen)
};

// decimal digits of c >= 1 (1 .. 10)
CVK_FN int digits_of(int64_t c)
{
    int n = 1;
    while (c >= 10) { c /= 10; ++n; }
    return n;
}

// byte t (0 = the most significant) of the nd digits of c
CVK_FN char digit_at(int64_t c, int nd, int t)
{
    for (int i = nd - 1 - t; i > 0; --i) c /= 10;
    return (char)('0' + (int)(c % 10));
}

CVK_FN Row row_of(int64_t c, bool touched, const uint8_t *ref, int64_t ref_first, int64_t ref_len)
{
    Row r{0, 0, 0, 0};
    const int64_t ri = c - 1 - ref_first;                    // the centre inside the loaded reference
    if (!touched || c < 1 || ri - FLANK < 0 || ri >= ref_len) return r;
    const unsigned b = upper(ref[ri]);
    if (b != 'A' && b != 'C' && b != 'G' && b != 'T') return r;
    const int64_t end = ri + FLANK + 1 < ref_len ? ri + FLANK + 1 : ref_len;
    r.keep = 1;
    r.digits = digits_of(c);
    r.w0 = ri - FLANK;
    r.wlen = (int)(end - r.w0);
    return r;
}

// value q (0 .. 5) of a row's meta: offset and length of the contig name, the coordinate and the window inside the text
CVK_FN int64_t meta_at(int q, int64_t ctg_len, int64_t coord_at, int digits, int64_t seq_at, int wlen)
{
    return q == 0 ? 0 : q == 1 ? ctg_len : q == 2 ? coord_at : q == 3 ? (int64_t)digits : q == 4 ? seq_at : (int64_t)wlen;
}

// All of it on the CPU, one centre after the other: what the kernels must give.  index [n], meta [n,6] and text
// [ctg_len + 43 n] are written for the k kept rows only; info [4] = {k, bytes of text, n, 0}.
inline void host_form(const char *ctg, int64_t ctg_len, const int32_t *centres, const uint8_t *touched, int64_t n, const uint8_t *ref,
                      int64_t ref_first, int64_t ref_len, int64_t *index, int64_t *meta, char *text, int64_t *info)
{
    int64_t k = 0, digits = 0, window = 0;
    for (int64_t i = 0; i < n; i++) {
        const Row r = row_of(centres[i], touched[i] != 0, ref, ref_first, ref_len);
        if (r.keep) { k++; digits += r.digits; }
    }
    for (int64_t t = 0; t < ctg_len; t++) text[t] = ctg[t];
    int64_t j = 0, coord_at = ctg_len;
    const int64_t seq0 = ctg_len + digits;
    for (int64_t i = 0; i < n; i++) {
        const Row r = row_of(centres[i], touched[i] != 0, ref, ref_first, ref_len);
        if (!r.keep) continue;
        const int64_t seq_at = seq0 + window;
        index[j] = i;
        for (int q = 0; q < 6; q++) meta[j * 6 + q] = meta_at(q, ctg_len, coord_at, r.digits, seq_at, r.wlen);
        for (int t = 0; t < r.digits; t++) text[coord_at + t] = digit_at(centres[i], r.digits, t);
        for (int t = 0; t < r.wlen; t++) text[seq_at + t] = (char)upper(ref[r.w0 + t]);
        coord_at += r.digits;
        window += r.wlen;
        j++;
    }
    info[0] = k; info[1] = seq0 + window; info[2] = n; info[3] = 0;
}

}  // namespace cvk
