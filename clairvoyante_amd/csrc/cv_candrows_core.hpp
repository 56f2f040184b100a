// cv_candrows_core.hpp -- the arithmetic of one candidate row of ExtractVariantCandidates.py (OutputCandidate :22-42), as
// candidate_rows of clairvoyante_amd/ExtractVariantCandidates.py prints it:
//
//     <ctg> <pos0 + 1> <ref byte> <total> <S1> <c1> ... <S7> <c7>\n
//
// total = the seven counts summed in 64 bits, the (symbol, count) pairs by descending count, ties in the order
// A,C,G,T,I,D,N (Python's stable sorted(..., key=lambda x: -x[1])).  The SAME text compiles for the device
// (cv_candrows_dev.hip: one lane per row) and for the host (cv_candidate_rows_host_form;
// tests/native/candrows_core_driver.cpp runs it under AddressSanitizer / UBSan against snprintf and std::stable_sort).
//
// What it vouches for: a row whose entry index lies inside the entry arrays, whose position is 0 .. 2^63 - 2, whose seven
// counts are not negative and whose reference byte lies inside the loaded window and is below 0x80 (Python's chr() +
// .encode() turns a byte of 0x80 or more into two bytes); a contig name of at most MAX_CTG bytes.  Everything else is
// the host's: length 0, status HOST.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVC_FN __host__ __device__ inline
#else
#define CVC_FN inline
#endif

namespace cvc {

constexpr int NSYM = 7;
constexpr int MAX_CTG = 255;                      // bytes of a contig name the device takes
constexpr int MAX_POS = 19;                       // digits of pos0 + 1 <= 2^63 - 1
constexpr int MAX_TOTAL = 11;                     // digits of 7 * (2^31 - 1) = 15 032 385 529
constexpr int MAX_COUNT = 10;                     // digits of 2^31 - 1
// name, ' ', position, ' ', byte, ' ', total, seven times " S count", newline
constexpr int MAX_ROW = MAX_CTG + 1 + MAX_POS + 1 + 1 + 1 + MAX_TOTAL + NSYM * (3 + MAX_COUNT) + 1;
static_assert(MAX_ROW == 381, "the kernels size their LDS from this bound");
constexpr uint8_t STATUS_DEVICE = 0, STATUS_HOST = 1;     // CV_CANDROWS_DEVICE / CV_CANDROWS_HOST

CVC_FN int digits_u64(uint64_t u)
{
    int n = 1;
    while (u >= 10u) { u /= 10u; ++n; }
    return n;
}

// the nd digits of u at dst
CVC_FN void write_u64(char *dst, uint64_t u, int nd)
{
    for (int i = nd - 1; i >= 0; --i) { dst[i] = (char)('0' + (int)(u % 10u)); u /= 10u; }
}

// idx = 0 .. 6 by descending count, equal counts in ascending index: an insertion sort moves an element only past
// strictly smaller ones, so it is stable
CVC_FN void sort7(const int32_t c[NSYM], int idx[NSYM])
{
    for (int k = 0; k < NSYM; ++k) {
        int at = k;
        while (at > 0 && c[idx[at - 1]] < c[k]) { idx[at] = idx[at - 1]; --at; }
        idx[at] = k;
    }
}

// the device's verdict on the row's numbers (the reference byte has its own: ref_ok)
CVC_FN bool entry_ok(int ctg_len, int64_t pos0, const int32_t c[NSYM])
{
    if (ctg_len < 0 || ctg_len > MAX_CTG || pos0 < 0 || pos0 == INT64_MAX) return false;
    for (int k = 0; k < NSYM; ++k) if (c[k] < 0) return false;
    return true;
}

CVC_FN bool ref_ok(int64_t pos0, int64_t ref_first0, int64_t ref_len)
{
    return pos0 >= ref_first0 && pos0 - ref_first0 < ref_len;
}

CVC_FN uint64_t total_of(const int32_t c[NSYM])
{
    uint64_t t = 0;
    for (int k = 0; k < NSYM; ++k) t += (uint64_t)(int64_t)c[k];
    return t;
}

// bytes of a row that passed entry_ok(), its newline included
CVC_FN int row_len(int ctg_len, int64_t pos0, const int32_t c[NSYM])
{
    int n = ctg_len + 1 + digits_u64((uint64_t)pos0 + 1u) + 3 + digits_u64(total_of(c)) + 1;
    for (int k = 0; k < NSYM; ++k) n += 3 + digits_u64((uint64_t)c[k]);
    return n;
}

// writes the row (entry_ok() and a reference byte below 0x80) -> bytes written = row_len()
CVC_FN int row_write(char *dst, const char *ctg, int ctg_len, int64_t pos0, uint8_t ref_byte, const int32_t c[NSYM])
{
    const char sym[NSYM + 1] = "ACGTIDN";
    char *q = dst;
    for (int i = 0; i < ctg_len; ++i) q[i] = ctg[i];
    q += ctg_len;
    *q++ = ' ';
    int nd = digits_u64((uint64_t)pos0 + 1u);
    write_u64(q, (uint64_t)pos0 + 1u, nd);
    q += nd;
    *q++ = ' ';
    *q++ = (char)ref_byte;
    *q++ = ' ';
    const uint64_t t = total_of(c);
    nd = digits_u64(t);
    write_u64(q, t, nd);
    q += nd;
    int idx[NSYM];
    sort7(c, idx);
    for (int k = 0; k < NSYM; ++k) {
        const uint64_t v = (uint64_t)c[idx[k]];
        *q++ = ' ';
        *q++ = sym[idx[k]];
        *q++ = ' ';
        nd = digits_u64(v);
        write_u64(q, v, nd);
        q += nd;
    }
    *q++ = '\n';
    return (int)(q - dst);
}

// length and status of output row r = entry order[r] (order may be null: entry r); 0 and STATUS_HOST for a row the
// device does not vouch for
CVC_FN int row_verdict(int ctg_len, const int64_t *order, int64_t r, int64_t n, const int64_t *pos0, const int32_t *counts7,
                       const uint8_t *ref, int64_t ref_first0, int64_t ref_len, int64_t *entry, uint8_t *ref_byte)
{
    const int64_t e = order ? order[r] : r;
    *entry = e;
    if (e < 0 || e >= n) return 0;
    const int64_t p = pos0[e];
    if (!entry_ok(ctg_len, p, counts7 + e * NSYM) || !ref_ok(p, ref_first0, ref_len)) return 0;
    const uint8_t b = ref[p - ref_first0];
    if (b >= 0x80) return 0;
    *ref_byte = b;
    return row_len(ctg_len, p, counts7 + e * NSYM);
}

// cv_candidate_rows_host_form: every row in turn, as the two kernels and the scan between them leave it.  off[rows + 1],
// status[rows]; text may be null (lengths and status only).  A row that would end behind text_cap is not written.
inline void rows_host_form(const char *ctg, int64_t ctg_len, const int64_t *order, int64_t rows, int64_t n, const int64_t *pos0,
                           const int32_t *counts7, const uint8_t *ref, int64_t ref_first0, int64_t ref_len, int64_t *off,
                           uint8_t *status, char *text, int64_t text_cap)
{
    int64_t at = 0;
    const int cl = ctg_len > MAX_CTG ? MAX_CTG + 1 : (int)ctg_len;
    for (int64_t r = 0; r < rows; ++r) {
        int64_t e = 0;
        uint8_t b = 0;
        const int len = row_verdict(cl, order, r, n, pos0, counts7, ref, ref_first0, ref_len, &e, &b);
        off[r] = at;
        status[r] = len ? STATUS_DEVICE : STATUS_HOST;
        if (len && text && at + len <= text_cap) row_write(text + at, ctg, cl, pos0[e], b, counts7 + e * NSYM);
        at += len;
    }
    off[rows] = at;
}

}  // namespace cvc
