// cv_vcf_core.hpp -- the arithmetic of one VCF record (callVar.py:72-153), restating vcf_record of cv_hostio.cpp field
// for field.  The SAME text compiles for the device (cv_vcf_dev.hip: one lane per candidate, a length pass and a write
// pass through record<Sink>) and for the host (cv_vcf_records_host_form; tests/native/vcf_core_driver.cpp runs it under
// AddressSanitizer / UBSan against cv_format_vcf), so the kernel is held to the host formatter through this header.
//
// What it vouches for (status DEVICE): decisions in range, a quality whose integer it can prove (below), a depth that is
// a positive integer below 2^24, |af| < 1e9, a position of 1..18 bare digits, a sequence of more than 16 bytes, a contig
// name of at most 255 bytes, a centre base of ACGT where one is needed.  Everything else is HOST: the caller sends the
// batch through cv_format_vcf, which gives the bytes or its own error.  NONE is a candidate without a record.
//
// The quality int(-4.343 * log(ratio)): libm's log is not correctly rounded and the device library's is another
// function, so log_pos() below is a fixed sequence of IEEE double + - * / (no library call, no contraction: both sides
// are built with -ffp-contract=off) that gives the same bits on host and device.  It stays within a few ulp of libm's
// (measured by the driver), and the integer is vouched for only where q lies further than M max(1, |q|) from the nearest
// integer, M = 2^-40 -- or where ratio == 1 exactly (q = -0.0, prints 0).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVV_FN __host__ __device__ inline
#else
#define CVV_FN inline
#endif

namespace cvv {

constexpr int FLANK = 16;
constexpr int WIDTH = 2 * FLANK + 1;
constexpr int ROW = WIDTH * 16;                   // floats of a candidate: [33][4 bases][4 matrices]
constexpr int MAX_CTG = 255;                      // bytes of a contig name the device takes
constexpr int MAX_POS_DIGITS = 18;
constexpr int MAX_TAIL = 160;                     // bytes of a record behind its contig name (the host's own bound)
constexpr double QUAL_MARGIN = 9.094947017729282379150390625e-13;      // M = 2^-40

enum { NONE = 0, DEVICE = 1, HOST = 2 };
// why a candidate is the host's (counted by the driver)
enum { WHY_NOT = 0, WHY_DECISION, WHY_QUALITY, WHY_DEPTH, WHY_CONTIG, WHY_POSITION, WHY_SEQUENCE, WHY_CENTRE, WHY_AF, WHY_COUNT };

CVV_FN uint64_t bits_of(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
CVV_FN double double_of(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
CVV_FN uint32_t bits_of(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
CVV_FN float float_of(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// log of a positive, normal, finite double: x = 2^e m with m in [sqrt(1/2), sqrt(2)], s = (m - 1) / (m + 1),
// log m = 2 atanh s = 2 s (1 + s^2/3 + s^4/5 + ...) with s^2 <= 0.0295 (the term behind s^24/25 is below 1e-19), and
// e ln 2 added in two parts (fdlibm's split: e LN2_HI is exact)
CVV_FN double log_pos(double x)
{
    const uint64_t u = bits_of(x);
    int e = (int)(u >> 52) - 1023;
    double m = double_of((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull);      // [1, 2)
    if (m > 1.4142135623730951) { m = m * 0.5; e += 1; }
    const double f = m - 1.0;                                                       // exact
    const double s = f / (2.0 + f);
    const double z = s * s;
    double p = 1.0 / 25.0;
    p = p * z + 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    const double r = 2.0 * s + (2.0 * s) * (z * p);
    const double de = (double)e;
    return de * 6.93147180369123816490e-01 + (r + de * 1.90821492927058770002e-10);
}

// the ratio of the fp32 top-2 products as the host forms it
CVV_FN double quality_ratio(float p1, float p2) { return ((double)p2 + 1e-300) / ((double)p1 + 1e-300); }

// the core's q = -4.343 log(ratio); false where ratio is not a positive normal number
CVV_FN bool quality_value(double ratio, double *q)
{
    *q = 0.0;
    if (!(ratio >= 2.2250738585072014e-308 && ratio <= 1.7976931348623157e308)) return false;      // (NaN fails)
    *q = -4.343 * log_pos(ratio);
    return true;
}

// int(q) where the core can prove it: ratio == 1, or q further than M max(1, |q|) from the nearest integer
CVV_FN bool quality_int(double ratio, int *qv)
{
    double q;
    if (!quality_value(ratio, &q)) return false;
    if (ratio == 1.0) { *qv = 0; return true; }
    const double t = (double)(long long)q;                                         // |q| < 3100: truncation toward zero
    const double fr = q - t < 0.0 ? t - q : q - t;
    const double dist = fr < 0.5 ? fr : 1.0 - fr;
    const double a = q < 0.0 ? -q : q;
    if (!(dist > QUAL_MARGIN * (a < 1.0 ? 1.0 : a))) return false;
    *qv = (int)t;
    return true;
}

// the host's own predicate for a depth it prints as an integer, without its zero
CVV_FN bool depth_ok(float dp) { return dp > 0.f && dp < 16777216.f && dp == (float)(int32_t)dp; }

CVV_FN float sum4(const float *p, int stride) { return ((p[0] + p[stride]) + p[2 * stride]) + p[3 * stride]; }
CVV_FN int argmax4(const float *p, int stride)
{
    int b = 0; float m = p[0];
    for (int k = 1; k < 4; k++) if (p[k * stride] > m) { m = p[k * stride]; b = k; }      // first maximum
    return b;
}
CVV_FN char upper(char ch) { return (ch >= 'a' && ch <= 'z') ? (char)(ch - 32) : ch; }
CVV_FN char base_of(int b) { return b == 0 ? 'A' : b == 1 ? 'C' : b == 2 ? 'G' : 'T'; }

// where a record goes: the length pass counts, the write pass stores
struct Count { int n; CVV_FN void put(char) { ++n; } };
struct Write { char *p; CVV_FN void put(char c) { *p++ = c; } };

template <class S> CVV_FN void put_str(S &s, const char *t) { while (*t) s.put(*t++); }
template <class S, class U> CVV_FN void put_uint(S &s, U u)
{
    U p = 1;
    while (u / p >= 10) p *= 10;
    for (; p; p /= 10) s.put((char)('0' + (int)((u / p) % 10)));
}
template <class S> CVV_FN void put_int(S &s, int v)
{
    if (v < 0) s.put('-');
    put_uint(s, v < 0 ? 0u - (uint32_t)v : (uint32_t)v);
}
// "%.4f" of an fp32 v with |v| < 1e9, as put_f4 of cv_hostio.cpp: |v| 10^4 is exact in double, adding and taking away
// 2^52 rounds it to the nearest integer, ties to even; the sign is the sign bit's ("-0.0000" exists)
template <class S> CVV_FN void put_f4(S &s, float v)
{
    const double a = (double)float_of(bits_of(v) & 0x7fffffffu);
    const uint64_t r = (uint64_t)((a * 10000.0 + 4503599627370496.0) - 4503599627370496.0);
    if (bits_of(v) >> 31) s.put('-');
    put_uint(s, r / 10000u);
    uint32_t f = (uint32_t)(r % 10000u);
    s.put('.');
    s.put((char)('0' + f / 1000u)); f %= 1000u;
    s.put((char)('0' + f / 100u)); f %= 100u;
    s.put((char)('0' + f / 10u));
    s.put((char)('0' + f % 10u));
}
CVV_FN bool af_ok(float v) { return (double)float_of(bits_of(v) & 0x7fffffffu) < 1e9; }      // (NaN, Inf fail)

// one candidate: c its 8 decision words, q its {p1, p2, dp, -}, x its tensor, the three tokens of its position
struct Cand {
    const int32_t *c; const float *q; const float *x;
    const char *chrom; int64_t chrom_len; const char *cs; int64_t cl; const char *seq; int64_t seq_len;
    int show_ref, has_qual, qual_min;
};

// the record of a candidate, '\n' included, into `out` -> NONE (nothing put), DEVICE, or HOST (what was put is void) with
// the reason in *why.  The order of the tests is vcf_record's.
template <class S> CVV_FN int record(const Cand &k, S &out, int *why)
{
    const int F = FLANK;
    const int32_t *c = k.c;
    *why = WHY_NOT;
    const int varType = c[0];
    if ((unsigned)varType > 3u || (unsigned)c[1] > 1u || (unsigned)c[2] > 5u) { *why = WHY_DECISION; return HOST; }
    if (varType == 0 && !k.show_ref) return NONE;
    int qv = 0;
    if (!quality_int(quality_ratio(k.q[0], k.q[1]), &qv)) { *why = WHY_QUALITY; return HOST; }
    const float dp = k.q[2];
    if (dp == 0.0f) return NONE;
    if (!depth_ok(dp)) { *why = WHY_DEPTH; return HOST; }
    if (k.chrom_len < 0 || k.chrom_len > MAX_CTG) { *why = WHY_CONTIG; return HOST; }
    if (k.cl < 1 || k.cl > MAX_POS_DIGITS) { *why = WHY_POSITION; return HOST; }
    uint64_t coord = 0;
    for (int i = 0; i < (int)k.cl; i++) {
        const char d = k.cs[i];
        if (d < '0' || d > '9') { *why = WHY_POSITION; return HOST; }
        coord = coord * 10u + (uint64_t)(d - '0');
    }
    if (k.seq_len <= F) { *why = WHY_SEQUENCE; return HOST; }
    const int sl = k.seq_len < WIDTH ? (int)k.seq_len : WIDTH;
    const float *x = k.x;
    const char centre = upper(k.seq[F]);
    int ref_len = 1, inferred = 0, nins = 0, varLength = c[2];
    bool sv = false;
    char ab = centre;
    float af;
    if (varType == 0 || varType == 1) {
        if (varType == 1) { const char b1 = base_of(c[3] & 3), b2 = base_of(c[4] & 3); ab = b1 != centre ? b1 : b2; }
        const int bi = ab == 'A' ? 0 : ab == 'C' ? 1 : ab == 'G' ? 2 : ab == 'T' ? 3 : -1;
        if (bi < 0) { *why = WHY_CENTRE; return HOST; }
        af = x[(F * 4 + bi) * 4 + 3] / dp;
    } else {
        const int mat = varType == 2 ? 1 : 2;
        if (varLength == 0) varLength = 1;
        af = sum4(x + (F + 1) * 16 + mat, 4) / dp;
        if (varLength == 5) {
            for (int p = F + 1; p < 2 * F + 1; p++) {
                if (p < F + 5 || sum4(x + p * 16 + mat, 4) >= 0.125f * sum4(x + p * 16 + 0, 4)) inferred++;
                else break;
            }
        }
        sv = inferred >= F;
        if (!sv) {
            const int want = varLength != 5 ? varLength : inferred;
            if (varType == 2) nins = want;
            else ref_len = F + want + 1 <= sl ? want + 1 : sl - F;                 // refSeq[F : F + want + 1], clipped like a slice
        }
    }
    if (!af_ok(af)) { *why = WHY_AF; return HOST; }

    for (int i = 0; i < (int)k.chrom_len; i++) out.put(k.chrom[i]);
    out.put('\t');
    put_uint(out, coord); out.put('\t'); out.put('.'); out.put('\t');
    for (int i = 0; i < ref_len; i++) out.put(upper(k.seq[F + i]));
    out.put('\t');
    if (sv) put_str(out, varType == 2 ? "<INS>" : "<DEL>");
    else {
        out.put(ab);
        for (int i = 0; i < nins; i++) out.put(base_of(argmax4(x + (F + 1 + i) * 16 + 1, 4)));
    }
    out.put('\t');
    put_int(out, qv); out.put('\t');
    put_str(out, !k.has_qual ? "." : (qv >= k.qual_min ? "PASS" : "LowQual")); out.put('\t');
    if (sv) put_str(out, varType == 2 ? "SVTYPE=INS" : "SVTYPE=DEL");
    else if (inferred > 0) { put_str(out, "LENGUESS="); put_int(out, inferred); }
    else out.put('.');
    put_str(out, "\tGT:GQ:DP:AF\t");
    put_str(out, varType == 0 ? "0/0" : (c[1] == 0 ? "0/1" : "1/1")); out.put(':');
    put_int(out, qv); out.put(':');
    put_uint(out, (uint32_t)(int32_t)dp); out.put(':');
    put_f4(out, af);
    out.put('\n');
    return DEVICE;
}

// the candidate i of a batch in cv_format_vcf's layout (pos_meta [rows, 6] = offset, length of contig / position / sequence)
CVV_FN Cand candidate(const int32_t *call, const float *qual, const float *x, const int64_t *xrow, const char *pos_buf,
                      const int64_t *pos_meta, const int64_t *pos_row, int show_ref, int has_qual, int qual_min, int64_t i)
{
    const int64_t *pm = pos_meta + (pos_row ? pos_row[i] : i) * 6;
    Cand k;
    k.c = call + i * 8; k.q = qual + i * 4; k.x = x + (xrow ? xrow[i] : i) * ROW;
    k.chrom = pos_buf + pm[0]; k.chrom_len = pm[1]; k.cs = pos_buf + pm[2]; k.cl = pm[3]; k.seq = pos_buf + pm[4]; k.seq_len = pm[5];
    k.show_ref = show_ref; k.has_qual = has_qual; k.qual_min = qual_min;
    return k;
}

}  // namespace cvv
