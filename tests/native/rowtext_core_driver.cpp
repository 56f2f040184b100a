// rowtext_core_driver.cpp -- the host form of csrc/cv_rowtext_core.hpp (what the rowtext kernels of cv_rowtext_dev.hip
// compute per value and per header) over a seeded corpus, checked against printf.  Built by
// tests/test_rowtext_core_host.py with -fsanitize=address,undefined; every row is formatted into a heap block of exactly
// its length, so one byte too many is a finding.
//
//   rowtext_core_driver SEED RANDOM_ROWS   -> "ok <rows> rows, <vouched> on the device side, <bytes> bytes", exit 0
//
// Per value: value_ok() must be the host formatter's predicate (v >= 0, v < 2^24, whole) and, where it holds,
// value_write() must give " " + snprintf("%0.1f") in value_len() bytes; where it does not, value_len() is 0 and the row
// is the host's.  Per row: the lanes' split of cv_rowtext_dev.hip (lane l takes the values [9 l, 9 l + 9), an exclusive
// sum of the lanes' byte counts places them) must give the row snprintf gives.
#include <inttypes.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_rowtext_core.hpp"

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(rng_state >> 32);
}

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

static int fail(const char *what, long row, int k, float v)
{
    uint32_t b; memcpy(&b, &v, 4);
    fprintf(stderr, "FAIL %s: row %ld value %d = %.9g (bits %08x)\n", what, row, k, (double)v, b);
    return 1;
}

// the reference: what cv_format_tensor_row prints for one value, through printf alone.  -0.0 passes the host's predicate
// and leaves through its integer branch as "0.0" (printf alone would say "-0.0"), so the sign of a zero is dropped here
static std::string printf_value(float v)
{
    char tmp[64];
    const int n = snprintf(tmp, sizeof tmp, " %0.1f", v == 0.f ? 0.0 : (double)v);
    return std::string(tmp, (size_t)n);
}

static bool whole_small(float v) { return v >= 0.f && v < 16777216.f && floorf(v) == v; }

struct Row { std::string ctg; int64_t centre, first0; std::string ref; std::vector<float> v; };

static long vouched = 0, bytes = 0;

static int check_row(long id, const Row &r)
{
    // 1. per value
    bool all_ok = true;
    for (int k = 0; k < cvr::NVALS; ++k) {
        const float v = r.v[(size_t)k];
        const bool ok = cvr::value_ok(v);
        if (ok != whole_small(v)) return fail("predicate", id, k, v);
        const int len = cvr::value_len(v);
        if (!ok) { if (len != 0) return fail("length of a value left to the host", id, k, v); all_ok = false; continue; }
        const std::string want = printf_value(v);
        if (len != (int)want.size()) return fail("length", id, k, v);
        if (len > cvr::MAX_VALUE) return fail("longer than MAX_VALUE", id, k, v);
        char *dst = (char *)malloc((size_t)len);            // exactly len bytes: ASan sees one too many
        const uint32_t u = (uint32_t)(int32_t)v;
        const int w = cvr::value_write(dst, u, cvr::digits_u32(u));
        const bool same = w == len && memcmp(dst, want.data(), (size_t)len) == 0;
        free(dst);
        if (!same) return fail("bytes", id, k, v);
    }
    // 2. the header
    int64_t s0 = 0; int sl = 0;
    const int head = cvr::header_len((int)r.ctg.size(), r.centre, r.first0, (int64_t)r.ref.size(), &s0, &sl);
    const int64_t new_pos = r.centre - r.first0;
    const bool head_ok = r.centre >= 1 && (int)r.ctg.size() <= cvr::MAX_CTG;
    if ((head != 0) != head_ok) { fprintf(stderr, "FAIL header verdict: row %ld\n", id); return 1; }
    if (!head_ok || !all_ok) return 0;
    std::string seq;
    for (int64_t at = new_pos - 17; at < new_pos + 16; ++at)            // what of the 33 positions lies inside the window
        if (at >= 0 && at < (int64_t)r.ref.size()) seq += r.ref[(size_t)at];
    char num[32];
    snprintf(num, sizeof num, "%" PRId64, r.centre);
    std::string want = r.ctg + " " + num + " " + seq;
    if (head != (int)want.size() || sl != (int)seq.size()) { fprintf(stderr, "FAIL header length: row %ld\n", id); return 1; }
    for (int k = 0; k < cvr::NVALS; ++k) want += printf_value(r.v[(size_t)k]);
    want += "\n";
    // 3. the row as the wave assembles it
    int mine[cvr::LANES], total = 0;
    for (int lane = 0; lane < cvr::LANES; ++lane) {
        mine[lane] = 0;
        for (int j = 0; j < cvr::PER_LANE; ++j)
            if (lane * cvr::PER_LANE + j < cvr::NVALS) mine[lane] += cvr::value_len(r.v[(size_t)(lane * cvr::PER_LANE + j)]);
        total += mine[lane];
    }
    const size_t len = (size_t)head + (size_t)total + 1;
    if (len != want.size() || len > (size_t)cvr::MAX_ROW) { fprintf(stderr, "FAIL row length: row %ld\n", id); return 1; }
    char *buf = (char *)malloc(len);
    memcpy(buf, r.ctg.data(), r.ctg.size());
    const int nd = cvr::digits_i64(r.centre);
    buf[r.ctg.size()] = ' ';
    cvr::centre_write(buf + r.ctg.size() + 1, r.centre, nd);
    buf[r.ctg.size() + 1 + (size_t)nd] = ' ';
    for (int i = 0; i < sl; ++i) buf[r.ctg.size() + 2 + (size_t)nd + (size_t)i] = r.ref[(size_t)(s0 + i)];
    int excl = 0;
    for (int lane = 0; lane < cvr::LANES; ++lane) {
        char *q = buf + head + excl;
        for (int j = 0; j < cvr::PER_LANE; ++j) {
            const int k = lane * cvr::PER_LANE + j;
            if (k >= cvr::NVALS) break;
            const uint32_t u = (uint32_t)(int32_t)r.v[(size_t)k];
            q += cvr::value_write(q, u, cvr::digits_u32(u));
        }
        excl += mine[lane];
        if (lane == cvr::LANES - 1) *q = '\n';
    }
    const bool same = memcmp(buf, want.data(), len) == 0;
    free(buf);
    if (!same) { fprintf(stderr, "FAIL row bytes: row %ld\n", id); return 1; }
    ++vouched;
    bytes += (long)len;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s SEED RANDOM_ROWS\n", argv[0]); return 2; }
    rng_state = strtoull(argv[1], nullptr, 10) * 2654435761ULL + 1;
    const long random_rows = strtol(argv[2], nullptr, 10);
    std::string ref;
    for (int i = 0; i < 400; ++i) ref += "ACGTNacgtn"[rnd() % 10];
    long id = 0;
    Row r;
    r.v.assign((size_t)cvr::NVALS, 0.f);
    // (a) the edges of every digit count, the predicate's borders, the specials
    const float edges[] = {0.f, -0.f, 1.f, 9.f, 10.f, 99.f, 100.f, 250.f, 999.f, 1000.f, 9999.f, 10000.f, 65535.f, 99999.f, 100000.f,
                           999999.f, 1000000.f, 9999999.f, 10000000.f, 16777215.f, 16777216.f, 16777218.f, -1.f, 0.5f, 1.5f,
                           8388607.5f, 3e38f, -3e38f, 1e-40f, from_bits(0x7f800000u), from_bits(0xff800000u), from_bits(0x7fc00000u),
                           from_bits(0xffc00001u), from_bits(0x00000001u), from_bits(0x80000001u), 2147483648.f, 4294967296.f};
    const int n_edges = (int)(sizeof edges / sizeof edges[0]);
    const int64_t centres[] = {1, 9, 17, 18, 99, 100, 383, 384, 390, 400, 417, 12345, 999999999999LL, 0, -5, INT64_MAX - 16};
    const size_t ctgs[] = {0, 1, 5, 255, 256};
    for (int e = 0; e < n_edges; ++e)
        for (int at = 0; at < 3; ++at) {                    // the edge value alone in a row of zeros: first, middle, last value
            r.ctg = "ctgA"; r.centre = 200; r.first0 = 0; r.ref = ref;
            r.v.assign((size_t)cvr::NVALS, 0.f);
            r.v[(size_t)(at == 0 ? 0 : at == 1 ? 263 : cvr::NVALS - 1)] = edges[e];
            if (check_row(id++, r)) return 1;
        }
    for (float fill : {0.f, 16777215.f, 250.f}) {            // the shortest and the longest row
        for (size_t cl : ctgs)
            for (int64_t c : centres)
                for (int64_t first0 : {(int64_t)0, (int64_t)100}) {
                    r.ctg.assign(cl, 'x'); r.centre = c; r.first0 = first0; r.ref = ref;
                    r.v.assign((size_t)cvr::NVALS, fill);
                    if (check_row(id++, r)) return 1;
                }
    }
    // (b) counts as the pileup leaves them: small whole numbers of every digit count
    for (int i = 0; i < 2000; ++i) {
        r.ctg = "chr21"; r.first0 = 50; r.ref = ref; r.centre = 50 + 17 + (int64_t)(rnd() % 400);
        for (int k = 0; k < cvr::NVALS; ++k) {
            const uint32_t d = rnd() % 9;
            uint32_t m = 1; for (uint32_t j = 0; j < d; ++j) m *= 10;
            r.v[(size_t)k] = (float)(rnd() % (m * 10 > 16777216u ? 16777216u : m * 10));
        }
        if (check_row(id++, r)) return 1;
    }
    // (c) random bit patterns: every row has values the device must hand back; the per-value checks run on all of them
    for (long i = 0; i < random_rows; ++i) {
        r.ctg = "c"; r.first0 = 0; r.ref = ref; r.centre = 17 + (int64_t)(rnd() % 400);
        for (int k = 0; k < cvr::NVALS; ++k) r.v[(size_t)k] = from_bits(rnd());
        if (i % 4 == 0)                                     // ... and exponents around the predicate's upper border
            for (int k = 0; k < cvr::NVALS; k += 2) r.v[(size_t)k] = from_bits((rnd() & 0x007fffffu) | ((127u + rnd() % 26) << 23));
        if (check_row(id++, r)) return 1;
    }
    printf("ok %ld rows, %ld on the device side, %ld bytes\n", id, vouched, bytes);
    return 0;
}
