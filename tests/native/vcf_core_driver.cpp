// vcf_core_driver.cpp -- the host form of csrc/cv_vcf_core.hpp (what the kernels of cv_vcf_dev.hip compute per
// candidate) over a seeded corpus, checked against libm and against cv_format_vcf of cv_hostio.cpp, which is linked in.
// Built by tests/test_vcf_core_host.py with -ffp-contract=off -fsanitize=address,undefined; every vouched record is
// written into a heap block of exactly its length, so one byte too many is a finding.
//
//   vcf_core_driver SEED PAIRS RECORDS  ->  one "key=value ..." line per part and "ok", exit 0; "FAIL ..." on stderr, exit 1
//
// 1. the integer: over PAIRS random fp32 pairs 0 < p2 <= p1 <= 1 (and p2 == 0, p2 == p1), and over the doubles within
//    8 ulp of exp(-k / 4.343), k = 0..3000, taken as the ratio, every integer the core vouches for is libm's
//    (int)(-4.343 * log(ratio)), and the core's q stays within M/16 max(1, |q|) of libm's (M = 2^-40)
// 2. records: RECORDS random candidates (decisions, products, depth, tensors, tokens; clean and broken ones) -- a vouched
//    record is cv_format_vcf's for that candidate alone, NONE gives no bytes there, HOST names one of the header's reasons
// 3. the edges, each built by hand
#include <ctype.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/clairvoyante_amd.h"
#include "../../clairvoyante_amd/csrc/cv_vcf_core.hpp"

static char g_err[512];
void cv_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
extern "C" const char *cv_last_error(void) { return g_err; }

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(rng_state >> 32);
}
static int below(int n) { return (int)(rnd() % (uint32_t)n); }
static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static float unit_float() { return from_bits(1u + rnd() % 0x3f800000u); }          // a bit pattern of (0, 1]

// ---- 1. the integer ----------------------------------------------------------------------------------------------
static double max_dev = 0.0;

// -> 0 vouched, 1 HOST, -1 failure
static int check_ratio(double ratio, const char *what)
{
    double q;
    int qv = 0;
    const bool have = cvv::quality_value(ratio, &q);
    const bool vouched = cvv::quality_int(ratio, &qv);
    if (!have) {
        if (vouched) { fprintf(stderr, "FAIL %s: ratio %a vouched without a value\n", what, ratio); return -1; }
        return 1;
    }
    const double ql = -4.343 * log(ratio);
    const double dev = fabs(q - ql) / fmax(1.0, fabs(ql));
    if (dev > max_dev) max_dev = dev;
    if (!vouched) return 1;
    if (!(fabs(ql) < 2.0e9) || qv != (int)ql) {
        fprintf(stderr, "FAIL %s: ratio %a: the core says %d, libm's q = %.17g\n", what, ratio, qv, ql);
        return -1;
    }
    return 0;
}

static int part_integer(long pairs)
{
    long host_margin = 0, n = 0;
    for (long i = 0; i < pairs; ++i, ++n) {
        float a = unit_float(), b = unit_float();
        if (b > a) { const float t = a; a = b; b = t; }
        const int kind = below(16);
        if (kind == 0) b = 0.f;
        if (kind == 1) b = a;
        const int r = check_ratio(cvv::quality_ratio(a, b), "pair");
        if (r < 0) return 1;
        host_margin += r;
    }
    if (host_margin * 100000 > n) { fprintf(stderr, "FAIL: %ld of %ld random pairs are the host's\n", host_margin, n); return 1; }
    long built = 0, built_host = 0;
    for (int k = 0; k <= 3000; ++k) {
        const double c = exp(-(double)k / 4.343);
        double lo = c, hi = c;
        for (int s = 0; s <= 8; ++s) {
            for (int side = 0; side < (s ? 2 : 1); ++side) {
                const int r = check_ratio(side ? hi : lo, "near-integer");
                if (r < 0) return 1;
                built++; built_host += r;
            }
            lo = nextafter(lo, 0.0); hi = nextafter(hi, 2.0);
        }
    }
    const double bound = cvv::QUAL_MARGIN / 16.0;
    printf("integer pairs=%ld pairs_host=%ld built=%ld built_host=%ld max_dev=%.3e bound=%.3e\n", n, host_margin, built, built_host,
           max_dev, bound);
    if (!(max_dev <= bound)) { fprintf(stderr, "FAIL: the core's q deviates from libm's by %.3e > M/16 = %.3e\n", max_dev, bound); return 1; }
    if (built_host == 0) { fprintf(stderr, "FAIL: none of the built near-integer ratios fell inside the margin\n"); return 1; }
    return 0;
}

// ---- 2. records --------------------------------------------------------------------------------------------------
struct Cand {
    int32_t c[8]; float q[4]; std::vector<float> x; std::string ctg, pos, seq;
    int show_ref, has_qual, qual_min;
};

static long n_dev = 0, n_none = 0, n_host = 0, why_count[cvv::WHY_COUNT], text_bytes = 0;

static bool bare_digits(const std::string &s)
{
    if (s.empty() || s.size() > 18) return false;
    for (char ch : s) if (ch < '0' || ch > '9') return false;
    return true;
}
static bool decisions_ok(const Cand &k) { return (unsigned)k.c[0] <= 3u && (unsigned)k.c[1] <= 1u && (unsigned)k.c[2] <= 5u; }
static bool depth_whole(float dp) { return dp > 0.f && dp < 16777216.f && floorf(dp) == dp; }

// the two reasons the tokens and decisions do not show, derived without the core.
// The quality, from libm: the ratio is no positive normal number, q is not finite, or q lies inside the margin -- M max(1, |q|)
// around an integer, widened by the M/8 that two values within M/16 of each other can differ by; ratio == 1 is vouched for
static bool quality_is_the_hosts(float p1, float p2)
{
    const double r = ((double)p2 + 1e-300) / ((double)p1 + 1e-300);
    if (r == 1.0) return false;
    if (!(r >= 2.2250738585072014e-308 && r <= 1.7976931348623157e308)) return true;
    const double ql = -4.343 * log(r);
    if (!(fabs(ql) < 2.0e9)) return true;
    return fabs(ql - nearbyint(ql)) <= 1.125 * cvv::QUAL_MARGIN * fmax(1.0, fabs(ql));
}
// The allele fraction as vcf_record of cv_hostio.cpp forms it (the candidate has passed the tests in front of it)
static float host_af(const Cand &k)
{
    const float *x = k.x.data();
    const float dp = k.q[2];
    if (k.c[0] <= 1) {
        const char centre = (char)toupper((unsigned char)k.seq[16]);
        char ab = centre;
        if (k.c[0] == 1) { const char b1 = "ACGT"[k.c[3] & 3], b2 = "ACGT"[k.c[4] & 3]; ab = b1 != centre ? b1 : b2; }
        const int bi = (int)(strchr("ACGT", ab) - "ACGT");
        return x[(16 * 4 + bi) * 4 + 3] / dp;
    }
    const float *p = x + 17 * 16 + (k.c[0] == 2 ? 1 : 2);
    return (((p[0] + p[4]) + p[8]) + p[12]) / dp;
}

// runs the core and the host formatter over one candidate -> the core's status (-1: failure); *line = the record
static int check_cand(long id, const Cand &k, std::string *line)
{
    const std::string buf = k.ctg + k.pos + k.seq;
    const int64_t meta[6] = {0, (int64_t)k.ctg.size(), (int64_t)k.ctg.size(), (int64_t)k.pos.size(),
                             (int64_t)(k.ctg.size() + k.pos.size()), (int64_t)k.seq.size()};
    // (the tokens in a heap block of exactly their length: a read past a token's end is a finding)
    std::vector<char> heap(buf.begin(), buf.end());
    const cvv::Cand cc = cvv::candidate(k.c, k.q, k.x.data(), nullptr, heap.data(), meta, nullptr, k.show_ref, k.has_qual, k.qual_min, 0);
    cvv::Count cnt{0};
    int why = -1;
    const int st = cvv::record(cc, cnt, &why);
    char host[1024];
    int64_t host_len = 0, host_recs = 0;
    const int rc = cv_format_vcf(k.c, k.q, 1, k.x.data(), nullptr, heap.data(), meta, nullptr, k.show_ref, k.has_qual, k.qual_min, host,
                                 (int64_t)sizeof host, &host_len, &host_recs);
    if (line) line->clear();
    if (st == cvv::DEVICE) {
        char *block = (char *)malloc((size_t)cnt.n);
        cvv::Write w{block};
        int why2;
        const int st2 = cvv::record(cc, w, &why2);
        const bool same = st2 == cvv::DEVICE && w.p == block + cnt.n && rc == 0 && host_len == cnt.n && memcmp(block, host, (size_t)cnt.n) == 0;
        if (!same) {
            fprintf(stderr, "FAIL candidate %ld: the core wrote [%.*s] (%d bytes), cv_format_vcf rc %d [%.*s] %s\n", id, (int)(w.p - block), block,
                    cnt.n, rc, (int)host_len, host, rc ? g_err : "");
            free(block);
            return -1;
        }
        if (cnt.n > (int)k.ctg.size() + cvv::MAX_TAIL) { fprintf(stderr, "FAIL candidate %ld: %d bytes exceed the bound\n", id, cnt.n); free(block); return -1; }
        if (line) line->assign(block, (size_t)cnt.n);
        free(block);
        n_dev++; text_bytes += cnt.n;
    } else if (st == cvv::NONE) {
        if (rc != 0 || host_len != 0) { fprintf(stderr, "FAIL candidate %ld: NONE, but cv_format_vcf rc %d, %ld bytes\n", id, rc, (long)host_len); return -1; }
        n_none++;
    } else if (st == cvv::HOST) {
        bool holds;
        switch (why) {
        case cvv::WHY_DECISION: holds = !decisions_ok(k); break;
        case cvv::WHY_QUALITY: holds = quality_is_the_hosts(k.q[0], k.q[1]); break;
        case cvv::WHY_DEPTH: holds = !depth_whole(k.q[2]) && k.q[2] != 0.f; break;
        case cvv::WHY_CONTIG: holds = k.ctg.size() > 255; break;
        case cvv::WHY_POSITION: holds = !bare_digits(k.pos); break;
        case cvv::WHY_SEQUENCE: holds = k.seq.size() <= 16; break;
        case cvv::WHY_CENTRE: holds = k.c[0] == 0 && !strchr("ACGTacgt", k.seq[16]); break;
        case cvv::WHY_AF: holds = !(fabs((double)host_af(k)) < 1e9); break;
        default: holds = false;
        }
        if (!holds) { fprintf(stderr, "FAIL candidate %ld: HOST for reason %d, which does not hold\n", id, why); return -1; }
        n_host++; why_count[why]++;
    } else {
        fprintf(stderr, "FAIL candidate %ld: status %d\n", id, st);
        return -1;
    }
    return st;
}

static const char ACGT[] = "ACGTacgtACGTACGTN";

static Cand clean_cand()
{
    Cand k;
    k.c[0] = below(4); k.c[1] = below(2); k.c[2] = below(6); k.c[3] = below(4); k.c[4] = below(4); k.c[5] = k.c[6] = k.c[7] = 0;
    float a = unit_float(), b = unit_float();
    if (b > a) { const float t = a; a = b; b = t; }
    k.q[0] = a; k.q[1] = b; k.q[3] = 0.f;
    const int dk = below(8);
    k.q[2] = dk == 0 ? 1.f : dk == 1 ? 16777215.f : dk < 5 ? (float)(1 + below(60)) : (float)(1 + rnd() % 16777215u);
    k.x.resize(cvv::ROW);
    const int xk = below(4);
    for (float &v : k.x) v = xk == 0 ? (float)(below(9) - 4) : xk == 1 ? (float)(below(300) - 100) : xk == 2 ? (float)(below(40)) : (float)(below(2000) - 1000) * 0.25f;
    const int cl = 1 + below(below(8) ? 12 : 255);
    for (int i = 0; i < cl; ++i) k.ctg.push_back((char)('!' + below(90)));
    const int pl = 1 + below(below(6) ? 9 : 18);
    for (int i = 0; i < pl; ++i) k.pos.push_back((char)('0' + below(10)));
    const int sl = below(4) ? 33 : 17 + below(24);
    for (int i = 0; i < sl; ++i) k.seq.push_back(ACGT[below(below(10) ? 16 : 17)]);
    k.show_ref = below(2); k.has_qual = below(2); k.qual_min = below(60);
    return k;
}

static void break_cand(Cand &k)
{
    static const uint32_t odd[] = {0x7fc00000u, 0x7f800000u, 0xff800000u, 0x80000000u, 0x00000001u, 0xbf800000u, 0x7f7fffffu, 0u};
    switch (below(12)) {
    case 0: k.c[below(3)] = below(2) ? -1 - below(5) : 6 + below(100); break;
    case 1: k.q[below(2)] = from_bits(odd[below(8)]); break;
    case 2: k.q[0] = from_bits(rnd()); k.q[1] = from_bits(rnd()); break;
    case 3: k.q[2] = from_bits(odd[below(8)]); break;
    case 4: k.q[2] = below(2) ? (float)below(100) + 0.5f : from_bits(rnd()); break;
    case 5: for (float &v : k.x) v = from_bits(rnd()); break;
    case 6: k.x[(size_t)below(cvv::ROW)] = from_bits(odd[below(8)]); k.x[(size_t)(16 * 16 + below(32))] = from_bits(odd[below(8)]); break;
    case 7: { static const char *bad[] = {"", "+12", "-7", " 12", "12 ", "12\r", "1234567890123456789", "1x", "\t5"}; k.pos = bad[below(9)]; break; }
    case 8: k.seq.resize((size_t)below(17)); break;
    case 9: k.ctg.assign((size_t)(256 + below(40)), 'c'); break;
    case 10: k.seq[16] = "NnRx*"[below(5)]; break;
    default: k.q[2] = 0.f; break;
    }
}

static int part_records(long records)
{
    long eligible = 0, eligible_dev = 0;
    for (long i = 0; i < records; ++i) {
        Cand k = clean_cand();
        const bool broken = below(10) < 3;
        if (broken) break_cand(k);
        const int st = check_cand(i, k, nullptr);
        if (st < 0) return 1;
        if (decisions_ok(k) && depth_whole(k.q[2]) && bare_digits(k.pos) && k.seq.size() > 16 && k.ctg.size() <= 255 && (k.c[0] != 0 || k.show_ref)) {
            eligible++;
            eligible_dev += st == cvv::DEVICE;
        }
    }
    printf("records n=%ld device=%ld none=%ld host=%ld decision=%ld quality=%ld depth=%ld contig=%ld position=%ld sequence=%ld centre=%ld af=%ld "
           "eligible=%ld eligible_device=%ld bytes=%ld\n", records, n_dev, n_none, n_host, why_count[cvv::WHY_DECISION], why_count[cvv::WHY_QUALITY],
           why_count[cvv::WHY_DEPTH], why_count[cvv::WHY_CONTIG], why_count[cvv::WHY_POSITION], why_count[cvv::WHY_SEQUENCE],
           why_count[cvv::WHY_CENTRE], why_count[cvv::WHY_AF], eligible, eligible_dev, text_bytes);
    if (eligible_dev * 10 < eligible * 9) { fprintf(stderr, "FAIL: only %ld of %ld clean candidates are vouched\n", eligible_dev, eligible); return 1; }
    return 0;
}

// ---- 3. the edges ------------------------------------------------------------------------------------------------
static Cand plain_cand(int varType)
{
    Cand k;
    const int32_t c[8] = {varType, 0, 2, 1, 2, 0, 0, 0};
    memcpy(k.c, c, sizeof c);
    k.q[0] = 0.75f; k.q[1] = 0.001f; k.q[2] = 32.f; k.q[3] = 0.f;
    k.x.assign(cvv::ROW, 0.f);
    k.ctg = "chr1"; k.pos = "100017"; k.seq = "ACGTACGTACGTACGTACGTACGTACGTACGTA";
    k.show_ref = 1; k.has_qual = 1; k.qual_min = 10;
    return k;
}
// matrix `mat` passes the length threshold at the first `inferred` positions behind the centre
static void plant_length(Cand &k, int mat, int inferred)
{
    k.c[2] = 5;
    for (int p = 17; p < 33; ++p)
        for (int b = 0; b < 4; ++b) { k.x[(size_t)(p * 16 + b * 4 + 0)] = 2.f; k.x[(size_t)(p * 16 + b * 4 + mat)] = p < 17 + inferred ? (b == 2 ? 3.f : 1.f) : 0.f; }
}

static long n_edges = 0;
static int edge(const char *name, const Cand &k, int want, const char *holds)
{
    std::string line;
    const int st = check_cand(-1, k, &line);
    if (st < 0) { fprintf(stderr, "(edge %s)\n", name); return 1; }
    if (st != want) { fprintf(stderr, "FAIL edge %s: status %d, expected %d\n", name, st, want); return 1; }
    if (holds && line.find(holds) == std::string::npos) { fprintf(stderr, "FAIL edge %s: [%s] lacks [%s]\n", name, line.c_str(), holds); return 1; }
    n_edges++;
    return 0;
}

static int part_edges()
{
    const int D = cvv::DEVICE, H = cvv::HOST, N = cvv::NONE;
    int bad = 0;
    Cand k;
    // "%.4f" ties: odd multiples of 1/32 are the fp32 quotients whose 10^4-fold ends in .5
    k = plain_cand(1); k.x[(16 * 4 + 1) * 4 + 3] = 1.f; bad |= edge("af 1/32", k, D, ":0.0312\n");
    k.x[(16 * 4 + 1) * 4 + 3] = 3.f; bad |= edge("af 3/32", k, D, ":0.0938\n");
    k.x[(16 * 4 + 1) * 4 + 3] = 5.f; bad |= edge("af 5/32", k, D, ":0.1562\n");
    k.x[(16 * 4 + 1) * 4 + 3] = 7.f; bad |= edge("af 7/32", k, D, ":0.2188\n");
    k.x[(16 * 4 + 1) * 4 + 3] = -1.f; bad |= edge("af -1/32", k, D, ":-0.0312\n");
    k.x[(16 * 4 + 1) * 4 + 3] = 1.f; k.q[2] = 20000.f; bad |= edge("af 1/20000", k, D, nullptr);
    k.x[(16 * 4 + 1) * 4 + 3] = 3.f; bad |= edge("af 3/20000", k, D, nullptr);
    k.x[(16 * 4 + 1) * 4 + 3] = 1.f; k.q[2] = 6667.f; bad |= edge("af 1/6667", k, D, nullptr);
    k = plain_cand(1); k.x[(16 * 4 + 1) * 4 + 3] = -0.f; bad |= edge("af -0", k, D, ":-0.0000\n");
    k.x[(16 * 4 + 1) * 4 + 3] = -1.f; k.q[2] = 16777215.f; bad |= edge("af tiny negative, dp 2^24-1", k, D, ":16777215:-0.0000\n");
    k.x[(16 * 4 + 1) * 4 + 3] = 3.e38f; k.q[2] = 1.f; bad |= edge("af absurd", k, H, nullptr);
    k.x[(16 * 4 + 1) * 4 + 3] = NAN; bad |= edge("af NaN", k, H, nullptr);
    k = plain_cand(1); k.q[2] = 1.f; k.x[(16 * 4 + 1) * 4 + 3] = 1.f; bad |= edge("dp 1", k, D, ":1:1.0000\n");
    k.q[2] = 16777216.f; bad |= edge("dp 2^24", k, H, nullptr);
    k.q[2] = 2.5f; bad |= edge("dp fractional", k, H, nullptr);
    k.q[2] = -3.f; bad |= edge("dp negative", k, H, nullptr);
    k.q[2] = 0.f; bad |= edge("dp 0", k, N, nullptr);
    k.q[2] = -0.f; bad |= edge("dp -0", k, N, nullptr);
    // lengths
    for (int vt = 2; vt <= 3; ++vt) {
        k = plain_cand(vt); k.c[2] = 0; bad |= edge("varLength 0", k, D, vt == 2 ? "\tA\tAA\t" : "\tAC\tA\t");
        k = plain_cand(vt); plant_length(k, vt - 1, 4); bad |= edge("inferred 4", k, D, "LENGUESS=4\t");
        k = plain_cand(vt); plant_length(k, vt - 1, 15); bad |= edge("inferred 15", k, D, "LENGUESS=15\t");
        k = plain_cand(vt); plant_length(k, vt - 1, 16); bad |= edge("inferred 16", k, D, vt == 2 ? "\t<INS>\t" : "\t<DEL>\t");
        bad |= edge("inferred 16 svtype", k, D, vt == 2 ? "\tSVTYPE=INS\t" : "\tSVTYPE=DEL\t");
    }
    k = plain_cand(2); plant_length(k, 1, 15); bad |= edge("inserted bases", k, D, "\tAGGGGGGGGGGGGGGG\t");
    // the slice of a deletion, clipped by the sequence
    k = plain_cand(3); k.c[2] = 3; k.seq.resize(17); bad |= edge("seq 17, deletion of 3", k, D, "\t.\tA\tA\t");
    k = plain_cand(3); plant_length(k, 2, 15); k.seq.resize(21); bad |= edge("seq 21, deletion of 15", k, D, "\t.\tACGTA\tA\t");
    k = plain_cand(3); plant_length(k, 2, 15); bad |= edge("seq 33, deletion of 15", k, D, "\t.\tACGTACGTACGTACGT\tA\t");
    k.seq.resize(16); bad |= edge("seq 16", k, H, nullptr);
    k = plain_cand(3); k.c[2] = 4; k.seq = "acgtacgtacgtacgtacgtacgtacgtacgta"; bad |= edge("lower case", k, D, "\t.\tACGTA\tA\t");
    k = plain_cand(0); k.seq = "acgtacgtacgtacgtacgtacgtacgtacgta"; bad |= edge("lower-case centre, REF", k, D, "\tA\tA\t");
    k.seq[16] = 'N'; bad |= edge("centre N, REF", k, H, nullptr);
    k.c[0] = 2; bad |= edge("centre N, INS", k, D, "\tN\tNAA\t");
    k = plain_cand(0); k.show_ref = 0; bad |= edge("REF without show_ref", k, N, nullptr);
    // tokens
    k = plain_cand(1); k.ctg = "7"; bad |= edge("contig of 1", k, D, nullptr);
    k.ctg.assign(255, 'q'); bad |= edge("contig of 255", k, D, nullptr);
    k.ctg.assign(256, 'q'); bad |= edge("contig of 256", k, H, nullptr);
    k = plain_cand(1); k.pos = "007"; bad |= edge("leading zeros", k, D, "\t7\t.\t");
    k.pos = "999999999999999999"; bad |= edge("18 digits", k, D, "\t999999999999999999\t");
    k.pos = "1234567890123456789"; bad |= edge("19 digits", k, H, nullptr);
    k.pos = "+5"; bad |= edge("sign", k, H, nullptr);
    k.pos = "-5"; bad |= edge("minus", k, H, nullptr);
    k.pos = " 5"; bad |= edge("blank", k, H, nullptr);
    k.pos = "5\r"; bad |= edge("carriage return", k, H, nullptr);
    k.pos = ""; bad |= edge("empty position", k, H, nullptr);
    // quality
    k = plain_cand(1); k.q[1] = k.q[0]; bad |= edge("p2 == p1", k, D, "\t0\tLowQual\t");
    k.q[1] = 0.f; bad |= edge("p2 == 0", k, D, "\t2998\tPASS\t");
    k.has_qual = 0; bad |= edge("no --qual", k, D, "\t2998\t.\t");
    k = plain_cand(1); k.q[0] = 0.001f; k.q[1] = 0.75f; bad |= edge("negative quality", k, D, "\t-28\tLowQual\t");
    for (int dp0 = 0; dp0 < 2; ++dp0) {
        k = plain_cand(1); if (dp0) k.q[2] = 0.f;
        k.q[0] = NAN; bad |= edge("p1 NaN", k, H, nullptr);
        k.q[0] = 0.5f; k.q[1] = NAN; bad |= edge("p2 NaN", k, H, nullptr);
        k.q[1] = INFINITY; bad |= edge("p2 Inf", k, H, nullptr);
        k.q[0] = INFINITY; k.q[1] = 0.5f; bad |= edge("p1 Inf", k, H, nullptr);
        k.q[0] = -0.5f; bad |= edge("p1 negative", k, H, nullptr);
    }
    // decisions
    k = plain_cand(1); k.c[0] = 4; bad |= edge("varType 4", k, H, nullptr);
    k.c[0] = -1; bad |= edge("varType -1", k, H, nullptr);
    k = plain_cand(1); k.c[1] = 2; bad |= edge("zygosity 2", k, H, nullptr);
    k = plain_cand(1); k.c[2] = 6; bad |= edge("length 6", k, H, nullptr);
    k = plain_cand(1); k.c[1] = 1; bad |= edge("1/1", k, D, "\t1/1:");
    printf("edges n=%ld\n", n_edges);
    return bad;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: vcf_core_driver SEED PAIRS RECORDS\n"); return 2; }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9e3779b97f4a7c15ULL + 1;
    if (part_integer(atol(argv[2]))) return 1;
    if (part_records(atol(argv[3]))) return 1;
    if (part_edges()) return 1;
    printf("ok\n");
    return 0;
}
