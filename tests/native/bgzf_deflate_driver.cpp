// The device's BGZF compressor (csrc/cv_bgzf_deflate_core.hpp) in its host form, built with AddressSanitizer and UBSan by
// tests/test_bgzf_deflate_core_host.py as a stand-alone program.  Every member is judged by an inflater that is not the
// code under test -- cv_inflate_raw of csrc/cv_inflate.cpp -- with the input, the member's DEFLATE data (plus the eight
// trailer bytes the inflater may read) and the inflated bytes each in a heap block of exactly its size; header, BSIZE,
// CRC-32 and ISIZE are checked by hand, the verdicts (length and distance of every position) against the window and the
// text's end, the codes against their limits and a Kraft sum of exactly 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../clairvoyante_amd/csrc/cv_inflate.cpp"
#include "../../clairvoyante_amd/csrc/cv_bgzf_deflate_core.hpp"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case.c_str()); exit(1); } } while (0)

static std::string g_case;
static int g_members, g_kinds[3];
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_rng >> 33); }

static uint32_t crc32_plain(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

static uint32_t kraft(const uint8_t *len, int n, int limit, int *used, int *longest)
{
    uint32_t k = 0;
    *used = *longest = 0;
    for (int s = 0; s < n; s++)
        if (len[s]) { k += 1u << (limit - len[s]); ++*used; if (len[s] > *longest) *longest = len[s]; }
    return k;
}

struct Result { int kind; uint32_t size; std::vector<uint32_t> ent; int dist_codes; };

// one member of `text` through the core; -> its block type, size, verdicts
static Result one(const std::string &name, const std::string &text)
{
    static const cvi::crc_consts C = [] { cvi::crc_consts c; cvi::make_crc_consts(&c); return c; }();
    g_case = name;
    const uint32_t n = (uint32_t)text.size();
    REQUIRE(n <= cvd::BLOCK_MAX);
    uint8_t *src = (uint8_t *)malloc(n ? n : 1);                       // exactly the text
    memcpy(src, text.data(), n);
    uint32_t *ent = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
    uint8_t *slot = (uint8_t *)malloc(cvd::SLOT);
    cvd::state *S = new cvd::state;
    memset(S, 0xa5, sizeof *S);                                         // nothing may rely on a cleared state
    cvd::member(*S, src, n, ent, slot, C);
    const uint32_t size = S->size;
    const uint8_t *m = slot + cvd::MEMBER_AT;
    REQUIRE(size >= 28 && size <= n + 5 + 26 && size <= 65536);         // never larger than its stored form
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    REQUIRE(memcmp(m, head, 16) == 0 && (uint32_t)(m[16] | m[17] << 8) == size - 1);
    const uint32_t body = size - 26;
    uint8_t *comp = (uint8_t *)malloc(body + 8);                        // the DEFLATE data and the trailer behind it
    memcpy(comp, m + 18, body + 8);
    uint8_t *back = (uint8_t *)malloc(n ? n : 1);
    REQUIRE(cv_inflate_raw(comp, body, back, n) == (int64_t)n);
    REQUIRE(memcmp(back, src, n) == 0);
    uint32_t crc, isize;
    memcpy(&crc, comp + body, 4); memcpy(&isize, comp + body + 4, 4);
    REQUIRE(crc == crc32_plain(src, n) && isize == n);
    REQUIRE(S->kind >= 0 && S->kind <= 2 && ((comp[0] >> 1) & 3) == (S->kind == cvd::B_STORED ? 0 : S->kind == cvd::B_FIXED ? 1 : 2));
    Result r;
    r.kind = S->kind; r.size = size; r.ent.assign(ent, ent + n); r.dist_codes = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!(ent[i] & cvd::MATCH)) { REQUIRE(ent[i] == src[i]); continue; }
        const uint32_t len = ((ent[i] >> 16) & 0xff) + 3, dist = (ent[i] & 0xffff) + 1;
        REQUIRE(len >= 3 && len <= 258 && len <= n - i && dist >= 1 && dist <= i && dist <= 32768);
        REQUIRE(memcmp(src + i, src + i - dist, len < dist ? len : dist) == 0);
    }
    for (int s = 0; s < cvd::NDIST; s++) r.dist_codes += S->freq[cvd::NLIT + s] != 0;
    if (S->kind == cvd::B_DYNAMIC) {
        int used, longest;
        REQUIRE(kraft(S->len, cvd::NLIT, 15, &used, &longest) == 1u << 15 && used >= 2 && longest <= 15);
        REQUIRE(kraft(S->len + cvd::NLIT, cvd::NDIST, 15, &used, &longest) == 1u << 15 && used >= 2 && longest <= 15);
        REQUIRE(kraft(S->cllen, cvd::NCL, 7, &used, &longest) == 1u << 7 && used >= 2 && longest <= 7);
    }
    g_members++; g_kinds[S->kind]++;
    delete S;
    free(back); free(comp); free(slot); free(ent); free(src);
    return r;
}

// text like the data plane's: tensor rows ("0.0 " runs, a few counts) and VCF-like lines
static std::string rows(size_t n)
{
    std::string t;
    while (t.size() < n) {
        char line[96];
        snprintf(line, sizeof line, "chr%u %u ACGTTGCA", 1 + rnd() % 3, 1000000 + rnd() % 4096);
        t += line;
        for (int k = 0; k < 40; k++) {
            if (rnd() % 5) t += " 0.0";
            else { snprintf(line, sizeof line, " %u.0", rnd() % 60); t += line; }
        }
        t += "\n";
    }
    t.resize(n);
    return t;
}

static void de_bruijn(int t, int p, int k, int n, std::vector<int> &a, std::string &seq, const char *alphabet)
{
    if (t > n) {
        if (n % p == 0) for (int i = 1; i <= p; i++) seq += alphabet[a[i]];
        return;
    }
    a[t] = a[t - p];
    de_bruijn(t + 1, p, k, n, a, seq, alphabet);
    for (int j = a[t - p] + 1; j < k; j++) { a[t] = j; de_bruijn(t + 1, t, k, n, a, seq, alphabet); }
}

static void fibonacci_codes(int nsym, int limit)
{
    g_case = "fibonacci " + std::to_string(nsym);
    std::vector<uint32_t> wt(nsym);
    uint32_t a = 1, b = 1;
    for (int s = 0; s < nsym; s++) { wt[(s * 7) % nsym] = a; const uint32_t c = a + b; a = b; b = c; }    // (7 is coprime to 30 and 19)
    cvd::tree_scratch *T = new cvd::tree_scratch;
    std::vector<uint8_t> len(nsym);
    const int m = cvd::sort_used(wt.data(), nsym, *T);
    REQUIRE(m == nsym);
    cvd::build_lengths(wt.data(), nsym, m, limit, len.data(), *T);
    int used, longest;
    REQUIRE(kraft(len.data(), nsym, limit, &used, &longest) == 1u << limit && used == nsym && longest == limit);
    for (int x = 0; x < nsym; x++)
        for (int y = 0; y < nsym; y++) REQUIRE(wt[x] <= wt[y] || len[x] <= len[y]);                          // the heavier, the shorter
    delete T;
}

int main()
{
    for (size_t n = 0; n <= 300; n++) one("rows " + std::to_string(n), rows(n));
    const size_t big[] = {4095, 4096, 65279, 65280};
    for (size_t n : big) REQUIRE(one("rows " + std::to_string(n), rows(n)).kind == cvd::B_DYNAMIC);
    const size_t runs[] = {257, 258, 259, 260, 261, 516, 517};
    for (size_t n : runs) {
        const Result r = one("run " + std::to_string(n), std::string(n, 'z'));
        REQUIRE(r.ent[1] == (cvd::MATCH | (uint32_t)((n - 1 < 258 ? n - 1 : 258) - 3) << 16) && r.dist_codes == 1 && r.size < 40);
    }
    for (int period = 2; period <= 4; period++) {
        std::string t;
        for (int i = 0; i < 1000 + period; i++) t += "abcd"[i % period];
        const Result r = one("period " + std::to_string(period), t);
        REQUIRE(r.dist_codes == 1 && (r.ent[period] & 0xffff) + 1 == (uint32_t)period && r.size < 60);      // a single distance
    }
    {
        std::string t(65280, 0);
        for (char &c : t) c = (char)rnd();
        REQUIRE(one("random", t).kind == cvd::B_STORED);
        t.resize(1000);
        REQUIRE(one("random 1000", t).kind == cvd::B_STORED);
    }
    for (int far = 32768; far <= 32769; far++) {                        // the only copy of R lies exactly `far` back
        std::string R(300, 0);
        for (char &c : R) c = (char)(rnd() % 200);
        const std::string t = R + std::string((size_t)far - 300, (char)0xee) + R;
        const Result r = one("window " + std::to_string(far), t);
        const uint32_t v = r.ent[far];
        if (far == 32768) REQUIRE(v == (cvd::MATCH | (258u - 3) << 16 | (32768u - 1)) && r.size < 700);
        else REQUIRE(!(v & cvd::MATCH) && r.size > 600);               // (one() has checked every distance against the window)
    }
    {
        std::string seq;
        std::vector<int> a(3 * 6 + 1, 0);
        de_bruijn(1, 1, 6, 3, a, seq, "ACGT\t\n");
        seq += seq.substr(0, 2);                                        // 216 trigrams, each once: nothing to match
        const Result r = one("no match", seq);
        REQUIRE(seq.size() == 218 && r.kind == cvd::B_DYNAMIC && r.dist_codes == 0);
        for (uint32_t e : r.ent) REQUIRE(!(e & cvd::MATCH));
    }
    fibonacci_codes(30, 15);
    fibonacci_codes(19, 7);
    printf("ok %d members, %d stored, %d fixed, %d dynamic\n", g_members, g_kinds[0], g_kinds[1], g_kinds[2]);
    return 0;
}
