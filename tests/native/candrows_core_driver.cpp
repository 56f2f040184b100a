// candrows_core_driver.cpp -- the host form of csrc/cv_candrows_core.hpp (what the kernels of cv_candrows_dev.hip compute
// per row, and cv_candidate_rows_host_form over a batch) checked against an independent rendering: snprintf for the
// numbers, std::stable_sort for the seven pairs.  Built by tests/test_candidate_rows_core_host.py with
// -fsanitize=address,undefined; every row is written into a heap block of exactly its length and every batch into one of
// exactly its bytes, so one byte too many is a finding.
//
//   candrows_core_driver SEED RANDOM_ENTRIES -> "ok <rows> rows, <vouched> on the device side, <bytes> bytes", exit 0
//   candrows_core_driver dump                -> the table of edge cases as text, for the tests that plant it on the GPU:
//                                               "C c0 .. c6" a count pattern, "W first0 hex" a reference window (its
//                                               bytes in hex), "G n" a contig name length
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_candrows_core.hpp"

static uint64_t rng_state;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(rng_state >> 32);
}

struct Counts { int32_t c[7]; };
struct Window { int64_t first0; std::string bytes; };

static const int32_t BIG = 2147483647;
// counts 0, 9, 10, 99, 100, 2^31 - 1; a total above 2^31; all equal; the tie pattern; a negative one (the host's)
static const Counts COUNTS[] = {
    {{0, 0, 0, 0, 0, 0, 0}},
    {{5, 5, 0, 0, 5, 0, 0}},                              // -> A 5 C 5 I 5 G 0 T 0 D 0 N 0
    {{7, 7, 7, 7, 7, 7, 7}},
    {{0, 9, 10, 99, 100, BIG, 1}},
    {{BIG, BIG, BIG, BIG, BIG, BIG, BIG}},                // total 15 032 385 529
    {{BIG, 0, 0, 2, 0, 0, BIG}},
    {{1, 2, 3, 4, 5, 6, 7}},
    {{9, 10, 9, 10, 99, 100, 99}},
    {{12, 0, 3, 12, 0, 3, 1000000000}},
    {{3, -1, 0, 0, 0, 0, 0}},
    {{0, 0, 0, 0, 0, 0, (int32_t)0x80000000}},
};
static const int N_COUNTS = (int)(sizeof COUNTS / sizeof COUNTS[0]);
static const size_t CTG_LENS[] = {1, 5, 255, 256};

// a window of 16 bytes around every power of ten up to the 10-digit positions, with the bytes a, N, 0x7F and 0x80 in it
static std::vector<Window> windows()
{
    std::vector<Window> w;
    const char pattern[17] = {'A', 'c', 'G', 't', 'a', 'N', 'n', 0x7F, (char)0x80, 'C', (char)0xFF, 'T', 'g', 'A', 'C', 'G', 0};
    w.push_back({0, std::string(pattern, 16)});
    int64_t p = 10;
    for (int k = 1; k <= 10; ++k, p *= 10) w.push_back({p - 9, std::string(pattern, 16)});   // pos0 + 1 = 10^k - 8 .. 10^k + 7
    return w;
}

static std::string name_of(size_t n)
{
    std::string s;
    for (size_t i = 0; i < n; ++i) s += (char)('a' + (i * 7 + n) % 26);
    return s;
}

// the independent rendering -> false for a row the device must hand back
static bool render(const std::string &ctg, int64_t pos0, int ref_byte, const int32_t c[7], std::string *out)
{
    if (ctg.size() > 255 || pos0 < 0 || pos0 == INT64_MAX || ref_byte < 0 || ref_byte >= 0x80) return false;
    std::vector<std::pair<char, int32_t>> v;
    int64_t total = 0;
    for (int k = 0; k < 7; ++k) {
        if (c[k] < 0) return false;
        v.emplace_back("ACGTIDN"[k], c[k]);
        total += c[k];
    }
    std::stable_sort(v.begin(), v.end(), [](const std::pair<char, int32_t> &a, const std::pair<char, int32_t> &b) { return a.second > b.second; });
    char tmp[96];
    snprintf(tmp, sizeof tmp, " %" PRId64 " %c %" PRId64, pos0 + 1, (char)ref_byte, total);
    *out = ctg + tmp;
    for (auto &x : v) {
        snprintf(tmp, sizeof tmp, " %c %d", x.first, (int)x.second);
        *out += tmp;
    }
    *out += "\n";
    return true;
}

struct Batch {
    std::string ctg;
    int64_t first0 = 0;
    std::string ref;
    std::vector<int64_t> order, pos0;
    std::vector<int32_t> counts;             // [n,7]
    bool identity = false;                    // pass a null order
};

static long rows_seen = 0, vouched = 0, bytes = 0;

static int fail(const char *what, long row)
{
    fprintf(stderr, "FAIL %s: row %ld\n", what, row);
    return 1;
}

template <class T> static T *exact(size_t n) { return (T *)malloc(n ? n * sizeof(T) : 1); }

static int check_batch(const Batch &b)
{
    const int64_t rows = (int64_t)b.order.size(), n = (int64_t)b.pos0.size();
    std::vector<std::string> want((size_t)rows);
    std::vector<bool> ok((size_t)rows);
    std::string all;
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t e = b.order[(size_t)r];
        bool v = e >= 0 && e < n;
        if (v) {
            const int64_t p = b.pos0[(size_t)e];
            const int rb = p >= b.first0 && p - b.first0 < (int64_t)b.ref.size() ? (int)(uint8_t)b.ref[(size_t)(p - b.first0)] : -1;
            v = render(b.ctg, p, rb, &b.counts[(size_t)e * 7], &want[(size_t)r]);
            if (v) {
                // the row alone, in a block of exactly its length
                const int len = cvc::row_len((int)b.ctg.size(), p, &b.counts[(size_t)e * 7]);
                if (len != (int)want[(size_t)r].size() || len > cvc::MAX_ROW) return fail("row length", rows_seen + r);
                char *dst = exact<char>((size_t)len);
                const int w = cvc::row_write(dst, b.ctg.data(), (int)b.ctg.size(), p, (uint8_t)rb, &b.counts[(size_t)e * 7]);
                const bool same = w == len && memcmp(dst, want[(size_t)r].data(), (size_t)len) == 0;
                free(dst);
                if (!same) return fail("row bytes", rows_seen + r);
            }
        }
        ok[(size_t)r] = v;
        if (v) { all += want[(size_t)r]; ++vouched; }
    }
    // the batch: lengths and status, then the text into exactly off[rows] bytes, then one byte short of the last row
    int64_t *order = exact<int64_t>((size_t)rows), *pos0 = exact<int64_t>((size_t)n), *off = exact<int64_t>((size_t)rows + 1);
    int32_t *c7 = exact<int32_t>((size_t)n * 7);
    uint8_t *status = exact<uint8_t>((size_t)rows), *ref = exact<uint8_t>(b.ref.size());
    char *ctg = exact<char>(b.ctg.size());
    if (rows) memcpy(order, b.order.data(), (size_t)rows * 8);
    if (n) { memcpy(pos0, b.pos0.data(), (size_t)n * 8); memcpy(c7, b.counts.data(), (size_t)n * 28); }
    if (!b.ref.empty()) memcpy(ref, b.ref.data(), b.ref.size());
    if (!b.ctg.empty()) memcpy(ctg, b.ctg.data(), b.ctg.size());
    const int64_t *ord = b.identity ? nullptr : order;
    int rc = 0;
    cvc::rows_host_form(ctg, (int64_t)b.ctg.size(), ord, rows, n, pos0, c7, ref, b.first0, (int64_t)b.ref.size(), off, status, nullptr, 0);
    int64_t at = 0, last = -1;
    for (int64_t r = 0; r < rows && !rc; ++r) {
        if (off[r] != at) rc = fail("offset", rows_seen + r);
        if ((status[r] == cvc::STATUS_DEVICE) != ok[(size_t)r] || status[r] > 1) rc = fail("verdict", rows_seen + r);
        at += ok[(size_t)r] ? (int64_t)want[(size_t)r].size() : 0;
        if (ok[(size_t)r]) last = r;
    }
    if (!rc && (off[rows] != at || at != (int64_t)all.size())) rc = fail("total", rows_seen + rows);
    if (!rc) {
        char *text = exact<char>((size_t)at);
        cvc::rows_host_form(ctg, (int64_t)b.ctg.size(), ord, rows, n, pos0, c7, ref, b.first0, (int64_t)b.ref.size(), off, status, text, at);
        if (memcmp(text, all.data(), (size_t)at) != 0) rc = fail("batch bytes", rows_seen);
        free(text);
    }
    if (!rc && last >= 0) {
        const int64_t keep = at - (int64_t)want[(size_t)last].size();       // the block ends where the short row would begin
        char *text = exact<char>((size_t)keep);
        cvc::rows_host_form(ctg, (int64_t)b.ctg.size(), ord, rows, n, pos0, c7, ref, b.first0, (int64_t)b.ref.size(), off, status, text, at - 1);
        if (memcmp(text, all.data(), (size_t)keep) != 0 || off[rows] != at) rc = fail("short cap", rows_seen + last);
        free(text);
    }
    free(order); free(pos0); free(off); free(c7); free(status); free(ref); free(ctg);
    rows_seen += rows;
    bytes += at;
    return rc;
}

int main(int argc, char **argv)
{
    const std::vector<Window> wins = windows();
    if (argc == 2 && strcmp(argv[1], "dump") == 0) {
        for (int i = 0; i < N_COUNTS; ++i) {
            printf("C");
            for (int k = 0; k < 7; ++k) printf(" %d", (int)COUNTS[i].c[k]);
            printf("\n");
        }
        for (auto &w : wins) {
            printf("W %" PRId64 " ", w.first0);
            for (char ch : w.bytes) printf("%02x", (unsigned)(uint8_t)ch);
            printf("\n");
        }
        for (size_t n : CTG_LENS) printf("G %zu\n", n);
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: %s SEED RANDOM_ENTRIES | dump\n", argv[0]); return 2; }
    rng_state = strtoull(argv[1], nullptr, 10) * 2654435761ULL + 1;
    const long random_entries = strtol(argv[2], nullptr, 10);
    // the tie pattern, spelled out
    {
        std::string got;
        if (!render("c", 4, 'a', COUNTS[1].c, &got) || got != "c 5 a 15 A 5 C 5 I 5 G 0 T 0 D 0 N 0\n") return fail("the reference rendering of the tie pattern", 0);
        char *dst = exact<char>(got.size());
        const int w = cvc::row_write(dst, "c", 1, 4, 'a', COUNTS[1].c);
        const bool same = w == (int)got.size() && memcmp(dst, got.data(), got.size()) == 0;
        free(dst);
        if (!same) return fail("tie pattern", 0);
    }
    // (a) every window x every position of it, one before and one behind it x every count pattern, per name length;
    //     the order: the late twins and the entries at and behind last_pos behind the others, as candidate_order gives it
    for (size_t cl : CTG_LENS)
        for (auto &w : wins) {
            Batch b;
            b.ctg = name_of(cl); b.first0 = w.first0; b.ref = w.bytes;
            const int64_t last_pos = w.first0 + 11;
            std::vector<int64_t> head, tail;
            int pat = 0;
            for (int64_t p = w.first0 - 1; p <= w.first0 + (int64_t)w.bytes.size(); ++p)
                for (int late = 0; late < 2; ++late)
                    for (int rep = 0; rep < (late ? 1 : N_COUNTS); ++rep) {
                        const int64_t e = (int64_t)b.pos0.size();
                        b.pos0.push_back(p);
                        for (int k = 0; k < 7; ++k) b.counts.push_back(COUNTS[(pat + rep) % N_COUNTS].c[k]);
                        (late == 0 && p < last_pos ? head : tail).push_back(e);
                        if (late) ++pat;
                    }
            b.order = head;
            b.order.insert(b.order.end(), tail.begin(), tail.end());
            b.order.push_back(-1);                                            // indices outside the entries: the host's
            b.order.push_back((int64_t)b.pos0.size());
            if (check_batch(b)) return 1;
        }
    // (b) positions the position test hands back, an empty window, no rows at all
    {
        Batch b;
        b.ctg = "chr1"; b.first0 = 0; b.ref = "ACGT";
        for (int64_t p : {(int64_t)-1, (int64_t)0, (int64_t)3, (int64_t)4, INT64_MAX, INT64_MAX - 1, INT64_MIN}) {
            b.order.push_back((int64_t)b.pos0.size());
            b.pos0.push_back(p);
            for (int k = 0; k < 7; ++k) b.counts.push_back(k);
        }
        b.identity = true;
        if (check_batch(b)) return 1;
        b.ref.clear();
        if (check_batch(b)) return 1;
        Batch none;
        none.ctg = "c";
        if (check_batch(none)) return 1;
    }
    // (c) random entries in batches of a few hundred, in a shuffled order, the window a little shorter than the positions
    for (long done = 0; done < random_entries;) {
        Batch b;
        b.ctg = name_of(1 + rnd() % 12);
        b.first0 = (int64_t)(rnd() % 3 ? rnd() % 2000000000u : (uint64_t)rnd() * 4u);
        const int len = 300 + (int)(rnd() % 200);
        for (int i = 0; i < len; ++i) b.ref += rnd() % 97 ? "ACGTNacgtn"[rnd() % 10] : (char)(rnd() & 255);
        const int n = 100 + (int)(rnd() % 400);
        for (int i = 0; i < n; ++i) {
            b.pos0.push_back(b.first0 + (int64_t)(rnd() % (uint32_t)(len + 6)) - 3);
            for (int k = 0; k < 7; ++k) {
                const uint32_t d = rnd() % 10;
                uint64_t m = 1; for (uint32_t j = 0; j < d; ++j) m *= 10;
                uint64_t v = rnd() % (m * 10 > 2147483648ULL ? 2147483648ULL : m * 10);
                if (rnd() % 5 == 0 && k) v = (uint64_t)b.counts.back();         // ties
                b.counts.push_back(rnd() % 4001 ? (int32_t)v : -(int32_t)(v % 1000) - 1);
            }
            b.order.push_back(i);
        }
        for (int i = n - 1; i > 0; --i) std::swap(b.order[(size_t)i], b.order[rnd() % (uint32_t)(i + 1)]);
        if (check_batch(b)) return 1;
        done += n;
    }
    printf("ok %ld rows, %ld on the device side, %ld bytes\n", rows_seen, vouched, bytes);
    return 0;
}
