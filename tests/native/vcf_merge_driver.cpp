// vcf_merge_driver.cpp -- csrc/cv_vcfmerge_core.hpp in its host form, as a stand-alone program for AddressSanitizer and UBSan
// (tests/test_vcf_merge_core_host.py builds and runs it; nothing of it is loaded into an interpreter).
//
//   bins     reg2bin against a restatement by levels
//   lines    line_fields over a table of records, every truncation of them and every byte of them replaced by a tab, a
//            blank, ';', 'E' and '\n', held to an independent reading (std::string, split at tabs); each line stands in a heap
//            block of exactly its length
//   copies   copy_record at all 16 x 16 phases of source and destination and a ladder of lengths; the source is a heap block
//            that ends with the 16-byte granule of the record's last byte, the tile a heap block of exactly d + len bytes
//   merge    merge_host_form + windows_host_form over random records (short ones: the tile; long ones: the wave-per-record
//            path) against std::stable_sort, memcpy and a per-record loop
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../clairvoyante_amd/csrc/cv_vcfmerge_core.hpp"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static int32_t bin_by_levels(int64_t beg, int64_t end)
{
    const int shift[5] = {14, 17, 20, 23, 26}, first[5] = {4681, 585, 73, 9, 1};
    for (int k = 0; k < 5; ++k)
        if (((end - 1) >> shift[k]) == (beg >> shift[k])) return (int32_t)(first[k] + (beg >> shift[k]));
    return 0;
}

// the definition's reading of a line -> vouched?, reflen, end
static bool reference_fields(const std::string &ln, int64_t *reflen, int64_t *end, int64_t *pos)
{
    if (ln.size() < 2 || ln.size() > 8192 || ln.back() != '\n') return false;
    std::vector<std::string> cols;
    std::string cur;
    for (size_t i = 0; i + 1 < ln.size(); ++i) {
        if (ln[i] == '\t') { cols.push_back(cur); cur.clear(); } else cur.push_back(ln[i]);
    }
    cols.push_back(cur);
    if (cols.size() < 8 || cols[0].empty() || cols[1].empty() || cols[3].empty()) return false;
    if (cols[0].find(' ') != std::string::npos) return false;
    for (char c : cols[1]) if (c < '0' || c > '9') return false;
    if (cols[1].size() > 18) return false;                           // (the item pass refuses far shorter numbers already)
    *pos = atoll(cols[1].c_str());
    const std::string &info = cols[7];
    for (size_t i = 0; i + 4 <= info.size(); ++i)
        if ((i == 0 || info[i - 1] == ';') && info.compare(i, 4, "END=") == 0) return false;
    *reflen = (int64_t)cols[3].size();
    *end = *pos - 1 + *reflen;
    return *pos >= 1 && *end <= ((int64_t)1 << 29);
}

static int64_t lines_checked = 0, lines_vouched = 0;
static void check_line(const std::string &ln)
{
    char *heap = (char *)malloc(ln.size() ? ln.size() : 1);          // exactly its length: a read past it is an error
    memcpy(heap, ln.data(), ln.size());
    int64_t reflen = 0, end = 0, pos = 0;
    const bool want = reference_fields(ln, &reflen, &end, &pos);
    // the item pass hands line_fields the position it read (pos stays 0 where the reference did not get that far)
    const cvm::Fields f = cvm::line_fields(heap, (int64_t)ln.size(), pos);
    ++lines_checked;
    if (want) {
        ++lines_vouched;
        CHECK(f.verdict == cvm::STATUS_DEVICE && f.reflen == reflen && f.end == end && f.bin == bin_by_levels(pos - 1, end), "%s", ln.c_str());
    } else {
        CHECK(f.verdict == cvm::STATUS_HOST, "vouched for: %s", ln.c_str());
    }
    free(heap);
}

static void test_lines()
{
    const char *table[] = {
        "chr1\t16384\t.\tA\tG\t51\tPASS\t.\tGT:GQ:DP:AF\t0/1:51:40:0.5000\n",
        "chr1\t16383\t.\tACGTA\tA\t33\tPASS\tLENGUESS=4\tGT:GQ:DP:AF\t1/1:33:40:0.5000\n",
        "chrUn_7\t3\t.\tC\t<INS>\t15\tLowQual\tSVTYPE=INS\tGT:GQ:DP:AF\t1/1:15:40:0.5000\n",
        "1\t536870911\t.\tAC\tA\t1\t.\t.\n",
        "1\t536870912\t.\tA\tC\t1\t.\t.\n",
        "1\t536870912\t.\tAC\tA\t1\t.\t.\n",
        "1\t0\t.\tA\tC\t1\t.\t.\n",
        "1\t5\t.\tA\tC\t1\t.\tEND=9\n",
        "1\t5\t.\tA\tC\t1\t.\tDP=3;END=9\tGT\t0/1\n",
        "1\t5\t.\tA\tC\t1\t.\tBEND=9;XEND=1\tGT\t0/1\n",
        "1\t5\t.\tA\tC\t1\t.\tEND\n",
        "1\t5\t.\t\tC\t1\t.\t.\n",
        "1\t5\t.\tA\tC\t1\t.\n",
        "1 5\t.\tA\tC\t1\t.\t.\t.\t.\n",
        "\t5\t.\tA\tC\t1\t.\t.\n",
        "a\t1\t.\tA\tC\t.\t.\t.\n",
        "\n", "x\n", "",
    };
    for (const char *t : table) {
        const std::string ln(t);
        check_line(ln);
        for (size_t cut = 0; cut < ln.size(); ++cut) {              // truncated, with and without a newline
            check_line(ln.substr(0, cut));
            check_line(ln.substr(0, cut) + "\n");
        }
        for (size_t i = 0; i < ln.size(); ++i)
            for (char c : {'\t', ' ', ';', 'E', '\n', '0'}) {
                std::string m = ln;
                m[i] = c;
                check_line(m);
            }
    }
    std::string big = "chr1\t77\t.\t" + std::string(8100, 'A') + "\tA\t1\t.\t.\n";
    check_line(big);
    check_line("chr1\t77\t.\t" + std::string(8200, 'A') + "\tA\t1\t.\t.\n");
}

static int64_t copies = 0;
static void test_copies()
{
    const int lens[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 60, 75, 90, 255, 300};
    for (int sp = 0; sp < 16; ++sp)
        for (int dp = 0; dp < 16; ++dp)
            for (int len : lens) {
                const int64_t s = 32 + sp;                          // some granules in front of the record
                const size_t src_bytes = (size_t)((s + len + 15) & ~(int64_t)15);
                unsigned char *src = (unsigned char *)aligned_alloc(16, src_bytes);
                for (size_t i = 0; i < src_bytes; ++i) src[i] = (unsigned char)(rnd() >> 24);
                const int d = 16 + dp;
                char *tile = (char *)aligned_alloc(16, (size_t)((d + len + 15) & ~15));
                char *exact = new char[d + len];                    // ... and once into a block of exactly d + len bytes
                memset(tile, 0x5a, (size_t)((d + len + 15) & ~15));
                memset(exact, 0x5a, (size_t)(d + len));
                cvm::copy_record(tile, d, src, s, len);
                cvm::copy_record(exact, d, src, s, len);
                bool same = memcmp(tile + d, src + s, (size_t)len) == 0 && memcmp(exact + d, src + s, (size_t)len) == 0;
                for (int i = 0; i < d; ++i) same = same && tile[i] == 0x5a && exact[i] == 0x5a;
                for (int i = d + len; i < ((d + len + 15) & ~15); ++i) same = same && tile[i] == 0x5a;
                CHECK(same, "copy sp=%d dp=%d len=%d", sp, dp, len);
                ++copies;
                free(src); free(tile); delete[] exact;
            }
}

static int64_t merged = 0;
static void test_merge(int n, int ref_max, int pad)
{
    // n lines over 3 named ranks; runs change whenever the contig does
    const char *ctg[3] = {"chrB", "chrA", "chrC"};
    const int32_t rank_of[3] = {1, 0, 2};
    std::string text;
    std::vector<int64_t> pos, off, len;
    std::vector<int32_t> run, run_rank;
    int last = -1;
    for (int i = 0; i < n; ++i) {
        const int c = (int)(rnd() % 3);
        if (c != last) { run_rank.push_back(rank_of[c]); last = c; }
        const int64_t p = 1 + (int64_t)(rnd() % 3 == 0 ? rnd() % 100000 : rnd() % 400000000);
        std::string ln = std::string(ctg[c]) + "\t" + std::to_string(p) + "\t.\t" + std::string(1 + rnd() % ref_max, 'G') + "\tT\t9\t.\t" +
                         std::string(1 + rnd() % (pad + 1), 'x') + "\tGT\t0/1\n";
        pos.push_back(p); off.push_back((int64_t)text.size()); len.push_back((int64_t)ln.size()); run.push_back((int32_t)run_rank.size() - 1);
        text += ln;
    }
    const int64_t text_len = (int64_t)text.size();
    char *src = (char *)aligned_alloc(16, (size_t)((text_len + 16) & ~(int64_t)15));
    memcpy(src, text.data(), (size_t)text_len);
    const int32_t nrank = 4;
    std::vector<int32_t> srank(n);
    std::vector<int64_t> sbeg(n), send(n), ooff(n + 1), chunks(4 * (size_t)n + 1), stats(4 * nrank), info(8);
    for (int shift = 0; shift < 16; shift += 5) {                   // the output at several phases
        char *out = new char[text_len + shift + 1];
        cvm::merge_host_form(src, text_len, n, pos.data(), run.data(), off.data(), len.data(), run_rank.data(), (int64_t)run_rank.size(),
                             nrank, srank.data(), sbeg.data(), send.data(), ooff.data(), out + shift, text_len, chunks.data(), stats.data(),
                             info.data());
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            const int32_t ra = run_rank[run[a]], rb = run_rank[run[b]];
            return ra != rb ? ra < rb : pos[a] < pos[b];
        });
        std::string want;
        for (int i : order) want += text.substr((size_t)off[i], (size_t)len[i]);
        CHECK(info[0] == 0 && info[2] == text_len && memcmp(out + shift, want.data(), (size_t)text_len) == 0, "merge n=%d shift=%d", n, shift);
        int64_t nchunk = 0, count[4] = {0, 0, 0, 0};
        for (int k = 0; k < n; ++k) {
            const int i = order[k];
            CHECK(srank[k] == run_rank[run[i]] && sbeg[k] == pos[i] - 1, "order at %d", k);
            ++count[srank[k]];
            if (k == 0 || srank[k] != srank[k - 1] || bin_by_levels(sbeg[k], send[k]) != bin_by_levels(sbeg[k - 1], send[k - 1])) ++nchunk;
        }
        CHECK(info[1] == nchunk, "chunks %lld, want %lld", (long long)info[1], (long long)nchunk);
        for (int64_t c = 1; c < info[1]; ++c)
            CHECK(chunks[c - 1] < chunks[c] || (chunks[c - 1] == chunks[c] && (chunks[n + c - 1] < chunks[n + c] ||
                  (chunks[n + c - 1] == chunks[n + c] && chunks[3 * n + c - 1] <= chunks[2 * n + c]))), "chunk order at %lld", (long long)c);
        for (int r = 0; r < nrank; ++r) CHECK(stats[2 * nrank + r] == count[r], "count of rank %d", r);
        // the windows
        std::vector<int64_t> win_off(nrank + 1, 0);
        for (int r = 0; r < nrank; ++r) win_off[r + 1] = win_off[r] + (count[r] ? ((stats[3 * nrank + r] - 1) >> 14) + 1 : 0);
        std::vector<int64_t> win((size_t)win_off[nrank]), want_win((size_t)win_off[nrank], INT64_MAX);
        cvm::windows_host_form(n, srank.data(), sbeg.data(), send.data(), ooff.data(), nrank, win_off.data(), win.data(), win_off[nrank]);
        for (int k = 0; k < n; ++k)
            for (int64_t w = sbeg[k] >> 14; w <= (send[k] - 1) >> 14; ++w)
                if (ooff[k] < want_win[(size_t)(win_off[srank[k]] + w)]) want_win[(size_t)(win_off[srank[k]] + w)] = ooff[k];
        for (int r = 0; r < nrank; ++r)
            for (int64_t w = win_off[r + 1] - 2; w >= win_off[r]; --w)
                if (want_win[(size_t)w] == INT64_MAX) want_win[(size_t)w] = want_win[(size_t)w + 1];
        CHECK(win == want_win, "windows n=%d", n);
        delete[] out;
        merged += n;
    }
    free(src);
}

int main()
{
    for (int k = 0; k < 200000; ++k) {
        const int64_t beg = (int64_t)(rnd() % ((1 << 29) - 70000)), end = beg + 1 + (int64_t)(rnd() % (k % 3 ? 40 : 70000));
        CHECK(cvm::reg2bin(beg, end) == bin_by_levels(beg, end), "bin of [%lld, %lld)", (long long)beg, (long long)end);
    }
    CHECK(cvm::reg2bin(0, 1) == 4681 && cvm::reg2bin(16382, 16387) == 585 && cvm::reg2bin(0, (int64_t)1 << 29) == 0, "bins");
    test_lines();
    test_copies();
    for (int n : {0, 1, 63, 64, 65, 257, 2000}) test_merge(n, 6, 3);
    test_merge(130, 400, 300);                                      // tiles past 16 KiB: the wave-per-record path
    if (fails) { fprintf(stderr, "%d checks failed\n", fails); return 1; }
    printf("ok %lld lines, %lld vouched for, %lld copies, %lld merged records\n", (long long)lines_checked, (long long)lines_vouched,
           (long long)copies, (long long)merged);
    return 0;
}
