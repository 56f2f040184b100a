// bed_items_driver.cpp -- csrc/cv_beditems_core.hpp (and format ITEM of csrc/cv_truth_core.hpp) as a stand-alone program
// (tests/test_bed_items_core_host.py builds it with AddressSanitizer and UBSan and runs it; nothing is loaded into an
// interpreter under a sanitizer).
//
//   bed_items_driver lines IN OUT    IN: int32 count, then per line int32 length + its bytes.  Every line is copied into a
//                                    heap block of exactly its length before the core sees it.
//                                    OUT: per line int32 status, ctg_off, ctg_len, int64 pos
//   bed_items_driver slab IN OUT     IN: int32 max_lines, int32 want_text, int64 length, the text; then the BED: int32 nctg,
//                                    per contig int32 length + name, int64 bed_off[nctg + 1], int64 nb, begin[nb], emax[nb].
//                                    The text and every array sit in heap blocks of exactly the bytes the two host forms
//                                    may touch; the runs get their contig ids by comparing the run-start tokens.
//                                    OUT: int64 info[8], pos[rows], int32 run[rows], int64 off[rows], len[rows],
//                                    tok[runs][2], int32 run_ctg[runs], int64 counts[4], the kept text
//   bed_items_driver copy            cvb::copy_lane by 64 lanes at all 16 x 16 source and destination alignments and a
//                                    ladder of lengths: exact blocks on the right, a canary on the left of the destination
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_beditems_core.hpp"

static bool read_all(const char *fn, std::vector<uint8_t> *out)
{
    FILE *f = fopen(fn, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

template <class T> static T take(const std::vector<uint8_t> &in, size_t *at)
{
    T v;
    memcpy(&v, in.data() + *at, sizeof v);
    *at += sizeof v;
    return v;
}

// a heap block that ENDS with n bytes starting at an address = align modulo 16 (whatever alignment the allocator gives)
static std::unique_ptr<uint8_t[]> block_at(int64_t n, int align, int *pad)
{
    for (int p = 0; p < 16; ++p) {
        std::unique_ptr<uint8_t[]> b(new uint8_t[p + n]);
        if ((((uintptr_t)b.get() + p) & 15) == (uintptr_t)align) { *pad = p; return b; }
    }
    return nullptr;
}

static int copies()
{
    const int64_t lengths[] = {0, 1, 2, 15, 16, 17, 31, 48, 63, 64, 65, 79, 80, 81, 95, 96, 127, 128, 129, 255, 1023, 1024, 1040, 2303, 2304, 3601};
    long done = 0;
    for (int64_t n : lengths)
        for (int sa = 0; sa < 16; ++sa)
            for (int da = 0; da < 16; ++da) {
                int sp = 0, dp = 0;
                std::unique_ptr<uint8_t[]> src = block_at(n, sa, &sp), dst = block_at(n, da, &dp);
                if (!src || !dst) { fprintf(stderr, "no block at alignment %d / %d\n", sa, da); return 2; }
                for (int64_t k = 0; k < sp + n; ++k) src[k] = (uint8_t)(k * 131 + sa * 7 + 3);
                memset(dst.get(), 0xA5, (size_t)(dp + n));
                for (int lane = 0; lane < cvb::WAVE; ++lane) cvb::copy_lane(dst.get() + dp, src.get() + sp, n, lane);
                for (int k = 0; k < dp; ++k)
                    if (dst[k] != 0xA5) { fprintf(stderr, "n %lld src %d dst %d: byte %d in front of the destination changed\n", (long long)n, sa, da, k); return 1; }
                if (memcmp(dst.get() + dp, src.get() + sp, (size_t)n)) { fprintf(stderr, "n %lld src %d dst %d: the copy differs\n", (long long)n, sa, da); return 1; }
                ++done;
            }
    printf("ok %ld copies\n", done);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "copy")) return copies();
    if (argc != 4) { fprintf(stderr, "usage: bed_items_driver lines|slab IN OUT | copy\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[2], &in) || in.size() < 4) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    FILE *out = fopen(argv[3], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    size_t at = 0;
    if (!strcmp(argv[1], "lines")) {
        const int32_t count = take<int32_t>(in, &at);
        int64_t status[3] = {0, 0, 0};
        for (int32_t i = 0; i < count; ++i) {
            const int32_t len = take<int32_t>(in, &at);
            std::unique_ptr<uint8_t[]> line(new uint8_t[len]);           // exactly the line: one byte beyond it is a finding
            memcpy(line.get(), in.data() + at, (size_t)len);
            at += (size_t)len;
            cvt::Line L;
            cvt::verdict(line.get(), len, cvt::FMT_ITEM, nullptr, false, &L);
            const int32_t head[3] = {L.status, L.ctg_off, L.ctg_len};
            fwrite(head, sizeof head, 1, out);
            fwrite(&L.pos, sizeof L.pos, 1, out);
            status[L.status]++;
        }
        printf("ok %d lines, %lld rows, %lld skipped, %lld host\n", count, (long long)status[0], (long long)status[1], (long long)status[2]);
    } else {
        const int32_t max_lines = take<int32_t>(in, &at);
        const int32_t want_text = take<int32_t>(in, &at);
        const int64_t len = take<int64_t>(in, &at);
        std::unique_ptr<uint8_t[]> text(new uint8_t[len]);
        memcpy(text.get(), in.data() + at, (size_t)len);
        at += (size_t)len;
        const int32_t nctg = take<int32_t>(in, &at);
        std::vector<std::string> names;
        for (int32_t c = 0; c < nctg; ++c) {
            const int32_t l = take<int32_t>(in, &at);
            names.emplace_back((const char *)in.data() + at, (size_t)l);
            at += (size_t)l;
        }
        std::unique_ptr<int64_t[]> bed_off(new int64_t[nctg + 1]);
        for (int32_t c = 0; c <= nctg; ++c) bed_off[c] = take<int64_t>(in, &at);
        const int64_t nb = take<int64_t>(in, &at);
        std::unique_ptr<int64_t[]> begin(new int64_t[nb]), emax(new int64_t[nb]);
        for (int64_t k = 0; k < nb; ++k) begin[k] = take<int64_t>(in, &at);
        for (int64_t k = 0; k < nb; ++k) emax[k] = take<int64_t>(in, &at);
        // sized by what the slab holds, not by max_lines: the rows and runs the core may write
        int64_t lines = 0;
        for (int64_t i = 0; i < len && lines < max_lines; ++i) lines += text[i] == '\n';
        std::unique_ptr<int64_t[]> pos(new int64_t[lines]), off(new int64_t[lines]), llen(new int64_t[lines]), tok(new int64_t[2 * lines]);
        std::unique_ptr<int32_t[]> run(new int32_t[lines]);
        int64_t info[8];
        cvb::lines_host_form(text.get(), len, max_lines, pos.get(), run.get(), off.get(), llen.get(), tok.get(), info);
        const int64_t rows = info[2], runs = info[5];
        std::unique_ptr<int32_t[]> run_ctg(new int32_t[runs]);
        for (int64_t k = 0; k < runs; ++k) {
            run_ctg[k] = -1;
            const std::string name((const char *)text.get() + tok[2 * k], (size_t)tok[2 * k + 1]);
            for (int32_t c = 0; c < nctg; ++c)
                if (names[c] == name) run_ctg[k] = c;
        }
        int64_t bytes = 0;
        for (int64_t r = 0; r < rows; ++r)
            if (cvb::keep_row(pos[r], run[r], run_ctg.get(), runs, nctg, bed_off.get(), begin.get(), emax.get())) bytes += llen[r];
        std::unique_ptr<uint8_t[]> kept(new uint8_t[want_text ? bytes : 0]);
        int64_t counts[4];
        cvb::keep_host_form(text.get(), len, rows, pos.get(), run.get(), off.get(), llen.get(), run_ctg.get(), runs, nctg, bed_off.get(),
                            begin.get(), emax.get(), want_text, kept.get(), want_text ? bytes : 0, counts);
        if (want_text && counts[2] != bytes) { fprintf(stderr, "kept bytes %lld against %lld\n", (long long)counts[2], (long long)bytes); return 1; }
        fwrite(info, sizeof info, 1, out);
        fwrite(pos.get(), 8, (size_t)rows, out);
        fwrite(run.get(), 4, (size_t)rows, out);
        fwrite(off.get(), 8, (size_t)rows, out);
        fwrite(llen.get(), 8, (size_t)rows, out);
        fwrite(tok.get(), 16, (size_t)runs, out);
        fwrite(run_ctg.get(), 4, (size_t)runs, out);
        fwrite(counts, sizeof counts, 1, out);
        if (want_text) fwrite(kept.get(), 1, (size_t)bytes, out);
        printf("ok %lld lines, %lld rows, %lld skipped, %lld host\n", (long long)info[1], (long long)info[2], (long long)info[3], (long long)info[4]);
    }
    fclose(out);
    return 0;
}
