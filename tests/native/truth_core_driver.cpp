// truth_core_driver.cpp -- csrc/cv_truth_core.hpp as a stand-alone program (tests/test_truth_core_host.py builds it with
// AddressSanitizer and UBSan and runs it; nothing is loaded into an interpreter under a sanitizer).
//
//   IN begins with int32 format and the source of format VCF: int32 has_bounds, int64 lower, upper, int32 length + bytes of
//   the wanted contig (zeros for the other formats).
//   truth_core_driver lines IN OUT    IN: the head, int32 count, then per line int32 length + its bytes.  Every line is
//                                     copied into a heap block of exactly its length before the core sees it.
//                                     OUT: per line int32 status, ctg_off, ctg_len, int64 pos, end, float label[16]
//   truth_core_driver slab IN OUT     IN: the head, int32 max_lines, int64 length, the text.  The text and every output
//                                     array sit in heap blocks of exactly the bytes cvt::host_form may touch.
//                                     OUT: int64 info[8], then pos[rows], end[rows] (BED) or label[rows][16] (VAR),
//                                     int32 run[rows], int64 tok[runs][2]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_truth_core.hpp"

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

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: truth_core_driver lines|slab IN OUT\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[2], &in) || in.size() < 8) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    FILE *out = fopen(argv[3], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    size_t at = 0;
    const int32_t format = take<int32_t>(in, &at);
    cvt::Filter filter;                                                   // the source of format VCF (all zero otherwise)
    memset(&filter, 0, sizeof filter);
    filter.has_bounds = take<int32_t>(in, &at);
    filter.lo = take<int64_t>(in, &at);
    filter.hi = take<int64_t>(in, &at);
    filter.ctg_len = take<int32_t>(in, &at);
    if (filter.ctg_len < 0 || filter.ctg_len > cvt::MAX_CTG) { fprintf(stderr, "contig name too long\n"); return 2; }
    memcpy(filter.ctg, in.data() + at, (size_t)filter.ctg_len);
    at += (size_t)filter.ctg_len;
    if (!strcmp(argv[1], "lines")) {
        const int32_t count = take<int32_t>(in, &at);
        int64_t status[3] = {0, 0, 0};
        for (int32_t i = 0; i < count; ++i) {
            const int32_t len = take<int32_t>(in, &at);
            std::unique_ptr<uint8_t[]> line(new uint8_t[len]);           // exactly the line: one byte beyond it is a finding
            memcpy(line.get(), in.data() + at, (size_t)len);
            at += (size_t)len;
            cvt::Line L;
            for (int k = 0; k < 16; ++k) L.label[k] = -1.0f;
            cvt::verdict(line.get(), len, format, &filter, true, &L);
            cvt::Line M;                                                  // the status does not depend on want_label
            cvt::verdict(line.get(), len, format, &filter, false, &M);
            if (M.status != L.status || M.pos != L.pos || M.end != L.end || M.ctg_off != L.ctg_off || M.ctg_len != L.ctg_len) {
                fprintf(stderr, "line %d: the two forms of the verdict differ\n", i);
                return 1;
            }
            const int32_t head[3] = {L.status, L.ctg_off, L.ctg_len};
            const int64_t nums[2] = {L.pos, L.end};
            fwrite(head, sizeof head, 1, out);
            fwrite(nums, sizeof nums, 1, out);
            fwrite(L.label, sizeof L.label, 1, out);
            status[L.status]++;
        }
        printf("ok %d lines, %lld rows, %lld skipped, %lld host\n", count, (long long)status[0], (long long)status[1], (long long)status[2]);
    } else {
        const int32_t max_lines = take<int32_t>(in, &at);
        const int64_t len = take<int64_t>(in, &at);
        std::unique_ptr<uint8_t[]> text(new uint8_t[len]);
        memcpy(text.get(), in.data() + at, (size_t)len);
        // sized by what the slab holds, not by max_lines: the rows and runs the core may write
        int64_t lines = 0;
        for (int64_t i = 0; i < len && lines < max_lines; ++i) lines += text[i] == '\n';
        std::unique_ptr<int64_t[]> pos(new int64_t[lines]), end(new int64_t[format == cvt::FMT_BED ? lines : 0]), tok(new int64_t[2 * lines]);
        std::unique_ptr<float[]> label(new float[format == cvt::FMT_BED ? 0 : 16 * lines]);
        std::unique_ptr<int32_t[]> run(new int32_t[lines]);
        int64_t info[8];
        cvt::host_form(text.get(), len, format, &filter, max_lines, pos.get(), end.get(), label.get(), run.get(), tok.get(), info);
        fwrite(info, sizeof info, 1, out);
        fwrite(pos.get(), 8, (size_t)info[2], out);
        if (format == cvt::FMT_BED) fwrite(end.get(), 8, (size_t)info[2], out);
        else fwrite(label.get(), 64, (size_t)info[2], out);
        fwrite(run.get(), 4, (size_t)info[2], out);
        fwrite(tok.get(), 16, (size_t)info[5], out);
        printf("ok %lld lines, %lld rows, %lld skipped, %lld host\n", (long long)info[1], (long long)info[2], (long long)info[3], (long long)info[4]);
    }
    fclose(out);
    return 0;
}
