// items_copy_driver.cpp -- cvb::copy_host_form of csrc/cv_beditems_core.hpp (the host form of cv_items_copy_dev) as a
// stand-alone program (tests/test_pair_route_host.py builds it with AddressSanitizer and UBSan and runs it; nothing is loaded
// into an interpreter under a sanitizer).
//
//   items_copy_driver IN OUT    IN: int64 len, the text, int64 n, int64 off[n], int64 kept_len[n], int64 out_cap.  The text,
//                               both arrays and the room sit in heap blocks of exactly their bytes, so one byte read or
//                               written beyond any of them is a finding.
//                               OUT: int64 counts[4], then the out_cap bytes of the room (0xA5 where nothing was written)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_beditems_core.hpp"

template <class T> static T take(const std::vector<uint8_t> &in, size_t *at)
{
    T v;
    memcpy(&v, in.data() + *at, sizeof v);
    *at += sizeof v;
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: items_copy_driver IN OUT\n"); return 2; }
    std::vector<uint8_t> in;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
    size_t at = 0;
    const int64_t len = take<int64_t>(in, &at);
    std::unique_ptr<uint8_t[]> text(new uint8_t[len]);
    memcpy(text.get(), in.data() + at, (size_t)len);
    at += (size_t)len;
    const int64_t n = take<int64_t>(in, &at);
    std::unique_ptr<int64_t[]> off(new int64_t[n]), kept_len(new int64_t[n]);
    for (int64_t i = 0; i < n; ++i) off[i] = take<int64_t>(in, &at);
    for (int64_t i = 0; i < n; ++i) kept_len[i] = take<int64_t>(in, &at);
    const int64_t out_cap = take<int64_t>(in, &at);
    std::unique_ptr<uint8_t[]> room(new uint8_t[out_cap]);
    memset(room.get(), 0xA5, (size_t)out_cap);
    int64_t counts[4];
    cvb::copy_host_form(text.get(), len, n, off.get(), kept_len.get(), room.get(), out_cap, counts);
    FILE *out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fwrite(counts, sizeof counts, 1, out);
    fwrite(room.get(), 1, (size_t)out_cap, out);
    fclose(out);
    printf("ok %lld rows, %lld bytes\n", (long long)n, (long long)counts[2]);
    return 0;
}
