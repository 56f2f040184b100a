// bgzf_core_driver.cpp -- the host form of the device's DEFLATE decode core (csrc/cv_inflate_core.hpp) over a file of
// members, for tests/test_bgzf_sanitized.py, which builds it with -fsanitize=address,undefined.
//   in : records  u32 len | u32 isize | u32 crc | len bytes of DEFLATE data          (little endian)
//   out: per record  u8 status (1 = OK, 2 = HOST)  [+ isize bytes when OK]
// Every member gets heap blocks of exactly its sizes, so a read or write one byte outside them is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_inflate_core.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s records results\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint32_t head[3];
    long records = 0, ok = 0;
    while (fread(head, 4, 3, in) == 3) {
        const uint32_t len = head[0], isize = head[1], crc = head[2];
        if (len > (1u << 20) || isize > (1u << 20)) { fprintf(stderr, "record %ld: sizes out of range\n", records); return 2; }
        uint8_t *data = new uint8_t[len], *text = new uint8_t[isize];
        if (len && fread(data, 1, len, in) != len) { fprintf(stderr, "record %ld: truncated\n", records); return 2; }
        memset(text, 0xA5, isize);
        const bool good = cvi::inflate_member_host(data, len, text, isize, crc);
        fputc(good ? 1 : 2, out);
        if (good) fwrite(text, 1, isize, out);
        delete[] data;
        delete[] text;
        records++; ok += good;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    fprintf(stderr, "%ld members, %ld OK\n", records, ok);
    return 0;
}
