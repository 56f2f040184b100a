// lz4_core_driver.cpp -- the host form of the device's .bin block decoder (csrc/cv_lz4_core.hpp: the plan, the LZ4
// stream decoder, the plane lookup) over a file of chunks, for tests/test_blosc_core_sanitized.py, which builds it with
// -fsanitize=address,undefined.
//   in : records  u32 clen | clen bytes of a c-blosc chunk                            (little endian)
//   out: per record  u8 status (1 = OK, 2 = HOST: the plan refused the chunk or a stream was refused)
//                    [+ u32 nbytes + nbytes decompressed (unshuffled) bytes when OK]
// Every chunk, every stream and every plane gets a heap block of exactly its size, so a read or write one byte outside
// it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_lz4_core.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s records results\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    const int64_t MAX_NBYTES = 1 << 22, MAX_STREAMS = 1 << 16;
    std::vector<int64_t> srows((size_t)MAX_STREAMS * cvl::STREAM_ROW);
    uint32_t clen;
    long records = 0, ok = 0;
    while (fread(&clen, 4, 1, in) == 1) {
        if (clen > (1u << 24)) { fprintf(stderr, "record %ld: size out of range\n", records); return 2; }
        uint8_t *chunk = new uint8_t[clen];
        if (clen && fread(chunk, 1, clen, in) != clen) { fprintf(stderr, "record %ld: truncated\n", records); return 2; }
        int64_t crow[cvl::CHUNK_ROW], ns = 0;
        bool good = cvl::plan_chunk(chunk, clen, 0, 0, MAX_NBYTES, 0, MAX_STREAMS, srows.data(), crow, &ns);
        uint32_t nbytes = 0;
        uint8_t *raw = nullptr;
        if (good) {
            nbytes = (uint32_t)crow[2];
            const uint32_t blocksize = (uint32_t)crow[3], ts = (uint32_t)crow[0];
            uint8_t *planes = new uint8_t[nbytes];
            memset(planes, 0xA5, nbytes);
            for (int64_t s = 0; s < ns && good; s++) {
                const int64_t *r = &srows[(size_t)s * cvl::STREAM_ROW];
                // the stream and its output in blocks of exactly their sizes
                if (r[0] < 0 || r[1] < 0 || r[0] + r[1] > (int64_t)clen || r[2] < 0 || r[3] < 0 || r[2] + r[3] > (int64_t)nbytes) {
                    fprintf(stderr, "record %ld: the plan left its chunk\n", records);
                    return 3;
                }
                uint8_t *data = new uint8_t[r[1]], *dst = new uint8_t[r[3]];
                memcpy(data, chunk + r[0], (size_t)r[1]);
                if (r[4]) {
                    if (r[1] != r[3]) { fprintf(stderr, "record %ld: a stored stream of another size\n", records); return 3; }
                    memcpy(dst, data, (size_t)r[3]);
                } else {
                    good = cvl::lz4_stream_host(data, (uint32_t)r[1], dst, (uint32_t)r[3]);
                }
                memcpy(planes + r[2], dst, (size_t)r[3]);
                delete[] data;
                delete[] dst;
            }
            if (good) {
                raw = new uint8_t[nbytes];
                for (uint32_t k = 0; k < nbytes; k++) raw[k] = cvl::plane_byte(planes, k, nbytes, blocksize, ts, crow[1] != 0 && ts > 1);
            }
            delete[] planes;
        }
        fputc(good ? 1 : 2, out);
        if (good) {
            fwrite(&nbytes, 4, 1, out);
            fwrite(raw, 1, nbytes, out);
            // the payload rule reads the first 1 KiB only
            int64_t off = 0, len = 0;
            const uint32_t hn = nbytes < 1024 ? nbytes : 1024;
            uint8_t *head = new uint8_t[hn];
            memcpy(head, raw, hn);
            if (cvl::find_array_payload(head, nbytes, &off, &len) && (off < 0 || len < 0 || off + len > (int64_t)nbytes)) {
                fprintf(stderr, "record %ld: a payload outside the stream\n", records);
                return 3;
            }
            delete[] head;
        }
        delete[] raw;
        delete[] chunk;
        records++; ok += good;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    fprintf(stderr, "%ld chunks, %ld OK\n", records, ok);
    return 0;
}
