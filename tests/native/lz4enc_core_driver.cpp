// lz4enc_core_driver.cpp -- the host form of the device's .bin block writer (csrc/cv_lz4enc_core.hpp: the LZ4 encoder of
// one stream, the chunk's geometry, the chunk writer) over a file of records, for tests/test_lz4enc_core_host.py, which
// builds it with -fsanitize=address,undefined.  Little endian.
//   in : u8 1 | u32 n | n bytes                                  a stream
//        u8 2 | u32 typesize | u32 blocksize | u32 head_len | u32 data_len | u32 tail_len | head | data | tail    a chunk
//   out: stream: u32 c | c bytes    the LZ4 block written under the cap n - 1 (c = 0: it does not fit, stored raw)
//                u32 c | c bytes    the same under a cap no stream exceeds (n + n / 255 + 16)
//                u8 strict          1 = cvl's STRICT decoder gives the input back from every block written, 0 = it does not
//        chunk:  u32 total | total bytes   (0 = HOST: the chunk does not shrink, or is not one the device writes)
//                u8 strict          1 = cvl's plan + STRICT decoder + unshuffle give head | data | tail back (or HOST)
// Every stream, every output and every part of a chunk gets a heap block of exactly its size (the output: of exactly its
// cap), so a read or write one byte outside it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../clairvoyante_amd/csrc/cv_lz4_core.hpp"
#include "../../clairvoyante_amd/csrc/cv_lz4enc_core.hpp"

static bool rd(FILE *in, void *p, size_t n) { return n == 0 || fread(p, 1, n, in) == n; }

static bool strict_roundtrip(const uint8_t *block, uint32_t c, const uint8_t *want, uint32_t n)
{
    uint8_t *data = new uint8_t[c], *out = new uint8_t[n ? n : 1];
    memcpy(data, block, c);
    const bool ok = cvl::lz4_stream_host(data, c, out, n) && memcmp(out, want, n) == 0;
    delete[] data;
    delete[] out;
    return ok;
}

static int one_stream(FILE *in, FILE *out)
{
    uint32_t n;
    if (!rd(in, &n, 4) || n > (1u << 24)) return 2;
    uint8_t *data = new uint8_t[n ? n : 1];
    if (!rd(in, data, n)) return 2;
    cve::source src;
    src.head = src.tail = nullptr; src.head_len = src.tail_len = 0;
    src.data = data; src.data_len = n; src.base = 0; src.ne = n; src.ts = 1; src.first = 0; src.plane = -1;
    uint8_t strict = 1;
    const uint32_t caps[2] = {n ? n - 1 : 0, n + n / 255 + 16};
    for (int k = 0; k < 2; k++) {
        uint8_t *dst = new uint8_t[caps[k] ? caps[k] : 1];
        const uint32_t c = cve::encode_host(src, n, dst, caps[k]);
        if (c > caps[k]) { fprintf(stderr, "a block of %u bytes under a cap of %u\n", c, caps[k]); return 3; }
        if (c && !strict_roundtrip(dst, c, data, n)) strict = 0;
        if (k == 1 && c == 0 && n > 0 && n <= cve::STREAM_CAP) { fprintf(stderr, "a stream of %u bytes does not fit its bound\n", n); return 3; }
        fwrite(&c, 4, 1, out);
        fwrite(dst, 1, c, out);
        delete[] dst;
    }
    fputc(strict, out);
    delete[] data;
    return 0;
}

static int one_chunk(FILE *in, FILE *out)
{
    uint32_t f[5];
    if (!rd(in, f, sizeof f)) return 2;
    const uint32_t ts = f[0], blocksize = f[1], hl = f[2], dl = f[3], tl = f[4];
    if (hl > (1u << 20) || tl > (1u << 20) || dl > (1u << 24)) return 2;
    uint8_t *head = new uint8_t[hl ? hl : 1], *data = new uint8_t[dl ? dl : 1], *tail = new uint8_t[tl ? tl : 1];
    if (!rd(in, head, hl) || !rd(in, data, dl) || !rd(in, tail, tl)) return 2;
    const uint32_t nbytes = hl + dl + tl;
    cve::geometry g;
    uint32_t total = 0;
    uint8_t *chunk = nullptr;
    uint8_t strict = 1;
    if (cve::make_geometry(nbytes, ts, blocksize, g)) {
        chunk = new uint8_t[(size_t)nbytes + 16];
        total = cve::pack_chunk_host(g, head, hl, data, dl, tail, tl, chunk);
    }
    if (total) {
        // back through the device decoder's host form: the plan, the strict stream decoder, the plane lookup
        const int64_t MAX_STREAMS = 1 << 16;
        std::vector<int64_t> srows((size_t)MAX_STREAMS * cvl::STREAM_ROW);
        int64_t crow[cvl::CHUNK_ROW], ns = 0;
        uint8_t *exact = new uint8_t[total];
        memcpy(exact, chunk, total);
        bool good = cvl::plan_chunk(exact, total, 0, 0, (int64_t)nbytes, 0, MAX_STREAMS, srows.data(), crow, &ns) && (uint32_t)crow[2] == nbytes;
        uint8_t *planes = new uint8_t[nbytes];
        for (int64_t s = 0; s < ns && good; s++) {
            const int64_t *r = &srows[(size_t)s * cvl::STREAM_ROW];
            if (r[0] < 0 || r[1] < 0 || r[0] + r[1] > (int64_t)total || r[2] < 0 || r[3] < 0 || r[2] + r[3] > (int64_t)nbytes) { good = false; break; }
            uint8_t *sd = new uint8_t[r[1] ? r[1] : 1], *dst = new uint8_t[r[3] ? r[3] : 1];
            memcpy(sd, exact + r[0], (size_t)r[1]);
            if (r[4]) memcpy(dst, sd, (size_t)r[3]);
            else good = cvl::lz4_stream_host(sd, (uint32_t)r[1], dst, (uint32_t)r[3]);
            memcpy(planes + r[2], dst, (size_t)r[3]);
            delete[] sd;
            delete[] dst;
        }
        for (uint32_t k = 0; k < nbytes && good; k++) {
            const uint8_t want = k < hl ? head[k] : k < hl + dl ? data[k - hl] : tail[k - hl - dl];
            good = cvl::plane_byte(planes, k, nbytes, (uint32_t)crow[3], (uint32_t)crow[0], crow[1] != 0 && crow[0] > 1) == want;
        }
        strict = good ? 1 : 0;
        delete[] planes;
        delete[] exact;
    }
    fwrite(&total, 4, 1, out);
    if (total) fwrite(chunk, 1, total, out);
    fputc(strict, out);
    delete[] chunk;
    delete[] head;
    delete[] data;
    delete[] tail;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s records results\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    long records = 0;
    int kind;
    while ((kind = fgetc(in)) != EOF) {
        const int rc = kind == 1 ? one_stream(in, out) : kind == 2 ? one_chunk(in, out) : 2;
        if (rc) { fprintf(stderr, "record %ld: %s\n", records, rc == 2 ? "malformed or truncated" : "the core broke its contract"); return rc; }
        records++;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    fprintf(stderr, "%ld records\n", records);
    return 0;
}
