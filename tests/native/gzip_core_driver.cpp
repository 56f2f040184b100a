// gzip_core_driver.cpp -- the host form of csrc/cv_gzip_core.hpp (the text the GPU runs), built by
// tests/test_gzip_core_host.py with -fsanitize=address,undefined:
//   pipeline FILE FIRST SPACING      the whole scheme on one gzip file whose DEFLATE data starts at byte FIRST: header test
//                                    at every bit offset behind evenly spaced guesses, chunks decoded into symbols with an
//                                    unknown window, the chain rule, resolution.  stdout: the text; stderr: one line
//                                    "chunks=.. decoys=.. markers=..".  Exit 2: the core does not vouch for the file.
//   fuzz FILE FIRST SEED COUNT       COUNT damaged variants of the DEFLATE data -- a flipped bit, a truncation, a random
//                                    bit offset as the chunk's start -- decoded to BFINAL with a 32 KiB window of known
//                                    bytes.  Whatever the core accepts, zlib (primed to the same bit, the same
//                                    dictionary) must accept, with the same bytes.  stderr: "accepted=.. of ..".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <zlib.h>
#include "../../clairvoyante_amd/csrc/cv_gzip_core.hpp"

static std::vector<uint8_t> slurp(const char *fn)
{
    std::vector<uint8_t> out;
    FILE *fh = fopen(fn, "rb");
    if (!fh) { perror(fn); exit(3); }
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, fh)) > 0) out.insert(out.end(), buf, buf + k);
    fclose(fh);
    return out;
}

// one chunk, counted and then written (an exact-size buffer: the sanitizer sees an overrun) -> how
static int chunk(const uint8_t *data, uint64_t n, int64_t start, int64_t end, uint32_t hist, std::vector<uint16_t> &sym, int64_t *ended)
{
    uint32_t count = 0, again = 0;
    int64_t e2 = 0;
    const int how = cvg::chunk_host(data, n, start, end, nullptr, 0, hist, &count, ended);
    if (how == cvg::BAD) return how;
    uint16_t *exact = (uint16_t *)malloc(count ? count * sizeof(uint16_t) : 1);
    const int how2 = cvg::chunk_host(data, n, start, end, exact, count, hist, &again, &e2);
    if (how2 != how || again != count || e2 != *ended) { fprintf(stderr, "the writing pass differs from the counting pass\n"); exit(1); }
    sym.assign(exact, exact + count);
    free(exact);
    return how;
}

static int pipeline(const std::vector<uint8_t> &file, int64_t first, int64_t spacing)
{
    const uint8_t *data = file.data();
    const uint64_t n = file.size() - 8;                                  // (the trailer is no DEFLATE data)
    std::vector<int64_t> found;
    for (int64_t lo = first * 8 + 1; lo < (int64_t)n * 8; ) {
        const int64_t g = (lo - first * 8) / (spacing * 8), hi = first * 8 + (g + 1) * spacing * 8;
        int64_t hit = -1;
        for (int64_t b = lo; b < hi && b < (int64_t)n * 8; b++)
            if (cvg::header_at(data, n, (uint64_t)b)) { hit = b; break; }
        if (hit >= 0) found.push_back(hit);
        lo = hi;
    }
    std::string text;
    int64_t start = first * 8, chunks = 0, decoys = 0, markers = 0;
    size_t next = 0;
    for (;;) {
        while (next < found.size() && found[next] <= start) next++;
        const int64_t end = next < found.size() ? found[next] : -1;
        std::vector<uint16_t> sym;
        int64_t ended = 0;
        const uint32_t hist = text.size() < cvg::WSIZE ? (uint32_t)text.size() : cvg::WSIZE;
        const int how = chunk(data, n, start, end, chunks ? cvg::WSIZE : hist, sym, &ended);
        if (how == cvg::BAD) return 2;
        if (how == cvg::PASSED) { decoys++; found.erase(found.begin() + (long)next); continue; }   // the chain rule: no chunk ends there
        const size_t base = text.size();
        int32_t bad = 0;
        text.resize(base + sym.size());
        for (size_t i = 0; i < sym.size(); i++) {
            markers += (sym[i] & cvg::MARK) != 0;
            text[base + i] = (char)cvg::resolve(sym[i], (const uint8_t *)text.data() + base, (int64_t)hist, &bad);
        }
        if (bad) return 2;
        chunks++;
        if (how == cvg::FINAL) break;
        start = ended;
    }
    fwrite(text.data(), 1, text.size(), stdout);
    fprintf(stderr, "chunks=%lld decoys=%lld markers=%lld\n", (long long)chunks, (long long)decoys, (long long)markers);
    return 0;
}

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static int fuzz(const std::vector<uint8_t> &file, int64_t first, uint64_t seed, int count)
{
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    std::vector<uint8_t> dict(cvg::WSIZE);
    for (auto &b : dict) b = (uint8_t)(rnd() >> 24);
    const size_t n0 = file.size() - 8 - (size_t)first;
    int accepted = 0;
    for (int it = 0; it < count; it++) {
        // an exact-size copy on the heap: reads behind the data are the sanitizer's to see
        size_t n = n0;
        const int kind = it % 3;
        if (kind == 1) n = 1 + rnd() % n0;
        uint8_t *data = (uint8_t *)malloc(n);
        memcpy(data, file.data() + first, n);
        int64_t start = 0;
        if (kind == 0) { const uint64_t bit = rnd() % (n * 8); data[bit >> 3] ^= (uint8_t)(1u << (bit & 7)); }
        if (kind == 2) start = (int64_t)(rnd() % (n * 8));
        std::vector<uint16_t> sym;
        int64_t ended = 0;
        const int how = chunk(data, n, start, -1, cvg::WSIZE, sym, &ended);
        if (how == cvg::FINAL) {
            accepted++;
            std::vector<uint8_t> mine(sym.size()), theirs(sym.size() + 1);
            int32_t bad = 0;
            // (no marker reads resolved bytes of the chunk itself: the window in front of byte 0 of `mine` is the dictionary)
            std::vector<uint8_t> both(dict);
            both.resize(dict.size() + sym.size());
            for (size_t i = 0; i < sym.size(); i++) both[dict.size() + i] = cvg::resolve(sym[i], both.data() + dict.size(), cvg::WSIZE, &bad);
            if (!sym.empty()) memcpy(mine.data(), both.data() + dict.size(), sym.size());
            z_stream z;
            memset(&z, 0, sizeof z);
            if (inflateInit2(&z, -15) != Z_OK) return 3;
            inflateSetDictionary(&z, dict.data(), (uInt)dict.size());
            const size_t base = (size_t)start >> 3;
            const int skip = (int)(start & 7);
            if (skip) inflatePrime(&z, 8 - skip, data[base] >> skip);
            z.next_in = data + base + (skip ? 1 : 0);
            z.avail_in = (uInt)(n - base - (skip ? 1 : 0));
            z.next_out = theirs.data();
            z.avail_out = (uInt)theirs.size();
            const int rc = inflate(&z, Z_FINISH);
            const bool same = rc == Z_STREAM_END && z.total_out == sym.size() && !bad && (sym.empty() || memcmp(mine.data(), theirs.data(), sym.size()) == 0);
            inflateEnd(&z);
            if (!same) {
                fprintf(stderr, "variant %d (kind %d, start %lld): the core accepted %zu bytes, zlib says %d after %lu\n", it, kind,
                        (long long)start, sym.size(), rc, (unsigned long)z.total_out);
                free(data);
                return 1;
            }
        }
        free(data);
    }
    fprintf(stderr, "accepted=%d of %d\n", accepted, count);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "pipeline")) return pipeline(slurp(argv[2]), atoll(argv[3]), atoll(argv[4]));
    if (argc == 6 && !strcmp(argv[1], "fuzz")) return fuzz(slurp(argv[2]), atoll(argv[3]), strtoull(argv[4], nullptr, 10), atoi(argv[5]));
    fprintf(stderr, "usage: %s pipeline FILE FIRST SPACING | fuzz FILE FIRST SEED COUNT\n", argv[0]);
    return 3;
}
