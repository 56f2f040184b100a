// inflate_tables_driver.cpp -- the tables of csrc/cv_inflate_core.hpp in its host form, for
// tests/test_deflate_foreign_host.py, which builds it with -fsanitize=address,undefined: cvi::bookkeeping and the
// lane-parallel cvi::fill over given code lengths, and cvi::symbol over every code of them.
//   in : records  288 bytes of literal/length code lengths | 32 bytes of distance code lengths
//   out: per record  u8 bookkeeping took both codes; when it did: lit[1 << LBITS] and dist[1 << DBITS] (u16 each), then
//        for every symbol with a code, literal/length first, twice (the bits behind the code all 0, all 1):
//        i16 what symbol() gave | u8 bits it used
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../clairvoyante_amd/csrc/cv_inflate_core.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s records results\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    uint8_t lens[cvi::NLIT + cvi::NDIST];
    cvi::state *S = new cvi::state;
    long records = 0;
    while (fread(lens, 1, sizeof lens, in) == sizeof lens) {
        cvi::begin(*S);
        memcpy(S->lens, lens, sizeof lens);
        const bool ok = cvi::bookkeeping(*S, 0, cvi::NLIT) && cvi::bookkeeping(*S, 1, cvi::NDIST);
        fputc(ok ? 1 : 0, out);
        records++;
        if (!ok) continue;
        memset(S->lit, 0xff, sizeof S->lit);                             // (pass 0 has to clear them)
        memset(S->dist, 0xff, sizeof S->dist);
        for (int pass = 0; pass < 2; pass++)
            for (int lane = cvi::LANES - 1; lane >= 0; lane--) cvi::fill(*S, pass, lane, cvi::LANES);
        fwrite(S->lit, sizeof(uint16_t), 1 << cvi::LBITS, out);
        fwrite(S->dist, sizeof(uint16_t), 1 << cvi::DBITS, out);
        for (int which = 0; which < 2; which++) {
            const int n = which ? cvi::NDIST : cvi::NLIT;
            const uint8_t *l = lens + (which ? cvi::NLIT : 0);
            // the canonical codes, restated: first code of each length, then in symbol order
            uint32_t next[cvi::MAXBITS + 2] = {0}, count[cvi::MAXBITS + 2] = {0};
            for (int s = 0; s < n; s++) count[l[s]]++;
            count[0] = 0;
            uint32_t code = 0;
            for (int b = 1; b <= cvi::MAXBITS; b++) { code = (code + count[b - 1]) << 1; next[b] = code; }
            for (int s = 0; s < n; s++) {
                if (!l[s]) continue;
                uint32_t c = next[l[s]]++, rev = 0;
                for (int k = 0; k < l[s]; k++) { rev = (rev << 1) | (c & 1); c >>= 1; }
                for (int junk = 0; junk < 2; junk++) {
                    S->buf = (uint64_t)rev | (junk ? ~(uint64_t)0 << l[s] : 0);
                    S->cnt = 64;
                    const int16_t got = (int16_t)cvi::symbol(*S, which);
                    const uint8_t used = (uint8_t)(64 - S->cnt);
                    fwrite(&got, sizeof got, 1, out);
                    fputc(used, out);
                }
            }
        }
    }
    delete S;
    fclose(in);
    if (fclose(out) != 0) return 2;
    fprintf(stderr, "%ld codes\n", records);
    return 0;
}
