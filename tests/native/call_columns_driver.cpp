// call_columns_driver.cpp -- the host form of csrc/cv_callcols_core.hpp (what the kernels of cv_callcols_dev.hip compute per
// centre, and cvk::host_form, the body of cv_call_columns_host_form) over a case that tests/test_call_columns_host.py
// wrote, for that test to hold to the Python definition.  Built by the test with -fsanitize=address,undefined; the inputs
// and the outputs live in heap blocks of exactly their size (the outputs: exactly the k rows and the bytes the core may
// write), so one byte read or written too far is a finding.
//
//   call_columns_driver CASE OUT
//   CASE: int64 ctg_len, n, ref_first, ref_len | ctg | centres int32 [n] | touched uint8 [n] | ref
//   OUT:  info int64 [4] | index int64 [k] | meta int64 [k,6] | text [info[1]]          -> "ok <n> centres, <k> kept, <bytes> bytes"
//
// On its own it holds the digits to printf and upper() to toupper in the C locale for every byte value.
#include <ctype.h>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../clairvoyante_amd/csrc/cv_callcols_core.hpp"

static int fail(const char *what) { fprintf(stderr, "FAIL %s\n", what); return 1; }

template <typename T> static T *exact(size_t count)          // a block of exactly count elements (one byte when empty)
{
    return (T *)malloc(count ? count * sizeof(T) : 1);
}

static bool read_all(FILE *f, void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

static int check_primitives()
{
    for (unsigned b = 0; b < 256; ++b) {
        const unsigned want = b < 128 ? (unsigned)toupper((int)b) : b;      // bytes.upper(): ASCII letters only
        if (cvk::upper(b) != want) return fail("upper");
    }
    const int64_t values[] = {1, 9, 10, 17, 99, 100, 999, 1000, 99999, 100000, 999999999, 1000000000, 2100000017, 2147483647};
    for (int64_t v : values) {
        char want[32];
        const int n = snprintf(want, sizeof want, "%" PRId64, v);
        if (cvk::digits_of(v) != n) return fail("digits_of");
        char *got = exact<char>((size_t)n);
        for (int t = 0; t < n; ++t) got[t] = cvk::digit_at(v, n, t);
        const bool same = memcmp(got, want, (size_t)n) == 0;
        free(got);
        if (!same) return fail("digit_at");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s CASE OUT\n", argv[0]); return 2; }
    if (check_primitives()) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("open case");
    int64_t head[4];
    if (!read_all(f, head, sizeof head)) return fail("read header");
    const int64_t ctg_len = head[0], n = head[1], ref_first = head[2], ref_len = head[3];
    if (ctg_len < 0 || n < 0 || ref_len < 0) return fail("header");
    char *ctg = exact<char>((size_t)ctg_len);
    int32_t *centres = exact<int32_t>((size_t)n);
    uint8_t *touched = exact<uint8_t>((size_t)n);
    uint8_t *ref = exact<uint8_t>((size_t)ref_len);
    if (!read_all(f, ctg, (size_t)ctg_len) || !read_all(f, centres, (size_t)n * 4) || !read_all(f, touched, (size_t)n) ||
        !read_all(f, ref, (size_t)ref_len))
        return fail("read case");
    fclose(f);
    // size the outputs exactly, through the per-centre core alone
    int64_t k = 0, bytes = ctg_len;
    for (int64_t i = 0; i < n; ++i) {
        const cvk::Row r = cvk::row_of(centres[i], touched[i] != 0, ref, ref_first, ref_len);
        if (!r.keep) { if (r.digits || r.wlen) return fail("a dropped row has a length"); continue; }
        if (r.digits < 1 || r.digits > cvk::MAX_DIGITS || r.wlen < cvk::FLANK + 1 || r.wlen > cvk::WIDTH) return fail("row lengths");
        if (r.w0 < 0 || r.w0 + r.wlen > ref_len) return fail("window outside the reference");
        ++k;
        bytes += r.digits + r.wlen;
    }
    if (bytes > ctg_len + cvk::MAX_ROW_TEXT * n) return fail("the bound on the text");
    int64_t *index = exact<int64_t>((size_t)k), *meta = exact<int64_t>((size_t)k * 6);
    char *text = exact<char>((size_t)bytes);
    int64_t info[4];
    cvk::host_form(ctg, ctg_len, centres, touched, n, ref, ref_first, ref_len, index, meta, text, info);
    if (info[0] != k || info[1] != bytes || info[2] != n || info[3] != 0) return fail("info");
    FILE *o = fopen(argv[2], "wb");
    if (!o) return fail("open out");
    fwrite(info, 8, 4, o);
    fwrite(index, 8, (size_t)k, o);
    fwrite(meta, 8, (size_t)k * 6, o);
    fwrite(text, 1, (size_t)bytes, o);
    if (fclose(o) != 0) return fail("write out");
    free(ctg); free(centres); free(touched); free(ref); free(index); free(meta); free(text);
    printf("ok %" PRId64 " centres, %" PRId64 " kept, %" PRId64 " bytes\n", n, k, bytes);
    return 0;
}
