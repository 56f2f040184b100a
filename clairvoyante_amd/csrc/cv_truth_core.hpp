// cv_truth_core.hpp -- one line of a truth list or of a BED file, as utils_v2._read_bed_truth reads it and utils_v2._label
// labels it.  The SAME text compiles for the device (cv_truth_dev.hip) and for the host (cv_truth_lines_host_form;
// tests/native/truth_core_driver.cpp runs it under AddressSanitizer / UBSan over heap blocks of exactly a line's bytes).
//
// The definition reads the file as text (ASCII, errors="replace", universal newlines) and splits each line with
// str.split().  That splits at \t \n \v \f \r, space and \x1c..\x1f too, and a byte >= 0x80 becomes U+FFFD; so a line is
// vouched for only when every byte of it is 0x21..0x7E, space or tab.  The verdict is one of
//   ROW   the definition makes a row of the line, and these are its fields;
//   SKIP  the definition skips the line (no token);
//   HOST  only the definition can answer: a byte outside the set above (a '\r' moves the line ends), a line longer than
//         LINE_CAP, too few tokens (IndexError there), an integer that is not canonical decimal (int() takes "+5", "007",
//         "1_0"; the tables key on str(int(...))), a contig token with ':', a first base outside ACGT where _label looks it
//         up (KeyError there).
// Vouching for too little is safe: one HOST line sends the whole call to the definition.
//
// Format VCF is a line of a truth VCF under the rules of GetTruth.variant_rows for ONE source -- `filter`: the wanted contig
// and GetTruth's bounds --, evaluated in its order: SKIP when the
// line is blank, when its first token starts with '#' or is not the wanted contig (whatever else the line holds: the
// byte rule covers the first token only); SKIP when the position lies outside the bounds (the byte rule covers two
// tokens); the genotype is the last column up to its first ':' and must be one digit or '.', '/' or '|', one digit or
// '.'; p1 <= p2; for 1|2 with a ',' in ALT the genotype becomes 0|1 and ALT the first of its shortest alleles (shorter than
// 99, not empty); then the label of (REF, ALT, p1, p2) as for format VAR.  GetTruth reads bytes and splits at ASCII
// whitespace; its row then passes through the truth list's reader, so from the position on the whole line is held to the
// byte rule above.
//
// Format ITEM is a line of any file whose first two columns are contig and position (bed_items.choose_items_host: a text
// tensor, a truth list), read as bytes: a ROW needs two tokens, the second canonical decimal; nothing behind them is
// looked at beyond the byte rule.  There is no SKIP: a line without a token is the definition's IndexError, so HOST.  The
// contig token is compared byte for byte and never becomes part of a key, so a ':' in it is no concern.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CVT_FN __host__ __device__ inline
#else
#define CVT_FN inline
#endif

namespace cvt {

enum { ROW = 0, SKIP = 1, HOST = 2 };
enum { FMT_VAR = 0, FMT_BED = 1, FMT_VCF = 2, FMT_ITEM = 3 };
constexpr int LINE_CAP = 8192;
constexpr int MAX_DIGITS = 12;                  // utils_v2.canonical_coordinate

constexpr int MAX_CTG = 256;                    // bytes of a wanted contig's name (format VCF)

struct Filter {                                 // one source of format VCF
    int64_t has_bounds, lo, hi, ctg_len;
    uint8_t ctg[MAX_CTG];
};

struct Line {
    int status;
    int32_t ctg_off, ctg_len;                   // the contig token inside the line
    int64_t pos;                                // VAR: the position; BED: begin
    int64_t end;                                // BED: int(tok2) - 1, + 1 when that equals begin
    float label[16];                            // VAR: _label(row)
};

CVT_FN bool blank(unsigned b) { return b == ' ' || b == '\t'; }

// token k >= 0 of line[0, n): its span, false when the line has no such token.  `from` = where to start looking,
// moved behind the token found (tokens are asked for in ascending order)
CVT_FN bool next_token(const uint8_t *line, int n, int *from, int *off, int *len)
{
    int i = *from;
    while (i < n && blank(line[i])) ++i;
    if (i >= n) { *from = i; return false; }
    const int s = i;
    while (i < n && !blank(line[i])) ++i;
    *off = s; *len = i - s; *from = i;
    return true;
}

// utils_v2.canonical_coordinate: digits only, no leading zero unless "0", 1 .. 12 digits
CVT_FN bool canonical(const uint8_t *t, int len, int64_t *v)
{
    if (len < 1 || len > MAX_DIGITS || (len > 1 && t[0] == '0')) return false;
    int64_t a = 0;
    for (int k = 0; k < len; ++k) {
        const unsigned d = (unsigned)t[k] - '0';
        if (d > 9) return false;
        a = a * 10 + (int64_t)d;
    }
    *v = a;
    return true;
}

// base2num: A,C,G,T -> 0..3, anything else -1 (KeyError in the definition)
CVT_FN int base_of(unsigned b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1; }

// _label over (ref, alt, g1, g2) -> false where the definition raises KeyError
CVT_FN bool label_of(const uint8_t *ref, int rl, const uint8_t *alt, int al, const uint8_t *g1, int g1l, const uint8_t *g2, int g2l,
                     float *v)
{
    for (int k = 0; k < 16; ++k) v[k] = 0.0f;
    const bool snp_like = rl == 1 && al == 1;
    const bool second_one = g2l == 1 && g2[0] == '1';
    if (g1l == 1 && g1[0] == '0' && second_one) {
        const int r = base_of(ref[0]);
        if (r < 0) return false;
        if (snp_like) {
            const int a = base_of(alt[0]);
            if (a < 0) return false;
            v[r] = 0.5f;
            v[a] = 0.5f;
        } else {
            v[r] = 0.5f;
        }
        v[4] = 1.0f;
    } else if (g1l == 1 && g1[0] == '1' && second_one) {
        if (snp_like) {
            const int a = base_of(alt[0]);
            if (a < 0) return false;
            v[a] = 1.0f;
        }
        v[5] = 1.0f;
    }
    if (rl > 1 && al == 1) v[9] = 1.0f;
    else if (al > 1 && rl == 1) v[8] = 1.0f;
    else v[7] = 1.0f;
    const int d = rl > al ? rl - al : al - rl;
    v[d > 4 ? 15 : 10 + d] = 1.0f;
    return true;
}

// format VCF behind the contig and position tests: line[0, n) holds only vouched bytes, `from` is behind the second token
CVT_FN void verdict_vcf(const uint8_t *line, int n, int from, bool want_label, Line *out)
{
    int off[5], len[5], last_off = 0, last_len = 0, ntok = 2;
    int o, l;
    while (next_token(line, n, &from, &o, &l)) {
        if (ntok < 5) { off[ntok] = o; len[ntok] = l; }
        last_off = o; last_len = l;
        ++ntok;
    }
    if (ntok < 5) return;                                        // row[3] / row[4]: IndexError there
    int g = 0;
    while (g < last_len && line[last_off + g] != ':') ++g;
    if (g != 3) return;
    const unsigned c0 = line[last_off], c1 = line[last_off + 1], c2 = line[last_off + 2];
    if (c1 != '/' && c1 != '|') return;
    int p1 = c0 == '.' ? 0 : (int)c0 - '0', p2 = c2 == '.' ? 0 : (int)c2 - '0';
    if (p1 < 0 || p1 > 9 || p2 < 0 || p2 > 9) return;
    if (p1 > p2) { const int t = p1; p1 = p2; p2 = t; }
    int alt_off = off[4], alt_len = len[4];
    bool comma = false;
    for (int k = 0; k < len[4]; ++k) comma = comma || line[off[4] + k] == ',';
    if (p1 == 1 && p2 == 2 && comma) {
        p1 = 0; p2 = 1;
        int best = 99, best_off = 0, s = off[4];
        bool found = false;
        for (int k = off[4]; k <= off[4] + len[4]; ++k) {
            if (k < off[4] + len[4] && line[k] != ',') continue;
            if (k - s < best) { best = k - s; best_off = s; found = true; }
            s = k + 1;
        }
        if (!found || best == 0) return;                         // no allele shorter than 99, or an empty one: five tokens there
        alt_off = best_off; alt_len = best;
    }
    const uint8_t g1 = (uint8_t)('0' + p1), g2 = (uint8_t)('0' + p2);
    float scratch[16];
    if (!label_of(line + off[3], len[3], line + alt_off, alt_len, &g1, 1, &g2, 1, want_label ? out->label : scratch)) return;
    out->status = ROW;
}

// the verdict over line[0, n) (without its newline); want_label = false leaves label alone (the status is the same);
// filter: format VCF only
CVT_FN void verdict(const uint8_t *line, int64_t n64, int format, const Filter *filter, bool want_label, Line *out)
{
    out->status = HOST;
    out->ctg_off = 0; out->ctg_len = 0; out->pos = 0; out->end = 0;
    if (format == FMT_VCF) {
        // the first token decides first, over its own bytes alone (a line of any length)
        int64_t i = 0;
        while (i < n64 && blank(line[i])) ++i;
        if (i >= n64) { out->status = SKIP; return; }
        if (line[i] == '#') { out->status = SKIP; return; }
        const int64_t s = i;
        while (i < n64 && !blank(line[i])) {
            if (line[i] < 0x21 || line[i] > 0x7E) return;
            ++i;
        }
        const uint8_t *want = filter->ctg;
        bool same = i - s == filter->ctg_len;
        for (int64_t k = 0; same && k < filter->ctg_len; ++k) same = line[s + k] == want[k];
        if (!same) { out->status = SKIP; return; }
        // the position, over the bytes up to its end
        while (i < n64 && blank(line[i])) ++i;
        const int64_t ps = i;
        while (i < n64 && !blank(line[i])) {
            if (line[i] < 0x21 || line[i] > 0x7E) return;
            ++i;
        }
        int64_t a = 0;
        if (i - ps > MAX_DIGITS || !canonical(line + ps, (int)(i - ps), &a)) return;
        if (filter->has_bounds && (a < filter->lo || a > filter->hi)) { out->status = SKIP; return; }
        if (n64 > LINE_CAP) return;
        for (int64_t k = i; k < n64; ++k)
            if (!blank(line[k]) && (line[k] < 0x21 || line[k] > 0x7E)) return;
        for (int64_t k = s; k < s + filter->ctg_len; ++k)
            if (line[k] == ':') return;
        out->ctg_off = (int32_t)s; out->ctg_len = (int32_t)filter->ctg_len; out->pos = a;
        verdict_vcf(line, (int)n64, (int)i, want_label, out);
        if (out->status != ROW) { out->ctg_off = 0; out->ctg_len = 0; out->pos = 0; }
        return;
    }
    if (n64 > LINE_CAP) return;
    const int n = (int)n64;
    bool any = false;
    for (int k = 0; k < n; ++k) {
        const unsigned b = line[k];
        if (blank(b)) continue;
        if (b < 0x21 || b > 0x7E) return;
        any = true;
    }
    if (!any) { if (format != FMT_ITEM) out->status = SKIP; return; }
    int from = 0, off[6], len[6];
    const int need = format == FMT_BED ? 3 : format == FMT_ITEM ? 2 : 6;
    for (int t = 0; t < need; ++t)
        if (!next_token(line, n, &from, &off[t], &len[t])) return;
    for (int k = 0; format != FMT_ITEM && k < len[0]; ++k)
        if (line[off[0] + k] == ':') return;                     // utils_v2.contig_token_ok (NUL and >= 0x80 went above)
    int64_t a = 0, b = 0;
    if (!canonical(line + off[1], len[1], &a)) return;
    if (format == FMT_BED) {
        if (!canonical(line + off[2], len[2], &b)) return;
        b -= 1;
        if (b == a) b += 1;
    } else if (format != FMT_ITEM) {
        float scratch[16];
        if (!label_of(line + off[2], len[2], line + off[3], len[3], line + off[4], len[4], line + off[5], len[5],
                      want_label ? out->label : scratch))
            return;
    }
    out->status = ROW;
    out->ctg_off = off[0]; out->ctg_len = len[0]; out->pos = a; out->end = b;
}

// Host form of the line pass of cv_truth_dev.hip over text[0, len): the same outputs in the same layout (see
// cv_truth_lines_dev in include/clairvoyante_amd.h).  Returns nothing; the caller has checked the arguments.
inline void host_form(const uint8_t *text, int64_t len, int format, const Filter *filter, int64_t max_lines, int64_t *pos, int64_t *end,
                      float *label, int32_t *run, int64_t *tok, int64_t *info)
{
    int64_t lines = 0, rows = 0, skipped = 0, host = 0, runs = 0, start = 0;
    int64_t prev_off = 0, prev_len = -1;                         // the contig token of the line before, when that was a ROW
    for (int64_t i = 0; i < len && lines < max_lines; ++i) {
        if (text[i] != '\n') continue;
        Line L;
        verdict(text + start, i - start, format, filter, true, &L);
        if (L.status == ROW) {
            bool differs = prev_len != L.ctg_len;
            for (int k = 0; !differs && k < L.ctg_len; ++k) differs = text[prev_off + k] != text[start + L.ctg_off + k];
            if (differs) { tok[2 * runs] = start + L.ctg_off; tok[2 * runs + 1] = L.ctg_len; ++runs; }
            pos[rows] = L.pos;
            if (format == FMT_BED) end[rows] = L.end;
            else for (int k = 0; k < 16; ++k) label[rows * 16 + k] = L.label[k];
            run[rows] = (int32_t)(runs - 1);
            ++rows;
            prev_off = start + L.ctg_off; prev_len = L.ctg_len;
        } else {
            prev_len = -1;
            if (L.status == SKIP) ++skipped;
            else ++host;
        }
        ++lines;
        start = i + 1;
    }
    info[0] = start; info[1] = lines; info[2] = rows; info[3] = skipped; info[4] = host; info[5] = runs; info[6] = 0; info[7] = 0;
}

}  // namespace cvt
