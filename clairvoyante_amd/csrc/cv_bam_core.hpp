// cv_bam_core.hpp -- the per-record logic of the device BAM reader (cv_bam_dev.hip), compiled for host and device:
// the kernels, the host fallback of a refused slab and the sanitized host driver of tests/native/ run this same text.
//
//   walk_step     one step along the record chain: what cv_bam_view_records (cv_bam.cpp) decides for the record at
//                 `at` -- the block_size and layout checks, the end of the view, the take decision.
//   count_record  parse_bam_record (cv_pileup.hip) without its output: the filters, the number of segments, SEQ bytes
//                 and alignment columns the record produces, whether a leading insertion / deletion opens it.
//   emit_record   the output itself: SEQ bytes and segments, written by `nlanes` cooperating lanes (lane l takes the
//                 bases and segments l, l + nlanes, ...); no lane reads what another wrote.
//
// Nothing here reads outside [d + at, d + lim) resp. the record's own block_size bytes: every length is checked against
// the bytes that are there before it is used (SAM/BAM specification 4.2).
#ifndef CV_BAM_CORE_HPP
#define CV_BAM_CORE_HPP
#include <stdint.h>

#if defined(__HIPCC__)
#define CVB_HD __host__ __device__ inline
#else
#define CVB_HD inline
#endif

namespace cvb {

constexpr int64_t MAX_RECORD = (int64_t)1 << 30;      // kMaxRecord of cv_bam.cpp
constexpr int SEG_MAX = 64;
constexpr int MIN_STRIDE = 36;                         // block_size field + the 32 fixed bytes: no record is shorter
enum { T_MATCH = 0, T_INS = 1, T_DEL = 2 };
enum { F_CT = 1 << 10, F_EVC = 1 << 11, F_LATE = 1 << 12, F_FIRST = 1 << 13 };     // seg_t::info of cv_pileup.hip

struct seg {                 // seg_t of cv_pileup.hip, field for field
    int32_t r0;
    uint32_t q0;
    int32_t info;
    int32_t adv0;
    int32_t pos;
};

struct view {                // the selection of cv_bam_view_begin
    int32_t tid, exclude;
    int64_t beg0, end0;
};

struct filters {             // of the pileup handle
    int32_t min_mq, evc, evc_min_mq, contig_pass;      // contig_pass: no contig set, or the view's contig is the one set
};

CVB_HD uint32_t u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
CVB_HD int32_t i32(const uint8_t *p) { return (int32_t)u32(p); }
CVB_HD int u16(const uint8_t *p) { return (int)p[0] | ((int)p[1] << 8); }

enum { W_TAKE = 0, W_SKIP = 1, W_END = 2, W_PARTIAL = 3, W_BAD_SIZE = 4, W_BAD_LAYOUT = 5, W_PLACEHOLDER = 6 };

// The record whose block_size field is at d[at]; d[at, lim) is what there is.  *bs = its block_size where that was read
// (W_BAD_SIZE: the offending value).  W_PLACEHOLDER: a record to take whose inline CIGAR is <l_seq>S<span>N.
CVB_HD int walk_step(const uint8_t *d, int64_t at, int64_t lim, const view &v, int64_t *bs)
{
    *bs = 0;
    if (lim - at < 4) return W_PARTIAL;
    const int64_t b = i32(d + at);
    *bs = b;
    if (b < 32) return W_BAD_SIZE;
    if (lim - at < 4 + b) return W_PARTIAL;
    const uint8_t *r = d + at + 4;
    const int32_t tid = i32(r), rpos = i32(r + 4);
    const int l_name = r[8];
    const int n_cig = u16(r + 12), flag = u16(r + 14);
    const int64_t l_seq = i32(r + 16);
    if (l_seq < 0 || b > MAX_RECORD || 32 + (int64_t)l_name + 4 * (int64_t)n_cig + (l_seq + 1) / 2 + l_seq > b) return W_BAD_LAYOUT;
    if (tid < 0 || tid > v.tid || (tid == v.tid && (int64_t)rpos >= v.end0)) return W_END;
    if (tid != v.tid || (flag & v.exclude)) return W_SKIP;
    const uint8_t *cig = r + 32 + l_name;
    if ((int64_t)rpos < v.beg0) {                     // starts left of the region: does it reach in?
        int64_t span = 0;
        for (int k = 0; k < n_cig; k++) {
            const uint32_t c = u32(cig + 4 * k);
            const int op = (int)(c & 15);
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += c >> 4;
        }
        if (span < 1) span = 1;
        if ((int64_t)rpos + span <= v.beg0) return W_SKIP;
    }
    if (n_cig == 2 && (u32(cig) & 15) == 4 && (int64_t)(u32(cig) >> 4) == l_seq && (u32(cig + 4) & 15) == 3) return W_PLACEHOLDER;
    return W_TAKE;
}

// One walker: from the record start `at` to `end` (the next anchor, or lim for the last walker), the starts (at refID)
// of the records to take written to mine[0, room).  S_LANDED: it stands exactly on `end`; S_END: the record at `stop` ends
// the view; S_PARTIAL: the record at `stop` runs past lim; S_MISS: it stepped over `end`; S_BAD: the record at `stop` is
// one the device does not vouch for (block_size, layout, a placeholder CIGAR).
enum { S_LANDED = 0, S_END = 1, S_PARTIAL = 2, S_MISS = 3, S_BAD = 4 };

struct walked {
    int32_t taken, records, status, pad;
    int64_t stop;
};

CVB_HD void walk_interval(const uint8_t *d, int64_t at, int64_t end, int64_t lim, const view &v, uint32_t *mine, int64_t room, walked *out)
{
    int32_t taken = 0, records = 0, status = S_LANDED;
    while (at < end) {
        int64_t bs;
        const int what = walk_step(d, at, lim, v, &bs);
        if (what == W_PARTIAL) { status = S_PARTIAL; break; }
        if (what == W_END) { status = S_END; break; }
        if (what != W_TAKE && what != W_SKIP) { status = S_BAD; break; }
        if (what == W_TAKE) {
            if (taken >= room) { status = S_BAD; break; }              // (cannot happen: MIN_STRIDE bytes per record)
            mine[taken++] = (uint32_t)(at + 4);
        }
        ++records;
        at += 4 + bs;
    }
    if (status == S_LANDED && at != end) status = S_MISS;
    out->taken = taken; out->records = records; out->status = status; out->pad = 0;
    out->stop = at;
}

enum { C_NONE = 0, C_READ = 1, C_RANGE = 2 };

struct counts {
    int64_t nseg, nseq, cols;     // segments, SEQ bytes (padding included), alignment columns
    int32_t pos;                  // POS, 0-based (inside int32 once the range check has passed)
    int32_t rf;                   // F_CT | F_EVC: the filters the read passed
    int32_t leading;              // an insertion / deletion run opens the read (provisional F_LATE)
};

// rec at refID (a record that passed walk_step).  C_NONE: passes neither filter, produces nothing.  C_RANGE: POS or the
// CIGAR's demands are outside what parse_bam_record accepts -- it raises, the device refuses.
CVB_HD int count_record(const uint8_t *rec, const filters &f, counts *out)
{
    const int64_t pos = i32(rec + 4);
    const int l_name = rec[8];
    const int64_t mq = rec[9];
    const int n_cig = u16(rec + 12);
    const int64_t l_seq = i32(rec + 16);
    const uint8_t *cg = rec + 32 + l_name;
    const int64_t seqlen = l_seq > 0 ? l_seq : 1;
    int64_t need = 0, total = 0, clipped = 0;
    for (int k = 0; k < n_cig; k++) {
        const uint32_t c = u32(cg + 4 * k);
        const int op = (int)(c & 15);
        const int64_t v = c >> 4;
        if (op > 8) continue;
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) need += v;
        total += v;
        if (op == 4) clipped += v;
    }
    const bool ct_ok = mq >= f.min_mq;
    bool evc_ok = f.evc != 0 && mq >= f.evc_min_mq && f.contig_pass != 0;
    if (evc_ok && 1.0 - (double)clipped / (double)(total + 1) < 0.55) evc_ok = false;
    out->nseg = out->nseq = out->cols = 0;
    out->pos = 0; out->rf = 0; out->leading = 0;
    if (!ct_ok && !evc_ok) return C_NONE;
    if (pos < -((int64_t)1 << 30) || pos > ((int64_t)1 << 31) - (1 << 24)) return C_RANGE;
    if (need > ((int64_t)1 << 31) || total > ((int64_t)1 << 40)) return C_RANGE;
    out->pos = (int32_t)pos;
    out->rf = (ct_ok ? F_CT : 0) | (evc_ok ? F_EVC : 0);
    out->nseq = seqlen + (need > seqlen ? need - seqlen : 0);
    int64_t r = pos;
    for (int k = 0; k < n_cig; k++) {
        const uint32_t c = u32(cg + 4 * k);
        const int op = (int)(c & 15);
        const int64_t v = c >> 4;
        const bool late = evc_ok && r == pos;
        if (op == 0 || op == 7 || op == 8) { out->nseg += (v + SEG_MAX - 1) / SEG_MAX; out->cols += v; r += v; }
        else if (op == 1) { if (late) out->leading = 1; out->nseg += (v + SEG_MAX - 1) / SEG_MAX; out->cols += v; }
        else if (op == 2) { if (late) out->leading = 1; out->nseg += (v + SEG_MAX - 1) / SEG_MAX; out->cols += v; r += v; }
    }
    return C_READ;
}

// The record's SEQ bytes to seq[0, nseq) and its segments to segs[0, nseg), as parse_bam_record + emit() write them and
// absorb_parts leaves them: rf the filters passed, `clear` the flag bits the running state takes away (F_CT, F_LATE),
// q0 the place of seq[0] in the batch's SEQ buffer.
CVB_HD void emit_record(const uint8_t *rec, int32_t rf, int32_t clear, int64_t nseq, uint64_t q0, seg *segs, uint8_t *seq, int lane,
                        int nlanes)
{
    const char NT[] = "=ACMGRSVTWYHKDBN";
    const int64_t pos = i32(rec + 4);
    const int l_name = rec[8];
    const int n_cig = u16(rec + 12);
    const int64_t l_seq = i32(rec + 16);
    const uint8_t *cg = rec + 32 + l_name;
    const uint8_t *sq = cg + 4 * (int64_t)n_cig;
    const int64_t seqlen = l_seq > 0 ? l_seq : 1;
    for (int64_t k = lane; k < l_seq; k += nlanes) seq[k] = (uint8_t)NT[(sq[k >> 1] >> ((~k & 1) << 2)) & 15];
    if (l_seq == 0 && lane == 0) seq[0] = (uint8_t)'*';
    for (int64_t k = seqlen + lane; k < nseq; k += nlanes) seq[k] = (uint8_t)'?';
    const bool evc_ok = (rf & F_EVC) != 0;
    int64_t r = pos, q = 0, at = 0;
    for (int k = 0; k < n_cig; k++) {
        const uint32_t c = u32(cg + 4 * k);
        const int op = (int)(c & 15);
        const int64_t v = c >> 4;
        const int lf = rf | ((evc_ok && r == pos) ? F_LATE : 0);
        int type;
        if (op == 4) { q += v; continue; }
        else if (op == 0 || op == 7 || op == 8) type = T_MATCH;
        else if (op == 1) type = T_INS;
        else if (op == 2) type = T_DEL;
        else continue;                                  // N, H, P and codes above 8 move nothing
        const int flags = (type == T_MATCH ? rf : lf) & ~clear;
        const bool ref_advances = type != T_INS;
        const int64_t ns = (v + SEG_MAX - 1) / SEG_MAX;
        for (int64_t s = lane; s < ns; s += nlanes) {
            const int64_t done = s * SEG_MAX;
            const int64_t len = v - done < SEG_MAX ? v - done : SEG_MAX;
            seg o;
            o.r0 = (int32_t)(ref_advances ? r + done : r);
            o.q0 = (uint32_t)(type == T_DEL ? 0 : q0 + (uint64_t)q + (uint64_t)done);
            o.info = (int32_t)len | (type << 8) | flags | (done == 0 ? F_FIRST : 0);
            o.adv0 = type == T_INS ? (int32_t)done : 0;
            o.pos = (int32_t)pos;
            segs[at + s] = o;
        }
        at += ns;
        if (ref_advances) r += v;
        if (type != T_DEL) q += v;
    }
}

}  // namespace cvb
#endif
