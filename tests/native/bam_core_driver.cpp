// bam_core_driver.cpp -- csrc/cv_bam_core.hpp in its host form, stand-alone, for tests/test_bam_core_host.py (built with
// AddressSanitizer + UBSan).  Every case's inflated BAM bytes, record table, segments and SEQ bytes live in heap blocks of
// exactly their sizes, so a read or write one byte outside them is a report.
//
// in : cases of  int64 hdr[12] = nbytes, first, tid, exclude, beg0, end0, min_mq, evc, evc_min_mq, contig_pass, n_anchors, 0
//                int64 anchors[n_anchors] | bytes[nbytes]
// out: per case  int32 status of the one-walker walk from `first` (cvb::S_*), int64 stop, int32 taken, uint32 offs[taken]
//                int32 refused by the anchored walk (1) or its table equals the one-walker table (0), int32 walkers used
//                and, unless the status is S_BAD / S_MISS, per taken record:
//                int32 what (cvb::C_*); for C_READ: int32 pos, rf, leading, int64 nseg, nseq, cols, seg[nseg], seq[nseq]
//                (what = 3: a C_READ of more than 65536 segments or 1 MiB of SEQ, the counts without the output)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../clairvoyante_amd/csrc/cv_bam_core.hpp"

static bool get(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }
static void put(FILE *f, const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(3); } }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: bam_core_driver CASES RESULTS\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    int64_t hdr[12];
    while (get(in, hdr, sizeof(hdr))) {
        const int64_t nbytes = hdr[0], first = hdr[1], na = hdr[10];
        if (nbytes < 0 || na < 0 || first < 0 || first > nbytes) { fprintf(stderr, "bad case header\n"); return 2; }
        const cvb::view v{(int32_t)hdr[2], (int32_t)hdr[3], hdr[4], hdr[5]};
        const cvb::filters f{(int32_t)hdr[6], (int32_t)hdr[7], (int32_t)hdr[8], (int32_t)hdr[9]};
        std::vector<int64_t> anchors((size_t)na);
        if (na && !get(in, anchors.data(), (size_t)na * 8)) return 2;
        uint8_t *d = (uint8_t *)malloc((size_t)nbytes ? (size_t)nbytes : 1);
        if (nbytes && !get(in, d, (size_t)nbytes)) return 2;
        // ---- one walker
        const int64_t room = (nbytes - first) / cvb::MIN_STRIDE + 1;
        uint32_t *offs = (uint32_t *)malloc((size_t)room * 4);
        cvb::walked w;
        cvb::walk_interval(d, first, nbytes, nbytes, v, offs, room, &w);
        put(out, &w.status, 4); put(out, &w.stop, 8); put(out, &w.taken, 4); put(out, offs, (size_t)w.taken * 4);
        // ---- a walker per anchor interval, combined as the slab loop of cv_bam_dev.hip combines them
        std::vector<int64_t> bounds;
        bounds.push_back(first);
        for (int64_t a : anchors) bounds.push_back(a);
        bounds.push_back(nbytes);
        std::vector<uint32_t> all;
        int32_t refused = 0, used = 0;
        for (size_t k = 0; k + 1 < bounds.size() && !refused; k++) {
            if (bounds[k] < 0 || bounds[k] > bounds[k + 1] || bounds[k + 1] > nbytes) { refused = 1; break; }
            const int64_t rm = (bounds[k + 1] - bounds[k]) / cvb::MIN_STRIDE + 1;
            uint32_t *mine = (uint32_t *)malloc((size_t)rm * 4);
            cvb::walked o;
            cvb::walk_interval(d, bounds[k], bounds[k + 1], nbytes, v, mine, rm, &o);
            all.insert(all.end(), mine, mine + o.taken);
            free(mine);
            ++used;
            if (o.status == cvb::S_LANDED) continue;
            if (o.status == cvb::S_END) break;
            if (o.status == cvb::S_PARTIAL && k + 2 == bounds.size()) break;
            refused = 1;
        }
        if (!refused && (w.status == cvb::S_BAD || w.status == cvb::S_MISS || (int64_t)all.size() != w.taken ||
                         (w.taken && memcmp(all.data(), offs, (size_t)w.taken * 4)))) {
            fprintf(stderr, "the anchored walk accepted a table the one-walker walk does not give\n");
            return 4;
        }
        put(out, &refused, 4); put(out, &used, 4);
        // ---- count and emit
        if (w.status != cvb::S_BAD && w.status != cvb::S_MISS) {
            for (int32_t i = 0; i < w.taken; i++) {
                const uint8_t *rec = d + offs[i];
                cvb::counts c;
                const int32_t what = cvb::count_record(rec, f, &c);
                if (what == cvb::C_READ && (c.nseg > (1 << 16) || c.nseq > (1 << 20))) {      // damage that asks for much: counts only
                    const int32_t big = 3;
                    put(out, &big, 4);
                    put(out, &c.pos, 4); put(out, &c.rf, 4); put(out, &c.leading, 4);
                    put(out, &c.nseg, 8); put(out, &c.nseq, 8); put(out, &c.cols, 8);
                    continue;
                }
                put(out, &what, 4);
                if (what != cvb::C_READ) continue;
                const uint64_t q0 = 1000 + (uint64_t)i;
                cvb::seg *s1 = (cvb::seg *)malloc((size_t)c.nseg * sizeof(cvb::seg) + 1), *s64 = (cvb::seg *)malloc((size_t)c.nseg * sizeof(cvb::seg) + 1);
                uint8_t *q1 = (uint8_t *)malloc((size_t)c.nseq), *q64 = (uint8_t *)malloc((size_t)c.nseq);
                memset(s1, 0xee, (size_t)c.nseg * sizeof(cvb::seg)); memset(s64, 0xdd, (size_t)c.nseg * sizeof(cvb::seg));
                memset(q1, 0xee, (size_t)c.nseq); memset(q64, 0xdd, (size_t)c.nseq);
                cvb::emit_record(rec, c.rf, 0, c.nseq, q0, s1, q1, 0, 1);
                for (int lane = 63; lane >= 0; lane--) cvb::emit_record(rec, c.rf, 0, c.nseq, q0, s64, q64, lane, 64);
                if (memcmp(s1, s64, (size_t)c.nseg * sizeof(cvb::seg)) || memcmp(q1, q64, (size_t)c.nseq)) {
                    fprintf(stderr, "one lane and 64 lanes emit different bytes\n");
                    return 4;
                }
                put(out, &c.pos, 4); put(out, &c.rf, 4); put(out, &c.leading, 4);
                put(out, &c.nseg, 8); put(out, &c.nseq, 8); put(out, &c.cols, 8);
                put(out, s1, (size_t)c.nseg * sizeof(cvb::seg)); put(out, q1, (size_t)c.nseq);
                free(s1); free(s64); free(q1); free(q64);
            }
        }
        free(offs); free(d);
    }
    fclose(in);
    if (fclose(out)) { perror("close"); return 3; }
    return 0;
}
