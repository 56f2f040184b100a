// cv_bam_dev.hip -- the BAM front end on the device: the compressed BGZF members of a view go to HBM, and the segments,
// SEQ bytes and flags the pileup kernels read are made there.  The host route (cv_bam_view_records + cv_pileup_add_bam)
// stays the definition; the per-record text is shared with it through cv_bam_core.hpp.
//
// A view is taken slab by slab (cv_bam_view_plan: whole BGZF members, the anchors of the linear index inside them):
//   inflate   cv_inflate_bgzf_dev, one wave per member, behind the tail carried from the slab before; a member that comes
//             back CV_BGZF_HOST is inflated by the host and copied into place.
//   walk      the record chain is sequential (block_size gives the next start), but every linear-index entry is a true
//             record start: one lane per anchor interval walks from its anchor and must land EXACTLY on the next.  It
//             checks every record as cv_bam_view_records does, writes the starts of the records to take, and stops at
//             the end of the view, at a record it cannot vouch for, or where the slab's bytes end.
//   gather    the walkers' parts -> one ordered record table.
//   count     a lane per record: filters and the number of segments / SEQ bytes / columns (count_record).
//   scan      hipCUB exclusive scan over those counts: every record's place; and the two pieces of running state of
//             absorb_parts (cv_pileup.hip) as "index within a run of equal POS" -- the depth cap over the tensor-pass
//             reads (a max-scan over run heads), the late mark over the candidate-pass reads (the read before).
//   emit      a wave per record: SEQ unpacked 64 bases a step, the segments of a run spread over the lanes.
//   hand-over cv_pileup_add_bam_dev: the batch goes where cv_pileup_flush puts an upload.
// What the device does not vouch for -- a walker that misses its anchor, a placeholder CIGAR, a record that fails the
// layout checks, POS or CIGAR demands out of range -- makes it refuse the slab BEFORE anything of the handle changes:
// the inflated bytes go back to the host, which walks them as cv_bam_view_records would and calls cv_pileup_add_bam.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/clairvoyante_amd.h"
#include "cv_bam_core.hpp"
#include "cv_dev_scan.hpp"


namespace {

using cvb::S_LANDED; using cvb::S_END; using cvb::S_PARTIAL;
typedef cvb::walked walk_out;

struct sum5 {
    int64_t nseg, nseq, cols, ct, evc;
};
struct add5 {
    __host__ __device__ sum5 operator()(const sum5 &a, const sum5 &b) const
    {
        return sum5{a.nseg + b.nseg, a.nseq + b.nseq, a.cols + b.cols, a.ct + b.ct, a.evc + b.evc};
    }
};

struct rinfo {                    // per taken record
    int32_t pos, rf, leading, clear;
};

struct slab_out {                 // what comes back to the host after the scans
    int64_t nseg, nseq, cols, kept;
    int64_t state[4];
    int32_t refuse, pad;
};

// bounds[i], bounds[i + 1]: the interval of walker i; part[i]: its place in the sparse table (room for every record
// that can start inside the interval)
__global__ void bam_walk(const uint8_t *__restrict__ d, int64_t lim, const int64_t *__restrict__ bounds, const int64_t *__restrict__ part,
                         int nwalk, cvb::view v, uint32_t *__restrict__ table, walk_out *__restrict__ out)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwalk) return;
    cvb::walk_interval(d, bounds[w], bounds[w + 1], lim, v, table + part[w], part[w + 1] - part[w], out + w);
}

__global__ void bam_gather(const uint32_t *__restrict__ table, const int64_t *__restrict__ part, const int64_t *__restrict__ place,
                           int nwalk, uint32_t *__restrict__ recs)
{
    for (int w = blockIdx.x; w < nwalk; w += gridDim.x) {
        const int64_t n = place[w + 1] - place[w];
        for (int64_t k = threadIdx.x; k < n; k += blockDim.x) recs[place[w] + k] = table[part[w] + k];
    }
}

__global__ void bam_count(const uint8_t *__restrict__ d, const uint32_t *__restrict__ recs, int64_t n, cvb::filters f,
                          sum5 *__restrict__ in, rinfo *__restrict__ ri, int32_t *__restrict__ refuse)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cvb::counts c;
    const int what = cvb::count_record(d + recs[i], f, &c);
    if (what == cvb::C_RANGE) atomicOr(refuse, 1);
    const bool read = what == cvb::C_READ;
    in[i] = sum5{c.nseg, c.nseq, c.cols, (read && (c.rf & cvb::F_CT)) ? 1 : 0, (read && (c.rf & cvb::F_EVC)) ? 1 : 0};
    ri[i] = rinfo{c.pos, read ? c.rf : 0, c.leading, 0};
}

// the POS of the tensor-pass reads and of the candidate-pass reads, each in read order
__global__ void bam_split(const sum5 *__restrict__ in, const sum5 *__restrict__ ex, const rinfo *__restrict__ ri, int64_t n,
                          int32_t *__restrict__ ctpos, int32_t *__restrict__ evcpos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (in[i].ct) ctpos[ex[i].ct] = ri[i].pos;
    if (in[i].evc) evcpos[ex[i].evc] = ri[i].pos;
}

// head[k] = k where tensor-pass read k opens a run of equal POS, else -1 (read 0 continues the handle's run when its
// POS is prev_pos: CreateTensor.py:165-172 as absorb_parts restates it)
__global__ void bam_heads(const sum5 *__restrict__ in, const sum5 *__restrict__ ex, int64_t n, const int32_t *__restrict__ ctpos,
                          int64_t prev_pos, int32_t *__restrict__ head)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nct = ex[n - 1].ct + in[n - 1].ct;
    if (k >= nct) return;
    const bool opens = k == 0 ? (int64_t)ctpos[0] != prev_pos : ctpos[k] != ctpos[k - 1];
    head[k] = opens ? (int32_t)k : -1;
}

__device__ __forceinline__ int64_t run_index(const int32_t *runstart, int64_t k, int64_t depth_cap)
{
    const int32_t rs = runstart[k];
    return rs >= 0 ? k - rs : depth_cap + 1 + k;
}

__global__ void bam_resolve(const sum5 *__restrict__ in, const sum5 *__restrict__ ex, rinfo *__restrict__ ri, int64_t n,
                            const int32_t *__restrict__ evcpos, const int32_t *__restrict__ runstart, int64_t dcov, int64_t depth_cap,
                            int64_t evc_prev_pos, unsigned long long *__restrict__ kept)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool alive = false;
    if (i < n && ri[i].rf) {
        int clear = 0;
        if (in[i].ct) {
            const int64_t idx = run_index(runstart, ex[i].ct, depth_cap);
            if (idx > 0 && idx >= dcov) clear |= cvb::F_CT;
        }
        bool late = false;
        if (in[i].evc) {
            const int64_t k = ex[i].evc;
            late = (k == 0 ? evc_prev_pos : (int64_t)evcpos[k - 1]) == (int64_t)ri[i].pos;
        }
        if (ri[i].leading && !late) clear |= cvb::F_LATE;
        ri[i].clear = clear;
        alive = clear == 0 || (in[i].nseg > 0 && ((ri[i].rf & ~clear) & (cvb::F_CT | cvb::F_EVC)));
    }
    const unsigned long long m = __ballot(alive);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(kept, (unsigned long long)__popcll(m));
}

__global__ void bam_totals(const sum5 *__restrict__ in, const sum5 *__restrict__ ex, int64_t n, const int32_t *__restrict__ ctpos,
                           const int32_t *__restrict__ evcpos, const int32_t *__restrict__ runstart, int64_t prev_pos,
                           int64_t depth_cap, int64_t evc_prev_pos, int64_t evc_reads, const unsigned long long *__restrict__ kept,
                           const int32_t *__restrict__ refuse, slab_out *__restrict__ out)
{
    if (blockIdx.x || threadIdx.x) return;
    const sum5 t = add5()(ex[n - 1], in[n - 1]);
    out->nseg = t.nseg; out->nseq = t.nseq; out->cols = t.cols; out->kept = (int64_t)*kept;
    out->state[0] = t.ct ? (int64_t)ctpos[t.ct - 1] : prev_pos;
    out->state[1] = t.ct ? run_index(runstart, t.ct - 1, depth_cap) : depth_cap;
    out->state[2] = t.evc ? (int64_t)evcpos[t.evc - 1] : evc_prev_pos;
    out->state[3] = evc_reads + t.evc;
    out->refuse = *refuse; out->pad = 0;
}

constexpr int EMIT_WAVES = 4;
constexpr int64_t HOST_FLUSH_COLUMNS = (int64_t)1 << 26;      // FLUSH_COLUMNS of pileup.py

__global__ void __launch_bounds__(EMIT_WAVES * 64)
bam_emit(const uint8_t *__restrict__ d, const uint32_t *__restrict__ recs, int64_t n, const sum5 *__restrict__ in,
         const sum5 *__restrict__ ex, const rinfo *__restrict__ ri, cvb::seg *__restrict__ segs, uint8_t *__restrict__ seq)
{
    const int64_t i = (int64_t)blockIdx.x * EMIT_WAVES + (threadIdx.x >> 6);
    if (i >= n || !ri[i].rf) return;
    cvb::emit_record(d + recs[i], ri[i].rf, ri[i].clear, in[i].nseq, (uint64_t)ex[i].nseq, segs + ex[i].nseg, seq + ex[i].nseq,
                     (int)(threadIdx.x & 63), 64);
}

struct devbuf {
    void *p = nullptr;
    size_t cap = 0;
};

int ensure(devbuf &b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    if (b.p) { hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 4 + 256;
    CV_HIP(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

}  // namespace

struct cv_bam_dev {
    int device = 0;
    devbuf comp, table, status, stream[2], bounds, part, place, sparse, wout, recs, in, ex, ri, ctpos, evcpos, head, runstart, tmp,
        small, segs, seq;
    int cur = 0;
    double ms[7] = {0, 0, 0, 0, 0, 0, 0};   // wall time between the synchronisations: inflate, walk, count + scans, emit + hand-over,
                                            // host slabs; HIP-event time of the inflate kernel and of the walk kernel
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<int64_t> place_host;
    int64_t tail = 0, from = 0;   // bytes carried in front of the next slab: stream[cur][from, from + tail)
};

extern "C" int cv_bam_dev_create(int device, cv_bam_dev **out)
{
    if (!out) { cv_set_error("cv_bam_dev_create: null argument"); return 1; }
    int ndev = 0;
    CV_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) { cv_set_error("cv_bam_dev_create: device %d not present (%d visible)", device, ndev); return 1; }
    cv_bam_dev *d = new (std::nothrow) cv_bam_dev();
    if (!d) { cv_set_error("cv_bam_dev_create: out of host memory"); return 1; }
    d->device = device;
    *out = d;
    return 0;
}

extern "C" void cv_bam_dev_destroy(cv_bam_dev *d)
{
    if (!d) return;
    hipSetDevice(d->device);
    devbuf *all[] = {&d->comp, &d->table, &d->status, &d->stream[0], &d->stream[1], &d->bounds, &d->part, &d->place, &d->sparse,
                     &d->wout, &d->recs, &d->in, &d->ex, &d->ri, &d->ctpos, &d->evcpos, &d->head, &d->runstart, &d->tmp, &d->small,
                     &d->segs, &d->seq};
    for (devbuf *b : all) hipFree(b->p);
    for (hipEvent_t e : d->ev) if (e) hipEventDestroy(e);
    delete d;
}

static double lap(std::chrono::steady_clock::time_point &t0)
{
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
}

extern "C" int cv_bam_dev_times(const cv_bam_dev *d, double ms[7])
{
    if (!d || !ms) { cv_set_error("cv_bam_dev_times: null argument"); return 1; }
    for (int k = 0; k < 7; k++) ms[k] = d->ms[k];
    return 0;
}

// a pageable source of an asynchronous copy must outlive the copy on every return, the error returns too
struct sync_on_exit {
    hipStream_t st;
    ~sync_on_exit() { hipStreamSynchronize(st); }
};

struct slab {                     // one slab on its way through the stages
    const uint8_t *comp;
    const int64_t *table, *anchors;
    int64_t members, comp_bytes, inflated, nanch;
    int64_t tail, first, lim;     // the stream is [tail | inflated]; the first record to look at; its end
    uint8_t *sb;                  // the stream in HBM
    // ---- results
    int64_t consumed, records, kept;
    int done;
};

// stage 1: the members behind the carried tail, inflated in HBM (a member the device gives back: by the host)
static int inflate_slab(cv_bam_dev *d, cv_bam *b, slab &s, hipStream_t st, int64_t counts[8])
{
    const int nxt = d->cur ^ 1;
    if (ensure(d->stream[nxt], (size_t)s.lim + 64) || ensure(d->comp, (size_t)s.comp_bytes + 64) ||
        ensure(d->table, (size_t)s.members * 32) || ensure(d->status, (size_t)s.members)) return 1;
    s.sb = (uint8_t *)d->stream[nxt].p;
    std::vector<uint8_t> status((size_t)s.members);
    {
        sync_on_exit wait{st};
        if (s.tail) CV_HIP(hipMemcpyAsync(s.sb, (const uint8_t *)d->stream[d->cur].p + d->from, (size_t)s.tail, hipMemcpyDeviceToDevice, st));
        d->cur = nxt;
        CV_HIP(hipMemcpyAsync(d->comp.p, s.comp, (size_t)s.comp_bytes, hipMemcpyHostToDevice, st));
        CV_HIP(hipMemcpyAsync(d->table.p, s.table, (size_t)s.members * 32, hipMemcpyHostToDevice, st));
        CV_HIP(hipMemsetAsync(d->status.p, 0, (size_t)s.members, st));
        CV_HIP(hipEventRecord(d->ev[0], st));
        if (cv_inflate_bgzf_dev((const uint8_t *)d->comp.p, (const int64_t *)d->table.p, s.members, s.sb + s.tail, s.inflated,
                                (uint8_t *)d->status.p, st)) return 1;
        CV_HIP(hipEventRecord(d->ev[1], st));
        CV_HIP(hipMemcpyAsync(status.data(), d->status.p, (size_t)s.members, hipMemcpyDeviceToHost, st));
    }
    float ms = 0.f;
    CV_HIP(hipEventElapsedTime(&ms, d->ev[0], d->ev[1]));
    d->ms[5] += ms;
    for (int64_t m = 0; m < s.members; m++) {
        if (status[(size_t)m] == CV_BGZF_OK) { counts[2] += 1; continue; }
        uint8_t tmp[65536];
        if (cv_bam_plan_inflate_host(b, m, tmp)) return 1;
        const int64_t isize = (int64_t)((uint64_t)s.table[4 * m + 3] >> 32);
        if (isize) CV_HIP(hipMemcpy(s.sb + s.tail + s.table[4 * m + 2], tmp, (size_t)isize, hipMemcpyHostToDevice));
        counts[3] += 1;
    }
    return 0;
}

// stage 2: a walker per anchor interval, their results combined in order, the record table gathered into d->recs.
// *refuse: a walker did not land where it had to.  s.records / s.done / s.consumed set otherwise.
static int walk_slab(cv_bam_dev *d, slab &s, const cvb::view &v, hipStream_t st, bool *refuse, int64_t counts[8])
{
    std::vector<int64_t> bounds, part;
    std::vector<int64_t> &place = d->place_host;          // (outlives its copy: the next synchronisation is a stage later)
    place.clear();
    bounds.push_back(s.first);
    for (int64_t k = 0; k < s.nanch; k++) bounds.push_back(s.tail + s.anchors[k]);
    bounds.push_back(s.lim);
    part.push_back(0);
    for (size_t k = 0; k + 1 < bounds.size(); k++) part.push_back(part.back() + (bounds[k + 1] - bounds[k]) / cvb::MIN_STRIDE + 1);
    const int nwalk = (int)bounds.size() - 1;
    std::vector<walk_out> wout((size_t)nwalk);
    if (ensure(d->bounds, bounds.size() * 8) || ensure(d->part, part.size() * 8) || ensure(d->place, part.size() * 8) ||
        ensure(d->sparse, (size_t)part.back() * 4) || ensure(d->wout, (size_t)nwalk * sizeof(walk_out))) return 1;
    {
        sync_on_exit wait{st};
        CV_HIP(hipMemcpyAsync(d->bounds.p, bounds.data(), bounds.size() * 8, hipMemcpyHostToDevice, st));
        CV_HIP(hipMemcpyAsync(d->part.p, part.data(), part.size() * 8, hipMemcpyHostToDevice, st));
        CV_HIP(hipEventRecord(d->ev[2], st));
        bam_walk<<<(unsigned)((nwalk + 63) / 64), 64, 0, st>>>(s.sb, s.lim, (const int64_t *)d->bounds.p, (const int64_t *)d->part.p, nwalk, v,
                                                              (uint32_t *)d->sparse.p, (walk_out *)d->wout.p);
        CV_HIP(hipGetLastError());
        CV_HIP(hipEventRecord(d->ev[3], st));
        CV_HIP(hipMemcpyAsync(wout.data(), d->wout.p, (size_t)nwalk * sizeof(walk_out), hipMemcpyDeviceToHost, st));
    }
    float ms = 0.f;
    CV_HIP(hipEventElapsedTime(&ms, d->ev[2], d->ev[3]));
    d->ms[6] += ms;
    place.push_back(0);
    int used = 0;
    for (int w = 0; w < nwalk && !*refuse; w++) {
        const walk_out &o = wout[(size_t)w];
        place.push_back(place.back() + o.taken);
        used = w + 1;
        if (o.status == S_LANDED) continue;
        if (o.status == S_END) { s.done = 1; s.consumed = o.stop; break; }
        if (o.status == S_PARTIAL && w == nwalk - 1) { s.consumed = o.stop; break; }
        *refuse = true;
    }
    counts[5] += used;
    if (*refuse) return 0;
    s.records = place.back();
    if (s.records == 0) return 0;
    while ((int)place.size() < nwalk + 1) place.push_back(place.back());     // the walkers behind the end of the view took nothing that counts
    if (ensure(d->recs, (size_t)s.records * 4)) return 1;
    CV_HIP(hipMemcpyAsync(d->place.p, place.data(), place.size() * 8, hipMemcpyHostToDevice, st));
    bam_gather<<<(unsigned)(nwalk < 4096 ? nwalk : 4096), 256, 0, st>>>((const uint32_t *)d->sparse.p, (const int64_t *)d->part.p,
                                                                       (const int64_t *)d->place.p, nwalk, (uint32_t *)d->recs.p);
    CV_HIP(hipGetLastError());
    return 0;
}

// stage 3: count, scans and running state over the record table; *refuse is decided BEFORE anything of the pileup
// handle changes; then the emit into the handle's own batch buffers and the hand-over.
static int emit_slab(cv_bam_dev *d, cv_pileup *p, slab &s, int contig_ok, hipStream_t st, bool *refuse, std::chrono::steady_clock::time_point &clock)
{
    const int64_t n = s.records;
    int64_t pp[9];
    if (cv_pileup_bam_params(p, pp)) return 1;
    const cvb::filters f{(int32_t)pp[0], (int32_t)pp[2], (int32_t)pp[3], (pp[4] == 0 || contig_ok) ? 1 : 0};
    if (ensure(d->in, (size_t)n * sizeof(sum5)) || ensure(d->ex, (size_t)n * sizeof(sum5)) || ensure(d->ri, (size_t)n * sizeof(rinfo)) ||
        ensure(d->ctpos, (size_t)n * 4) || ensure(d->evcpos, (size_t)n * 4) || ensure(d->head, (size_t)n * 4) ||
        ensure(d->runstart, (size_t)n * 4) || ensure(d->small, 256)) return 1;
    const uint32_t *recs = (const uint32_t *)d->recs.p;
    sum5 *in = (sum5 *)d->in.p, *ex = (sum5 *)d->ex.p;
    rinfo *ri = (rinfo *)d->ri.p;
    int32_t *ctpos = (int32_t *)d->ctpos.p, *evcpos = (int32_t *)d->evcpos.p, *head = (int32_t *)d->head.p, *runstart = (int32_t *)d->runstart.p;
    slab_out *so = (slab_out *)d->small.p;
    unsigned long long *keptd = (unsigned long long *)((uint8_t *)d->small.p + 128);
    int32_t *refd = (int32_t *)((uint8_t *)d->small.p + 136);
    size_t t1 = 0, t2 = 0;
    if (cv_exclusive_scan_temp_bytes(n, add5(), sum5{0, 0, 0, 0, 0}, &t1) || cv_max_scan_temp_bytes<int32_t>(n, &t2)) return 1;
    if (ensure(d->tmp, t1 > t2 ? t1 : t2)) return 1;
    const unsigned g = (unsigned)((n + 255) / 256);
    CV_HIP(hipMemsetAsync(d->small.p, 0, 256, st));
    bam_count<<<g, 256, 0, st>>>(s.sb, recs, n, f, in, ri, refd);
    size_t tb = d->tmp.cap;
    CV_HIP(hipcub::DeviceScan::ExclusiveScan(d->tmp.p, tb, in, ex, add5(), sum5{0, 0, 0, 0, 0}, (int)n, st));
    CV_HIP(hipMemsetAsync(head, 0xff, (size_t)n * 4, st));                 // -1: no head (entries behind the last read)
    bam_split<<<g, 256, 0, st>>>(in, ex, ri, n, ctpos, evcpos);
    bam_heads<<<g, 256, 0, st>>>(in, ex, n, ctpos, pp[5], head);
    tb = d->tmp.cap;
    CV_HIP(hipcub::DeviceScan::InclusiveScan(d->tmp.p, tb, head, runstart, hipcub::Max(), (int)n, st));
    bam_resolve<<<g, 256, 0, st>>>(in, ex, ri, n, evcpos, runstart, pp[1], pp[6], pp[7], keptd);
    bam_totals<<<1, 64, 0, st>>>(in, ex, n, ctpos, evcpos, runstart, pp[5], pp[6], pp[7], pp[8], keptd, refd, so);
    CV_HIP(hipGetLastError());
    slab_out res;
    CV_HIP(hipMemcpyAsync(&res, so, sizeof(res), hipMemcpyDeviceToHost, st));
    CV_HIP(hipStreamSynchronize(st));
    d->ms[2] += lap(clock);
    if (res.refuse || (uint64_t)res.nseq >= 0xffffff00ull - 64 || res.nseg >= ((int64_t)1 << 31)) { *refuse = true; return 0; }
    if (res.nseg > 0) {
        void *segs = nullptr;
        uint8_t *seq = nullptr;
        if (cv_pileup_reserve_bam_dev(p, res.nseg, res.nseq, &segs, &seq, st)) return 1;
        bam_emit<<<(unsigned)((n + EMIT_WAVES - 1) / EMIT_WAVES), EMIT_WAVES * 64, 0, st>>>(s.sb, recs, n, in, ex, ri, (cvb::seg *)segs, seq);
        CV_HIP(hipGetLastError());
        if (cv_pileup_add_bam_dev(p, segs, res.nseg, seq, res.nseq, res.cols, res.state, st)) return 1;
    } else if (cv_pileup_add_bam_dev(p, nullptr, 0, nullptr, 0, res.cols, res.state, st)) return 1;
    s.kept = res.kept;
    d->ms[3] += lap(clock);
    return 0;
}

// the refused slab on the host, from the same inflated bytes: the walk of cv_bam_view_records, then cv_pileup_add_bam
// (and the flush the host route's loop does once enough columns are queued)
static int host_slab(cv_bam_dev *d, cv_pileup *p, const cvb::view &v, slab &s, int contig_ok, hipStream_t st)
{
    std::vector<uint8_t> bytes((size_t)s.lim + 8);
    CV_HIP(hipMemcpyAsync(bytes.data(), s.sb, (size_t)s.lim, hipMemcpyDeviceToHost, st));
    CV_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> offs;
    int64_t at = s.first;
    s.done = 0; s.kept = 0;
    for (;;) {
        int64_t bs;
        const int what = cvb::walk_step(bytes.data(), at, s.lim, v, &bs);
        if (what == cvb::W_PARTIAL) break;
        if (what == cvb::W_BAD_SIZE) { cv_set_error("bam: corrupt record (block_size %lld)", (long long)bs); return 1; }
        if (what == cvb::W_BAD_LAYOUT) { cv_set_error("bam: corrupt record layout"); return 1; }
        if (what == cvb::W_END) { s.done = 1; break; }
        if (what == cvb::W_PLACEHOLDER) {
            const uint8_t *ops; int64_t nops;
            if (cv_bam_record_cigar(bytes.data() + at + 4, &ops, &nops)) { cv_set_error("bam: placeholder CIGAR without a CG:B,I tag"); return 1; }
        }
        if (what != cvb::W_SKIP) offs.push_back((uint32_t)(at + 4));
        at += 4 + bs;
    }
    s.consumed = at;
    s.records = (int64_t)offs.size();
    if (offs.empty()) return 0;
    if (cv_pileup_add_bam(p, bytes.data(), offs.data(), (int64_t)offs.size(), contig_ok, &s.kept)) return 1;
    if (cv_pileup_pending(p) >= HOST_FLUSH_COLUMNS && cv_pileup_flush(p, st)) return 1;
    return 0;
}

// counts[8]: slabs, records taken on the device, members inflated on the device, members inflated on the host, slabs
// handed over to the host, walkers, records of the slabs handed over, members read in all
extern "C" int cv_bam_dev_view(cv_bam_dev *d, cv_bam *b, cv_pileup *p, int64_t slab_bytes, int contig_ok, void *stream, int64_t *kept_out,
                               int64_t counts[8])
{
    if (!d || !b || !p || !kept_out || !counts) { cv_set_error("cv_bam_dev_view: null argument"); return 1; }
    CV_HIP(hipSetDevice(d->device));
    hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < 8; k++) counts[k] = 0;
    *kept_out = 0;
    d->tail = 0;
    for (int k = 0; k < 4; k++)
        if (!d->ev[k]) CV_HIP(hipEventCreate(&d->ev[k]));
    int64_t vp[4];
    if (cv_bam_view_params(b, vp)) return 1;
    const cvb::view v{(int32_t)vp[0], (int32_t)vp[1], vp[2], vp[3]};
    for (;;) {
        int64_t info[8];
        slab s = {};
        if (cv_bam_view_plan(b, slab_bytes, info, &s.comp, &s.table, &s.anchors)) return 1;
        s.members = info[0]; s.comp_bytes = info[1]; s.inflated = info[2]; s.nanch = info[4];
        const bool eof = info[5] != 0;
        if (s.members == 0) {
            if (d->tail) { cv_set_error("bam: truncated record"); return 1; }
            return 0;
        }
        auto clock = std::chrono::steady_clock::now();
        s.tail = d->tail; s.lim = s.tail + s.inflated; s.first = s.tail ? 0 : info[3];
        if (s.lim >= ((int64_t)1 << 31) - 65536) { cv_set_error("bam: record larger than 2 GiB"); return 1; }
        if (s.first > s.lim) { cv_set_error("bam: the view starts behind its first block"); return 1; }
        s.consumed = s.lim;
        counts[0] += 1; counts[7] += s.members;
        if (inflate_slab(d, b, s, st, counts)) return 1;
        d->ms[0] += lap(clock);
        bool refuse = false;
        if (walk_slab(d, s, v, st, &refuse, counts)) return 1;
        d->ms[1] += lap(clock);
        if (!refuse && s.records > 0 && emit_slab(d, p, s, contig_ok, st, &refuse, clock)) return 1;
        if (refuse) {                          // nothing of p has changed: the same bytes on the host
            if (host_slab(d, p, v, s, contig_ok, st)) return 1;
            counts[4] += 1; counts[6] += s.records;
            d->ms[4] += lap(clock);
        } else counts[1] += s.records;
        *kept_out += s.kept;
        if (s.done) { d->tail = 0; return 0; }
        d->tail = s.lim - s.consumed;
        d->from = s.consumed;
        if (eof) {
            if (d->tail) { cv_set_error("bam: truncated record"); return 1; }
            return 0;
        }
    }
}
