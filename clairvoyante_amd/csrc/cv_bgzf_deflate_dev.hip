// cv_bgzf_deflate_dev.hip -- BGZF members compressed in HBM (utils_v2.BgzfWriter, deflate="device"): the text of a slab
// never crosses to the host, the file's bytes cross once.  cv_bgzf_deflate_core.hpp holds the encoder -- one workgroup per
// member, position-parallel -- once for these kernels and for cv_bgzf_deflate_host_form.
//
//   bd_compress   one workgroup of 256 per member, looping over the members (the grid is capped): cvd::member.  The state
//                 is the CU's LDS (the text and the hash table, later the parse's steps, later the block's image), the
//                 verdict per position (256 KiB per workgroup) lies in the workspace.  The member goes to its own 64 KiB
//                 slot, its size to sizes[k], its block type is counted.
//   bd_offsets    one workgroup: the running sum of the sizes -> where each member lies in the file; the total.
//   bd_assemble   one workgroup per member, looping: the slot's bytes to their place, 16 bytes per lane where source and
//                 destination share their phase, bytes at the ends and otherwise.  A member that does not fit below
//                 out_cap is not written (info[0] still says what was needed).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/clairvoyante_amd.h"
#include "cv_dev_common.hpp"
#include "cv_bgzf_deflate_core.hpp"

namespace {

constexpr int MAX_GRID = 512;                 // workgroups of bd_compress: two rounds of the 256 CUs, 128 MiB of verdicts
constexpr int64_t MAX_MEMBERS = (int64_t)1 << 24;
typedef unsigned long long u64;

__global__ __launch_bounds__(cvd::THREADS) void bd_compress(const uint8_t *__restrict__ text, int64_t len, int64_t block, int64_t members,
                                                             uint32_t *__restrict__ verdicts, int64_t per_group, uint8_t *__restrict__ slots,
                                                             int32_t *__restrict__ sizes, int64_t *__restrict__ info,
                                                             const cvi::crc_consts C)
{
    __shared__ cvd::state S;
    uint32_t *ent = verdicts + (int64_t)blockIdx.x * per_group;
    for (int64_t m = blockIdx.x; m < members; m += gridDim.x) {
        const int64_t lo = m * block;
        int64_t n = len - lo < block ? len - lo : block;
        if (n < 0) n = 0;
        cvd::member(S, text + lo, (uint32_t)n, ent, slots + m * (int64_t)cvd::SLOT, C);
        if (threadIdx.x == 0) {
            sizes[m] = (int32_t)S.size;
            atomicAdd((u64 *)&info[2 + S.kind], (u64)1);
        }
        __syncthreads();                        // the next member clears the state
    }
}

__global__ __launch_bounds__(256) void bd_offsets(const int32_t *__restrict__ sizes, int64_t members, int64_t *__restrict__ off,
                                                   int64_t *__restrict__ info)
{
    __shared__ int64_t s[256];
    const int t = threadIdx.x;
    int64_t running = 0;
    for (int64_t lo = 0; lo < members; lo += 256) {     // (wave-uniform: every thread takes every barrier)
        const int64_t k = lo + t;
        const int64_t v = k < members ? sizes[k] : 0;
        s[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t x = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += x;
            __syncthreads();
        }
        if (k < members) off[k] = running + s[t] - v;
        running += s[255];
        __syncthreads();
    }
    if (t == 0) { off[members] = running; info[0] = running; info[1] = members; }
}

__global__ __launch_bounds__(256) void bd_assemble(const uint8_t *__restrict__ slots, const int32_t *__restrict__ sizes,
                                                    const int64_t *__restrict__ off, int64_t members, uint8_t *__restrict__ out,
                                                    int64_t out_cap)
{
    const int t = threadIdx.x;
    for (int64_t m = blockIdx.x; m < members; m += gridDim.x) {
        const int64_t size = sizes[m], at = off[m];
        if (size < 0 || size > (int64_t)cvd::SLOT - cvd::MEMBER_AT || at < 0 || at > out_cap - size) continue;
        const uint8_t *src = slots + m * (int64_t)cvd::SLOT + cvd::MEMBER_AT;
        uint8_t *dst = out + at;
        if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0) {
            int64_t head = (16 - (int64_t)((uintptr_t)dst & 15)) & 15;
            if (head > size) head = size;
            const int64_t granules = (size - head) >> 4, done = head + 16 * granules;
            for (int64_t g = t; g < granules; g += 256)
                *reinterpret_cast<uint4 *>(dst + head + 16 * g) = *reinterpret_cast<const uint4 *>(src + head + 16 * g);
            if (t < head) dst[t] = src[t];
            if (t < size - done) dst[done + t] = src[done + t];
        } else {
            for (int64_t i = t; i < size; i += 256) dst[i] = src[i];
        }
    }
}

// the workspace of cv_bgzf_deflate_dev
struct deflate_ws {
    uint8_t *slots;
    uint32_t *verdicts;
    int64_t *off;                    // members + 1
    int64_t per_group;
    int groups;
};

void plan(cv_carver &c, int64_t members, int64_t block, deflate_ws *W)
{
    W->groups = cv_grid_for(members, 1, MAX_GRID);
    W->per_group = (int64_t)(cv_up256((size_t)block * sizeof(uint32_t)) / sizeof(uint32_t));
    W->slots = c.take<uint8_t>((size_t)members * cvd::SLOT);
    W->verdicts = c.take<uint32_t>((size_t)W->groups * (size_t)W->per_group);
    W->off = c.take<int64_t>((size_t)members + 1);
}

bool shape_ok(const char *who, int64_t members, int64_t block)
{
    if (block < 1 || block > (int64_t)cvd::BLOCK_MAX || members < 1 || members > MAX_MEMBERS) {
        cv_set_error("%s: block %lld (1 .. %u) or %lld members (1 .. %lld) out of range", who, (long long)block, cvd::BLOCK_MAX,
                     (long long)members, (long long)MAX_MEMBERS);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int cv_bgzf_deflate_workspace(int64_t members, int64_t block, int64_t *bytes)
{
    const char *who = "cv_bgzf_deflate_workspace";
    if (!bytes) { cv_set_error("%s: null argument", who); return 1; }
    if (!shape_ok(who, members, block)) return 1;
    cv_carver c;
    deflate_ws W;
    plan(c, members, block, &W);
    *bytes = (int64_t)c.total();
    return 0;
}

// phases: bit 0 bd_compress, bit 1 bd_offsets, bit 2 bd_assemble
static int deflate_launch(const char *who, int phases, const uint8_t *text_dev, int64_t len, int64_t block, uint8_t *out_dev, int64_t out_cap,
                          int32_t *sizes_dev, int64_t *info_dev, void *workspace, int64_t workspace_bytes, void *stream)
{
    static const cvi::crc_consts C = [] { cvi::crc_consts c; cvi::make_crc_consts(&c); return c; }();
    if (len < 0 || out_cap < 0 || !out_dev || !sizes_dev || !info_dev || (len > 0 && !text_dev)) {
        cv_set_error("%s: null argument, or a negative length", who);
        return 1;
    }
    const int64_t members = block > 0 ? cvd::members_of(len, block) : 0;
    if (!shape_ok(who, members, block)) return 1;
    if (((uintptr_t)sizes_dev & 3) || ((uintptr_t)info_dev & 7)) {
        cv_set_error("%s: the sizes must be 4-byte, info 8-byte aligned", who);
        return 1;
    }
    cv_carver c(workspace);
    deflate_ws W;
    plan(c, members, block, &W);
    if (!cv_workspace_ok(who, workspace, workspace_bytes, c.total())) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (phases & 1) {
        CV_HIP(hipMemsetAsync(info_dev, 0, 8 * sizeof(int64_t), st));
        hipLaunchKernelGGL(bd_compress, dim3(W.groups), dim3(cvd::THREADS), 0, st, text_dev, len, block, members, W.verdicts, W.per_group,
                           W.slots, sizes_dev, info_dev, C);
        CV_HIP(hipGetLastError());
    }
    if (phases & 2) {
        hipLaunchKernelGGL(bd_offsets, dim3(1), dim3(256), 0, st, (const int32_t *)sizes_dev, members, W.off, info_dev);
        CV_HIP(hipGetLastError());
    }
    if (phases & 4) {
        hipLaunchKernelGGL(bd_assemble, dim3(cv_grid_for(members, 1, 4096)), dim3(256), 0, st, (const uint8_t *)W.slots,
                           (const int32_t *)sizes_dev, (const int64_t *)W.off, members, out_dev, out_cap);
        CV_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int cv_bgzf_deflate_dev(const uint8_t *text_dev, int64_t len, int64_t block, uint8_t *out_dev, int64_t out_cap,
                                   int32_t *sizes_dev, int64_t *info_dev, void *workspace, int64_t workspace_bytes, void *stream)
{
    return deflate_launch("cv_bgzf_deflate_dev", 7, text_dev, len, block, out_dev, out_cap, sizes_dev, info_dev, workspace, workspace_bytes,
                          stream);
}

// One phase alone, for tools/gpu_bgzf_deflate_probe.py: 0 compress, 1 offsets, 2 assemble -- the same launches as
// cv_bgzf_deflate_dev, which must have run once on these buffers.
extern "C" int cv_bgzf_deflate_phase_dev(int phase, const uint8_t *text_dev, int64_t len, int64_t block, uint8_t *out_dev, int64_t out_cap,
                                         int32_t *sizes_dev, int64_t *info_dev, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *who = "cv_bgzf_deflate_phase_dev";
    if (phase < 0 || phase > 2) { cv_set_error("%s: phase must be 0, 1 or 2", who); return 1; }
    return deflate_launch(who, 1 << phase, text_dev, len, block, out_dev, out_cap, sizes_dev, info_dev, workspace, workspace_bytes, stream);
}

extern "C" int cv_bgzf_deflate_host_form(const uint8_t *text, int64_t len, int64_t block, uint8_t *out, int64_t out_cap, int32_t *sizes,
                                         int64_t *info)
{
    const char *who = "cv_bgzf_deflate_host_form";
    if (len < 0 || out_cap < 0 || !out || !sizes || !info || (len > 0 && !text)) {
        cv_set_error("%s: null argument, or a negative length", who);
        return 1;
    }
    if (!shape_ok(who, block > 0 ? cvd::members_of(len, block) : 0, block)) return 1;
    cvd::deflate_host_form(text, len, block, out, out_cap, sizes, info);
    return 0;
}
