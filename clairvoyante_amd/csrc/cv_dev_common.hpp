// cv_dev_common.hpp -- the launch and workspace plumbing every device entry point shares (cv_X_workspace / cv_X_dev):
// the HIP error check, the launch geometry of the grid-stride kernels, the carver that lays arrays out in a caller's
// workspace and the check of that workspace.  Needs no cv_model: files that do not want cv_internal.hpp include this one
// alone.  The hipcub size queries live beside it in cv_dev_scan.hpp, so that only their users compile hipcub.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

void cv_set_error(const char *fmt, ...);

#define CV_HIP(expr)                                                                     \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            cv_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

inline size_t cv_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// blocks of `threads` for n items walked by CV_GRID_STRIDE: at least one, at most max_grid
inline int cv_grid_for(int64_t n, int threads = 256, int max_grid = 4096)
{
    const int64_t b = (n + threads - 1) / threads;
    return (int)(b < 1 ? 1 : b < max_grid ? b : max_grid);
}

#define CV_GRID_STRIDE(i, n) \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// Arrays one behind the other, each at the next multiple of 256 bytes.  A layout is ONE function that takes its arrays
// from a carver: over no base it is the size query (every pointer null, total() the bytes to ask for), over the caller's
// workspace it is the carve -- the two cannot disagree.
struct cv_carver {
    char *base;
    size_t off = 0;
    explicit cv_carver(void *workspace = nullptr) : base((char *)workspace) {}
    void *take_bytes(size_t bytes)
    {
        const size_t at = off;
        off = cv_up256(off + bytes);
        return base ? base + at : nullptr;
    }
    template <class T> T *take(size_t count) { return (T *)take_bytes(count * sizeof(T)); }
    size_t total() const { return off; }
};

// the workspace a caller gave against what the layout needs (the carver's total); false = refused, the error text is set
inline bool cv_workspace_ok(const char *who, const void *workspace, int64_t have, size_t need)
{
    if (!workspace || ((uintptr_t)workspace & 255)) {
        cv_set_error("%s: the workspace must be there and 256-byte aligned", who);
        return false;
    }
    if (have < (int64_t)need) {
        cv_set_error("%s: workspace holds %lld bytes, need %lld", who, (long long)have, (long long)need);
        return false;
    }
    return true;
}
