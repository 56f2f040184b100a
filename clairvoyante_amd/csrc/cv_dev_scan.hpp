// cv_dev_scan.hpp -- the temporary-storage size queries of the hipcub scans and sorts the device entry points run
// between their kernels.  Each makes the call with null pointers, as hipcub defines the query; hipcub counts items in an
// int, so each refuses a count past INT_MAX itself: the entry points' own range checks fire first, this is the backstop
// that keeps the narrowing cast in one place.
#pragma once
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include "cv_dev_common.hpp"

inline bool cv_cub_count_ok(const char *what, int64_t n)
{
    if (n < 0 || n > INT_MAX) {
        cv_set_error("%s: %lld items are more than hipcub counts (0 .. %d)", what, (long long)n, INT_MAX);
        return false;
    }
    return true;
}

// DeviceScan::ExclusiveSum over n values of T
template <class T> int cv_scan_temp_bytes(int64_t n, size_t *bytes)
{
    if (!cv_cub_count_ok("cv_scan_temp_bytes", n)) return 1;
    CV_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const T *)nullptr, (T *)nullptr, (int)n, (hipStream_t)0));
    return 0;
}

// DeviceScan::InclusiveSum over n values of T
template <class T> int cv_inclusive_sum_temp_bytes(int64_t n, size_t *bytes)
{
    if (!cv_cub_count_ok("cv_inclusive_sum_temp_bytes", n)) return 1;
    CV_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, *bytes, (const T *)nullptr, (T *)nullptr, (int)n, (hipStream_t)0));
    return 0;
}

// DeviceScan::InclusiveScan with hipcub::Max over n values of T
template <class T> int cv_max_scan_temp_bytes(int64_t n, size_t *bytes)
{
    if (!cv_cub_count_ok("cv_max_scan_temp_bytes", n)) return 1;
    CV_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, *bytes, (const T *)nullptr, (T *)nullptr, hipcub::Max(), (int)n, (hipStream_t)0));
    return 0;
}

// DeviceScan::ExclusiveScan with the caller's operator and initial value over n values of T
template <class T, class Op> int cv_exclusive_scan_temp_bytes(int64_t n, Op op, T init, size_t *bytes)
{
    if (!cv_cub_count_ok("cv_exclusive_scan_temp_bytes", n)) return 1;
    CV_HIP(hipcub::DeviceScan::ExclusiveScan(nullptr, *bytes, (const T *)nullptr, (T *)nullptr, op, init, (int)n, (hipStream_t)0));
    return 0;
}

// DeviceRadixSort::SortPairs over n (key K, value V) pairs, all key bits
template <class K, class V> int cv_sort_pairs_temp_bytes(int64_t n, size_t *bytes)
{
    if (!cv_cub_count_ok("cv_sort_pairs_temp_bytes", n)) return 1;
    CV_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const K *)nullptr, (K *)nullptr, (const V *)nullptr, (V *)nullptr, (int)n, 0,
                                              (int)sizeof(K) * 8, (hipStream_t)0));
    return 0;
}
