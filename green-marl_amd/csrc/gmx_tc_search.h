// gmx_tc_search.h -- the sorted-list searches the triangle-counting kernels share (gmx_tc.hip, gmx_tcd.hip).
#ifndef GMX_TC_SEARCH_H_
#define GMX_TC_SEARCH_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

// first position in a[lo, hi) (non-decreasing, global memory) whose value is >= x
__device__ __forceinline__ int32_t tc_lower_bound(const int32_t* __restrict__ a, int32_t lo, int32_t hi, int32_t x) {
    while (lo < hi) {
        int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool tc_contains(const int32_t* __restrict__ a, int32_t lo, int32_t hi, int32_t x) {
    int32_t p = tc_lower_bound(a, lo, hi, x);
    return p < hi && a[p] == x;
}

// the same on a list staged in LDS (no __restrict__: the list is written by the lanes that search it)
__device__ __forceinline__ int32_t tco_lds_lower_bound(const int32_t* a, int32_t lo, int32_t hi, int32_t x) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

#endif
