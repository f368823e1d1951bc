// gmx_rowgroup.h -- the row-group work loop of the degree-oriented neighbour-list kernels: tc_oriented_kernel and
// aa_rows_kernel (gmx_tc.hip), tcd_count_kernel (gmx_tcd.hip) and lcc_count_kernel (gmx_lcc.hip).
//
// A work item is (vertex v, group of 64 slots of v's row); grp_off[0 .. V] is the exclusive scan of the rows' group counts.
// A wave claims CLAIM items at a time from a 64-bit counter (rg_items), stages the row from the group's first slot on in
// its own LDS slice (rg_stage) and takes the group's slots one per lane.  What a kernel does with a slot -- which side it
// walks, alone or as a wave, what it credits and tallies -- is its own and stays in its unit.
//
// Next to the loop, the searches on a sorted list that these kernels, gmx_ktruss.hip, gmx_kclique.hip and the common-neighbour
// kernels share: rg_lower_bound, rg_contains, rg_run.
#ifndef GMX_ROWGROUP_H_
#define GMX_ROWGROUP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

// ---- sorted-list searches.  LDS: the list is staged in LDS by the lanes that search it, so the pointer carries no
// __restrict__; otherwise it is a row in global memory that nobody writes.
template <bool LDS>
using rg_list = std::conditional_t<LDS, const int32_t*, const int32_t* __restrict__>;

// first position in a[lo, hi) (non-decreasing) whose value is >= x
template <bool LDS>
__device__ __forceinline__ int32_t rg_lower_bound(rg_list<LDS> a, int32_t lo, int32_t hi, int32_t x) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool LDS>
__device__ __forceinline__ bool rg_contains(rg_list<LDS> a, int32_t lo, int32_t hi, int32_t x) {
    const int32_t p = rg_lower_bound<LDS>(a, lo, hi, x);
    return p < hi && a[p] == x;
}

// number of entries of a[lo, hi) equal to x
template <bool LDS>
__device__ __forceinline__ int32_t rg_run(rg_list<LDS> a, int32_t lo, int32_t hi, int32_t x) {
    const int32_t f = rg_lower_bound<LDS>(a, lo, hi, x);
    if (f >= hi || a[f] != x) return 0;
    if (f + 1 >= hi || a[f + 1] != x) return 1;
    return rg_lower_bound<LDS>(a, f + 2, hi, x + 1) - f;
}

// ---- the wave and its LDS slice
// lane 0's value, as one the compiler knows to be the same in every lane (scalar registers, scalar branches)
__device__ __forceinline__ unsigned long long rg_first_lane(unsigned long long x) {
    return ((unsigned long long) (unsigned int) __builtin_amdgcn_readfirstlane((int) (x >> 32)) << 32) |
           (unsigned int) __builtin_amdgcn_readfirstlane((int) x);
}

// the wave's own LDS writes and atomics have landed and are visible to all its lanes.  The barriers keep the compiler from
// moving LDS accesses across the wait; 0xc07f is lgkmcnt(0) with the other counters left alone.
__device__ __forceinline__ void rg_lds_landed() {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
}

// row[0, da) into the wave's slice A, readable by every lane on return.  The copy is pinned to two entries per lane and step
// with a one-entry remainder, the form the kernels had when each wrote the loop out: left to itself the compiler interleaves
// it by eight here (then four, then one, each step behind its own test), which most items, short rows, only pay for.
__device__ __forceinline__ void rg_stage(int32_t* A, const int32_t* __restrict__ row, int32_t da, int lane) {
#pragma clang loop vectorize(disable) interleave_count(2) unroll(disable)
    for (int32_t k = lane; k < da; k += 64) A[k] = row[k];
    rg_lds_landed();
}

// all lanes are done with A before it is overwritten
__device__ __forceinline__ void rg_slice_done() { __builtin_amdgcn_wave_barrier(); }

// ---- the item loop: body(v, group) for every item `part`, `part + nparts`, ... that this wave claims (a kernel without
// parts passes 0, 1), the whole wave converged, group = the item's index among v's groups.  Items of one claim are
// consecutive, so the vertex of the last one is tried before grp_off is searched again.
// One flat loop with the claim as a step of it, not a loop over a claim's items inside a loop over claims: what the bodies
// carry from item to item (their tallies) then goes round one loop, and lcc_count_kernel keeps its 8 waves per SIMD (as
// two nested loops the compiler held every tally in two scalar registers: 106 of them, 7 waves).
template <int CLAIM, class Off, class Body>
__device__ __forceinline__ void rg_items(const Off* grp_off, int64_t V, int part, int nparts,
                                         unsigned long long* next_claim, int lane, Body body) {
    const int64_t G = grp_off[V];
    const int64_t Q = G > part ? (G - part + nparts - 1) / nparts : 0;   // this part's items: q -> item q * nparts + part
    int64_t q = 0, qe = 0;   // [q, qe): what is left of the wave's claim
    int32_t v = -1;
    for (;; q++) {
        if (q == qe) {
            unsigned long long b = 0;
            if (lane == 0) b = atomicAdd(next_claim, (unsigned long long) CLAIM);
            b = rg_first_lane(b);
            if ((int64_t) b >= Q) break;
            q = (int64_t) b;
            qe = q + CLAIM < Q ? q + CLAIM : Q;
            v = -1;
        }
        const int64_t item = q * nparts + part;
        if (v < 0 || (int64_t) grp_off[v + 1] <= item) {   // vertex of the item: last v with grp_off[v] <= item
            uint32_t lo = 0, hi = (uint32_t) V;            // (V < 2^31: lo + hi fits)
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((int64_t) grp_off[mid] <= item) lo = mid; else hi = mid;
            }
            v = (int32_t) lo;
        }
        body(v, (int32_t) (item - grp_off[v]));
    }
}

#endif
