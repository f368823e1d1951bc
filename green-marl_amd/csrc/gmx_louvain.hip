// gmx_louvain.hip -- Louvain modularity communities on gfx950: gmx_louvain (gmx.h has the definition).
//
// Every level is a symmetric CSR with 64-bit weights and a diagonal: key[j] = (row << 32 | column) ascending, w[j], beg[n + 1],
// k[i] = the sum of row i.  Level 0 is the contraction of the doubled slot list under the identity map, so one builder
// (louvain_contract: device sort of the keys, reduce-by-key of the weights, row offsets, k) makes every level.  All decisions
// are taken in integers: a score m2 e[D] - k[i] (tot[D] - [D == c] k[i]) is a signed 128-bit value, the modularity numerator
// Qnum = m2 intra - sum tot^2 likewise.  The partition is therefore a pure function of the schedule in gmx.h.
//
// A half-round is a chain of launches on the default stream, none of which the host waits for:
//   compact   the vertices of this half with a non-empty row -> three lists by row length
//   short     rows below WAVE_MIN (at most 32 entries): 16 lanes per row, two (label, weight) per lane in registers, the
//             weights of equal labels summed by all-pairs comparison over the lane group
//   wave      rows below BLOCK_MIN: a wave per row, open-addressing table (CAS on the key, 64-bit LDS add on the sum) in the
//             wave's LDS slice; every lane scores the table entries it scans (tot[D] is a gather from the snapshot) and the
//             wave reduces (score, label) in a fixed total order: higher score, then smaller label
//   block     the rest: a workgroup per row, the same table in the workgroup's LDS
//   overflow  rows whose table filled are counted again in passes over DISJOINT LABEL CLASSES (fmix32(label) mod 2^k == c,
//             split further while a class still fills), the classes of a row dealt over 32 workgroups; a workgroup keeps its
//             best (score, label) and e[c] across its passes in registers and hands them on as a partial: no row length or
//             label count is refused
//   final     the overflowed rows' decisions: the 32 partials of a row reduced in the same total order
//   commit    comm[i] = D for the pending list (i, old, new), tot[old] -= k[i], tot[new] += k[i] by 64-bit atomics
//   measure   intra by one sweep of the entries, sum tot^2 as 128-bit partials per workgroup (both return at once when the
//             pending list is empty)
//   judge     one wave adds the partials, lane 0 decides: Qnum strictly greater -> keep, else the roll-back flag
//   undo      returns at once unless the flag is set; else the pending list backwards: comm and tot as before
// comm and tot are only read between compact and commit.  The host reads one record per round (pinned memory).
#include "gmx_internal.h"

#include <rocprim/rocprim.hpp>

#define LV_THREADS 256
#define LV_EMPTY (-1)
#define LV_PROBES 64               // linear probes after which a table counts as full
#define LV_WAVE_MIN 33             // defaults of GMX_LOUVAIN_WAVE_MIN, GMX_LOUVAIN_BLOCK_MIN, GMX_LOUVAIN_LDS_SLOTS
#define LV_WAVE_MIN_MAX 33         // a short row lies in the registers of its 16 lanes: at most 32 entries
#define LV_BLOCK_MIN 256
#define LV_LDS_SLOTS 4096
#define LV_LDS_SLOTS_MIN 512
#define LV_LDS_SLOTS_MAX 8192      // 12 bytes per slot: 96 KiB of the 160 KiB of a CU
#define LV_WAVE_SHARE 8            // a wave's table holds LDS_SLOTS / LV_WAVE_SHARE slots
#define LV_SPREAD 32               // workgroups that share the label classes of one overflowed row
#define LV_SPREAD_ROWS 4096        // overflowed rows (by list position) that are shared in that way; the others get a workgroup each
#define LV_PARTS 1024              // workgroups of the measure kernel = 128-bit partial sums the judge adds

typedef __int128 lv_i128;
typedef unsigned __int128 lv_u128;
typedef unsigned long long lv_u64;

enum { K_SHORT, K_WAVE, K_BLOCK, K_OVF, K_PEND, K_NCTR };

struct lv_state {   // one per call, on the device; its pinned mirror is the record the host reads once per round
    lv_u64 q_lo;              // Qnum of the kept state
    long long q_hi;
    long long intra;          // of the kept state
    long long intra_new;      // the measure kernel's sum; zeroed by the judge
    lv_u64 weight_sum;        // the weights pass
    unsigned int bad_weight;
    unsigned int undo_n;      // pending entries the undo kernel takes back (0: the half-round was kept)
    unsigned int kept;        // this round: moves kept
    unsigned int rollbacks;   // this round: half-rounds rolled back
    unsigned int ovf;         // this round: rows that went to the class passes
    int32_t n_next;           // labels of the level in use (louvain_rank_kernel)
};

struct lv_partial {   // what one workgroup found in its share of an overflowed row's label classes
    lv_u64 score_lo;
    long long score_hi;
    long long ec;
    int32_t lab;      // < 0: none
    int32_t pad;
};

struct lv_level {
    const int64_t* beg;    // [n + 1]
    const uint64_t* key;   // [nnz] (row << 32 | column), ascending
    const int64_t* w;      // [nnz]
    const int64_t* k;      // [n]
    int32_t* comm;         // [n]
    int64_t* tot;          // [n]
    int32_t* list[3];      // [n] each: the rows of the running half-round by regime
    int32_t* ovf;          // [n]
    int32_t* pend_v;       // [n]
    int32_t* pend_old;
    int32_t* pend_new;
    unsigned int* ctr;     // [K_NCTR]
    lv_partial* spread;    // [LV_SPREAD_ROWS * LV_SPREAD]
    lv_u64* part;          // [2 * LV_PARTS] lo, hi of every workgroup's sum of tot^2
    lv_state* st;
    int64_t n, nnz;
    int64_t m2;
};

__device__ __forceinline__ uint32_t lv_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ void lv_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ lv_i128 lv_shfl_xor128(lv_i128 x, int o, int width) {
    lv_u64 lo = (lv_u64) (lv_u128) x, hi = (lv_u64) ((lv_u128) x >> 64);
    lo = __shfl_xor(lo, o, width);
    hi = __shfl_xor(hi, o, width);
    return (lv_i128) (((lv_u128) hi << 64) | (lv_u128) lo);
}
// the best candidate so far: lab < 0 = none.  Higher score first, then the SMALLER label: a total order, so a reduction
// gives the same answer in any shape.
struct lv_best {
    lv_i128 score;
    int32_t lab;
};
__device__ __forceinline__ void lv_take(lv_best& b, lv_i128 s, int32_t l) {
    if (l >= 0 && (b.lab < 0 || s > b.score || (s == b.score && l < b.lab))) {
        b.score = s;
        b.lab = l;
    }
}
__device__ __forceinline__ void lv_reduce(lv_best& b, long long& ec, int from, int width) {
    for (int o = from; o; o >>= 1) {
        const lv_i128 s = lv_shfl_xor128(b.score, o, width);
        const int32_t l = __shfl_xor(b.lab, o, width);
        lv_take(b, s, l);
        const long long e = __shfl_xor(ec, o, width);
        ec = e > ec ? e : ec;
    }
}
// score(D) of a vertex of label c and weight ki that has e = e[D]
__device__ __forceinline__ lv_i128 lv_score(const lv_level& L, long long e, int32_t D, int32_t c, long long ki) {
    const long long t = L.tot[D] - (D == c ? ki : 0);
    return (lv_i128) L.m2 * (lv_i128) e - (lv_i128) ki * (lv_i128) t;
}
// wave-converged: vertex v of label c moves to the best candidate unless score(c) is the maximum
__device__ __forceinline__ void lv_decide(const lv_level& L, bool act, int32_t v, int32_t c, long long ki, long long ec, const lv_best& b) {
    const bool move = act && b.lab >= 0 && b.score > lv_score(L, ec, c, c, ki);
    const unsigned long long m = __ballot(move);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_ctzll(m);
    unsigned int at = 0;
    if (lane == leader) at = atomicAdd(&L.ctr[K_PEND], (unsigned int) __builtin_popcountll(m));
    at = __shfl(at, leader, 64);
    if (move) {
        const unsigned int p = at + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        L.pend_v[p] = v;
        L.pend_old[p] = c;
        L.pend_new[p] = b.lab;
    }
}

// ---------------------------------------------------------------- the weights, level 0's pairs
// a weight below 1 sets the flag; the sum of the weights
__global__ void __launch_bounds__(LV_THREADS) louvain_weight_kernel(const int32_t* __restrict__ weight, int64_t E, lv_state* st) {
    lv_u64 s = 0;
    bool bad = false;
    for (int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; j < E; j += (int64_t) gridDim.x * blockDim.x) {
        const int32_t x = weight[j];
        bad |= x < 1;
        s += (lv_u64) (x < 1 ? 0 : x);
    }
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&st->weight_sum, s);
    if (bad) st->bad_weight = 1u;
}
// slot j of row u (found by bisection of begin) with column c and weight x: the entries (u, c, x) and (c, u, x)
__global__ void __launch_bounds__(LV_THREADS) louvain_pairs_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx,
                                                                   const int32_t* __restrict__ weight, const int32_t* __restrict__ order, int64_t V,
                                                                   int64_t E, uint64_t* __restrict__ key, int64_t* __restrict__ val) {
    for (int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; j < E; j += (int64_t) gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = V;   // the last row with begin[row] <= j
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t) begin[mid] <= j) lo = mid;
            else hi = mid;
        }
        const uint64_t u = (uint64_t) lo, c = (uint64_t) (uint32_t) idx[j];
        const int64_t x = weight ? (int64_t) weight[order ? order[j] : j] : 1;
        key[2 * j] = (u << 32) | c;
        key[2 * j + 1] = (c << 32) | u;
        val[2 * j] = x;
        val[2 * j + 1] = x;
    }
}

// ---------------------------------------------------------------- a level's rows
// beg[r] = the first entry whose row is >= r, r = 0 .. n
__global__ void __launch_bounds__(LV_THREADS) louvain_rows_kernel(const uint64_t* __restrict__ key, int64_t nnz, int64_t n, int64_t* __restrict__ beg) {
    for (int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; r <= n; r += (int64_t) gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = nnz;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t) (key[mid] >> 32) < r) lo = mid + 1;
            else hi = mid;
        }
        beg[r] = lo;
    }
}
// k[row] += w over the entries: a thread adds a run of 8 entries and flushes where the row changes (k is zero before)
__global__ void __launch_bounds__(LV_THREADS) louvain_k_kernel(const uint64_t* __restrict__ key, const int64_t* __restrict__ w, int64_t nnz,
                                                               int64_t* __restrict__ k) {
    const int64_t runs = (nnz + 7) >> 3;
    for (int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; t < runs; t += (int64_t) gridDim.x * blockDim.x) {
        const int64_t j0 = t * 8, j1 = j0 + 8 < nnz ? j0 + 8 : nnz;
        int64_t row = (int64_t) (key[j0] >> 32);
        lv_u64 s = 0;
        for (int64_t j = j0; j < j1; j++) {
            const int64_t r = (int64_t) (key[j] >> 32);
            if (r != row) {
                atomicAdd((lv_u64*) &k[row], s);
                row = r;
                s = 0;
            }
            s += (lv_u64) w[j];
        }
        atomicAdd((lv_u64*) &k[row], s);
    }
}
__global__ void __launch_bounds__(LV_THREADS) louvain_init_kernel(lv_level L) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < L.n; i += (int64_t) gridDim.x * blockDim.x) {
        L.comm[i] = (int32_t) i;
        L.tot[i] = L.k[i];
    }
}

// the vertices of this half (half < 0: all) with a non-empty row, by row length; a claim per wave and class
__global__ void __launch_bounds__(LV_THREADS) louvain_compact_kernel(lv_level L, uint32_t salt, int half, int64_t wave_min, int64_t block_min) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t base = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) & ~63ll; base < L.n; base += stride) {
        const int64_t i = base + lane;
        bool sel = i < L.n;
        if (sel && half >= 0) sel = (int) (lv_fmix32((uint32_t) i ^ salt) & 1u) == half;
        int64_t d = 0;
        if (sel) {
            d = L.beg[i + 1] - L.beg[i];
            sel = d > 0;
        }
        const int cls = d >= block_min ? K_BLOCK : (d >= wave_min ? K_WAVE : K_SHORT);
        for (int c = 0; c < 3; c++) {
            const unsigned long long mc = __ballot(sel && cls == c);
            if (!mc) continue;
            unsigned int at = 0;
            if (lane == 0) at = atomicAdd(&L.ctr[c], (unsigned int) __builtin_popcountll(mc));
            at = __shfl(at, 0, 64);
            if (sel && cls == c) L.list[c][at + __builtin_popcountll(mc & ((1ull << lane) - 1ull))] = (int32_t) i;
        }
    }
}

// ---------------------------------------------------------------- short rows: 16 lanes per row, at most 32 entries
__global__ void __launch_bounds__(LV_THREADS) louvain_short_kernel(lv_level L) {
    const int lane = threadIdx.x & 63, sub = lane & 15;
    const int64_t n = L.ctr[K_SHORT];
    const int32_t* __restrict__ list = L.list[K_SHORT];
    const int64_t wave = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t base = wave * 4; base < n; base += nwaves * 4) {   // (wave-uniform: shuffles inside)
        const int64_t i = base + (lane >> 4);
        const bool act = i < n;
        const int32_t v = act ? list[i] : 0;
        const int64_t b = act ? L.beg[v] : 0;
        const int32_t len = act ? (int32_t) (L.beg[v + 1] - b) : 0;
        const int32_t c = act ? L.comm[v] : 0;
        const long long ki = act ? L.k[v] : 0;
        int32_t l0 = -1, l1 = -1;   // the diagonal entry is no neighbour
        long long w0 = 0, w1 = 0;
        if (sub < len) {
            const int32_t u = (int32_t) (uint32_t) L.key[b + sub];
            if (u != v) {
                l0 = L.comm[u];
                w0 = L.w[b + sub];
            }
        }
        if (sub + 16 < len) {
            const int32_t u = (int32_t) (uint32_t) L.key[b + sub + 16];
            if (u != v) {
                l1 = L.comm[u];
                w1 = L.w[b + sub + 16];
            }
        }
        // e[l0], e[l1]: the weights of equal labels among the 32 registers of the lane group
        long long e0 = w0 + (l1 == l0 ? w1 : 0), e1 = w1 + (l0 == l1 ? w0 : 0);
#pragma unroll
        for (int r = 1; r < 16; r++) {
            const int src = (lane & ~15) | ((sub + r) & 15);
            const int32_t o0 = __shfl(l0, src, 64), o1 = __shfl(l1, src, 64);
            const long long x0 = __shfl(w0, src, 64), x1 = __shfl(w1, src, 64);
            e0 += (o0 == l0 ? x0 : 0) + (o1 == l0 ? x1 : 0);
            e1 += (o0 == l1 ? x0 : 0) + (o1 == l1 ? x1 : 0);
        }
        lv_best best{0, -1};
        long long ec = 0;
        if (l0 >= 0) {
            lv_take(best, lv_score(L, e0, l0, c, ki), l0);
            if (l0 == c) ec = e0;
        }
        if (l1 >= 0) {
            lv_take(best, lv_score(L, e1, l1, c, ki), l1);
            if (l1 == c) ec = e1;
        }
        lv_reduce(best, ec, 8, 16);
        lv_decide(L, act && sub == 0, v, c, ki, ec, best);
    }
}

// ---------------------------------------------------------------- table rows: NT = 64 (a wave) or LV_THREADS (the workgroup)
template <int NT>
__device__ __forceinline__ void lv_group_sync() {
    if (NT == 64) lv_wave_sync();
    else __syncthreads();
}
// One pass of NT threads over the entries [b, e) of row v: the labels of class cl (fmix32(label) mod 2^lp == cl) are summed in
// the table keys / sums [cap] (cap a power of two), then every thread scores the table entries it scans into best / ec.
// true: an insert found no slot within LV_PROBES (the same answer in every thread); best / ec are then untouched.
template <int NT>
__device__ bool lv_table_pass(const lv_level& L, int32_t v, int64_t b, int64_t e, int32_t* keys, lv_u64* sums, int32_t cap, int lp, uint32_t cl, int tid,
                              int* s_full, int32_t c, long long ki, lv_best& best, long long& ec) {
    for (int32_t s = tid; s < cap; s += NT) {
        keys[s] = LV_EMPTY;
        sums[s] = 0ull;
    }
    if (tid == 0) *s_full = 0;
    lv_group_sync<NT>();
    const uint32_t mask = (uint32_t) cap - 1u, pmask = lp >= 32 ? 0xFFFFFFFFu : (1u << lp) - 1u;
    const int limit = cap < LV_PROBES ? cap : LV_PROBES;
    volatile int32_t* vkeys = keys;
    volatile int* vfull = s_full;
    constexpr int U = 4;   // entries per thread and step: the gathers of a step are in flight together
    for (int64_t j0 = b; j0 < e; j0 += NT * U) {
        if (__builtin_amdgcn_readfirstlane(*vfull)) break;   // somebody found no slot: the pass is void anyway
        int32_t nb[U], labs[U];
        long long wt[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int64_t j = j0 + (int64_t) u * NT + tid;
            nb[u] = j < e ? (int32_t) (uint32_t) L.key[j] : -1;
            wt[u] = j < e ? L.w[j] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; u++) labs[u] = nb[u] >= 0 && nb[u] != v ? L.comm[nb[u]] : -1;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int32_t lab = labs[u];
            const uint32_t h = lv_fmix32((uint32_t) lab);
            if (lab < 0 || (h & pmask) != cl) continue;
            uint32_t s = (lp >= 32 ? 0u : (h >> lp)) & mask;
            int i = 0;
            for (; i < limit; i++) {
                const int32_t k = vkeys[s];
                if (k == lab) break;
                if (k == LV_EMPTY) {
                    const int32_t old = atomicCAS(&keys[s], LV_EMPTY, lab);
                    if (old == LV_EMPTY || old == lab) break;
                }
                s = (s + 1u) & mask;
            }
            if (i < limit) atomicAdd(&sums[s], (lv_u64) wt[u]);
            else *vfull = 1;
        }
    }
    lv_group_sync<NT>();
    const bool f = *s_full != 0;
    if (!f)
        for (int32_t s = tid; s < cap; s += NT) {
            const int32_t k = keys[s];
            if (k >= 0) {
                const long long ek = (long long) sums[s];
                lv_take(best, lv_score(L, ek, k, c, ki), k);
                if (k == c) ec = ek;
            }
        }
    lv_group_sync<NT>();   // (the next pass clears the table)
    return f;
}
// the part of a table a row of len entries uses: at least four slots per entry (clearing and scanning the rest is wasted)
__device__ __forceinline__ int32_t lv_table_for(int64_t len, int32_t cap) {
    while (cap > 64 && cap / 8 >= len) cap >>= 1;
    return cap;
}
// every thread of the workgroup gets the reduced values
__device__ __forceinline__ void lv_block_reduce(lv_best& best, long long& ec, lv_best* s_best, long long* s_ec) {
    lv_reduce(best, ec, 32, 64);
    if ((threadIdx.x & 63) == 0) {
        s_best[threadIdx.x >> 6] = best;
        s_ec[threadIdx.x >> 6] = ec;
    }
    __syncthreads();
    for (int w = 0; w < LV_THREADS / 64; w++) {
        lv_take(best, s_best[w].score, s_best[w].lab);
        ec = s_ec[w] > ec ? s_ec[w] : ec;
    }
    __syncthreads();
}

// one wave per row; dynamic LDS per wave: sums[cap] (64-bit), keys[cap], the full flag
__global__ void __launch_bounds__(LV_THREADS) louvain_wave_kernel(lv_level L, int32_t cap) {
    extern __shared__ lv_u64 lv_lds[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    lv_u64* mine = lv_lds + (size_t) wid * ((size_t) cap + (size_t) cap / 2 + 2);
    lv_u64* sums = mine;
    int32_t* keys = (int32_t*) (mine + cap);
    int* s_full = (int*) (mine + cap + cap / 2);
    const int64_t n = L.ctr[K_WAVE];
    const int32_t* __restrict__ list = L.list[K_WAVE];
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t i = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
        const int32_t v = list[i];
        const int64_t b = L.beg[v], e = L.beg[v + 1];
        const int32_t c = L.comm[v];
        const long long ki = L.k[v];
        lv_best best{0, -1};
        long long ec = 0;
        const bool full = lv_table_pass<64>(L, v, b, e, keys, sums, lv_table_for(e - b, cap), 0, 0u, lane, s_full, c, ki, best, ec);
        if (full) {
            if (lane == 0) L.ovf[atomicAdd(&L.ctr[K_OVF], 1u)] = v;
            continue;
        }
        lv_reduce(best, ec, 32, 64);
        lv_decide(L, lane == 0, v, c, ki, ec, best);
    }
}

// one workgroup per row; dynamic LDS: sums[cap], keys[cap]
__global__ void __launch_bounds__(LV_THREADS) louvain_block_kernel(lv_level L, int32_t cap) {
    extern __shared__ lv_u64 lv_lds[];
    __shared__ lv_best s_best[LV_THREADS / 64];
    __shared__ long long s_ec[LV_THREADS / 64];
    __shared__ int s_full;
    lv_u64* sums = lv_lds;
    int32_t* keys = (int32_t*) (lv_lds + cap);
    const int64_t n = L.ctr[K_BLOCK];
    const int32_t* __restrict__ list = L.list[K_BLOCK];
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t v = list[i];
        const int64_t b = L.beg[v], e = L.beg[v + 1];
        const int32_t c = L.comm[v];
        const long long ki = L.k[v];
        lv_best best{0, -1};
        long long ec = 0;
        const bool full = lv_table_pass<LV_THREADS>(L, v, b, e, keys, sums, lv_table_for(e - b, cap), 0, 0u, threadIdx.x, &s_full, c, ki, best, ec);
        if (full) {
            if (threadIdx.x == 0) L.ovf[atomicAdd(&L.ctr[K_OVF], 1u)] = v;
            continue;
        }
        lv_block_reduce(best, ec, s_best, s_ec);
        if (threadIdx.x < 64) lv_decide(L, threadIdx.x == 0, v, c, ki, ec, best);
    }
}

// The overflowed rows: the row is summed in 2^lp0 label classes, lp0 from its length (half a table of distinct labels per
// class if every entry differs).  A class that fills all the same is split by the next hash bit until its parts fit (fmix32 is
// a bijection: at 32 bits a class holds one label).  The classes are disjoint, so the best (score, label) over all passes is
// the row's, and e[c] is found in exactly one of them.  The first LV_SPREAD_ROWS rows of the list deal their classes over
// LV_SPREAD workgroups each (class c0 to workgroup c0 mod LV_SPREAD), which leave their best and their e[c] in the row's
// partials for louvain_final_kernel; a score does not fit an atomicMax key, and the order (score, smaller label) is total, so the
// partials reduce to one answer in any order.  Rows further down the list are one workgroup's, all classes.
__global__ void __launch_bounds__(LV_THREADS) louvain_overflow_kernel(lv_level L, int32_t cap) {
    extern __shared__ lv_u64 lv_lds[];
    __shared__ lv_best s_best[LV_THREADS / 64];
    __shared__ long long s_ec[LV_THREADS / 64];
    __shared__ int s_full;
    lv_u64* sums = lv_lds;
    int32_t* keys = (int32_t*) (lv_lds + cap);
    const int64_t n = L.ctr[K_OVF];
    const int64_t ns = n < LV_SPREAD_ROWS ? n : LV_SPREAD_ROWS;
    const int64_t items = ns * LV_SPREAD + (n - ns);
    for (int64_t t = blockIdx.x; t < items; t += gridDim.x) {
        const bool shared = t < ns * LV_SPREAD;
        const int64_t i = shared ? t / LV_SPREAD : ns + (t - ns * LV_SPREAD);
        const uint64_t first = shared ? (uint64_t) (t % LV_SPREAD) : 0ull, step = shared ? LV_SPREAD : 1;
        const int32_t v = L.ovf[i];
        const int64_t b = L.beg[v], e = L.beg[v + 1];
        const int32_t c = L.comm[v];
        const long long ki = L.k[v];
        int lp0 = 0;
        while (lp0 < 31 && ((e - b) >> lp0) > cap / 2) lp0++;
        const uint64_t P0 = 1ull << lp0;
        lv_best best{0, -1};
        long long ec = 0;
        for (uint64_t c0 = first; c0 < P0; c0 += step) {
            for (int lp = lp0; lp <= 32; lp++) {
                lv_best tb{0, -1};
                long long te = 0;
                bool full = false;
                const uint64_t P = 1ull << lp;
                for (uint64_t cl = c0; cl < P && !full; cl += P0)
                    full = lv_table_pass<LV_THREADS>(L, v, b, e, keys, sums, cap, lp, (uint32_t) cl, threadIdx.x, &s_full, c, ki, tb, te);
                if (!full) {
                    lv_take(best, tb.score, tb.lab);
                    ec = te > ec ? te : ec;
                    break;
                }
            }
        }
        lv_block_reduce(best, ec, s_best, s_ec);
        if (shared) {
            if (threadIdx.x == 0) {
                lv_partial p;
                p.score_lo = (lv_u64) (lv_u128) best.score;
                p.score_hi = (long long) (best.score >> 64);
                p.ec = ec;
                p.lab = best.lab;
                p.pad = 0;
                L.spread[t] = p;
            }
        } else if (threadIdx.x < 64) {
            lv_decide(L, threadIdx.x == 0, v, c, ki, ec, best);
        }
    }
}
// the shared overflowed rows' decisions from their LV_SPREAD partials, a lane per row
__global__ void __launch_bounds__(LV_THREADS) louvain_final_kernel(lv_level L) {
    const int64_t n = L.ctr[K_OVF];
    const int64_t ns = n < LV_SPREAD_ROWS ? n : LV_SPREAD_ROWS;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t base = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) & ~63ll; base < ns; base += stride) {   // (wave-uniform)
        const int64_t i = base + (threadIdx.x & 63);
        const bool act = i < ns;
        const int32_t v = act ? L.ovf[i] : 0;
        const int32_t c = act ? L.comm[v] : 0;
        const long long ki = act ? L.k[v] : 0;
        lv_best best{0, -1};
        long long ec = 0;
        if (act)
            for (int s = 0; s < LV_SPREAD; s++) {
                const lv_partial p = L.spread[i * LV_SPREAD + s];
                lv_take(best, (lv_i128) (((lv_u128) (lv_u64) p.score_hi << 64) | (lv_u128) p.score_lo), p.lab);
                ec = p.ec > ec ? p.ec : ec;
            }
        lv_decide(L, act, v, c, ki, ec, best);
    }
}

// ---------------------------------------------------------------- commit, measure, judge, undo
__global__ void __launch_bounds__(LV_THREADS) louvain_commit_kernel(lv_level L) {
    const int64_t n = L.ctr[K_PEND];
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const int32_t v = L.pend_v[i];
        const lv_u64 kv = (lv_u64) L.k[v];
        L.comm[v] = L.pend_new[i];
        atomicAdd((lv_u64*) &L.tot[L.pend_old[i]], 0ull - kv);
        atomicAdd((lv_u64*) &L.tot[L.pend_new[i]], kv);
    }
}
// intra = the weights of the entries whose two ends share a label; part[workgroup] = its share of sum tot^2 (128-bit).
// Without pending moves (and force == 0) the state is the judged one: nothing to do.
__global__ void __launch_bounds__(LV_THREADS) louvain_measure_kernel(lv_level L, int force) {
    __shared__ lv_u64 s_lo[LV_THREADS / 64], s_hi[LV_THREADS / 64];
    __shared__ long long s_in[LV_THREADS / 64];
    if (!force && L.ctr[K_PEND] == 0u) return;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    long long in = 0;
    for (int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; j < L.nnz; j += stride) {
        const uint64_t key = L.key[j];
        if (L.comm[(uint32_t) (key >> 32)] == L.comm[(uint32_t) key]) in += L.w[j];
    }
    lv_u128 sq = 0;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < L.n; i += stride) {
        const lv_u128 t = (lv_u128) (lv_u64) L.tot[i];
        sq += t * t;
    }
    for (int o = 32; o; o >>= 1) {
        in += __shfl_xor(in, o, 64);
        sq += (lv_u128) lv_shfl_xor128((lv_i128) sq, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_in[threadIdx.x >> 6] = in;
        s_lo[threadIdx.x >> 6] = (lv_u64) sq;
        s_hi[threadIdx.x >> 6] = (lv_u64) (sq >> 64);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a = 0;
        lv_u128 q = 0;
        for (int w = 0; w < LV_THREADS / 64; w++) {
            a += s_in[w];
            q += ((lv_u128) s_hi[w] << 64) | (lv_u128) s_lo[w];
        }
        if (a) atomicAdd((lv_u64*) &L.st->intra_new, (lv_u64) a);
        L.part[2 * blockIdx.x] = (lv_u64) q;
        L.part[2 * blockIdx.x + 1] = (lv_u64) (q >> 64);
    }
}
// one wave.  mode 0: the first Qnum of the call (nothing to compare with).  mode 1: a half-round; first_half zeroes the round's
// counters.  The pending list stays as it is for the undo kernel; its length is zeroed here and kept in undo_n.
__global__ void louvain_judge_kernel(lv_level L, int mode, int first_half) {
    const int lane = threadIdx.x;
    lv_state* st = L.st;
    const unsigned int np = L.ctr[K_PEND];
    lv_u128 sq = 0;
    if (mode == 0 || np)
        for (int p = lane; p < LV_PARTS; p += 64) sq += ((lv_u128) L.part[2 * p + 1] << 64) | (lv_u128) L.part[2 * p];
    for (int o = 32; o; o >>= 1) sq += (lv_u128) lv_shfl_xor128((lv_i128) sq, o, 64);
    if (lane != 0) return;
    if (first_half) {
        st->kept = 0u;
        st->rollbacks = 0u;
        st->ovf = 0u;
    }
    st->ovf += L.ctr[K_OVF];
    const long long intra = st->intra_new;
    const lv_i128 qn = (lv_i128) L.m2 * (lv_i128) intra - (lv_i128) sq;
    const lv_i128 q = (lv_i128) (((lv_u128) (lv_u64) st->q_hi << 64) | (lv_u128) st->q_lo);
    unsigned int undo = 0u;
    if (mode == 0 || (np && qn > q)) {
        st->q_lo = (lv_u64) (lv_u128) qn;
        st->q_hi = (long long) (qn >> 64);
        st->intra = intra;
        if (mode) st->kept += np;
    } else if (np) {
        st->rollbacks += 1u;
        undo = np;
    }
    st->undo_n = undo;
    st->intra_new = 0;
    for (int c = 0; c < K_NCTR; c++) L.ctr[c] = 0u;
}
__global__ void __launch_bounds__(LV_THREADS) louvain_undo_kernel(lv_level L) {
    const int64_t n = L.st->undo_n;
    if (n == 0) return;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const int32_t v = L.pend_v[i];
        const lv_u64 kv = (lv_u64) L.k[v];
        L.comm[v] = L.pend_old[i];
        atomicAdd((lv_u64*) &L.tot[L.pend_old[i]], kv);
        atomicAdd((lv_u64*) &L.tot[L.pend_new[i]], 0ull - kv);
    }
}

// ---------------------------------------------------------------- the end of a level
__global__ void __launch_bounds__(LV_THREADS) louvain_flag_kernel(const int32_t* __restrict__ comm, int64_t n, int32_t* __restrict__ flag) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) flag[comm[i]] = 1;
}
// comm[i] = the rank of its label among the labels in use (ascending label order); st->n_next = their number
__global__ void __launch_bounds__(LV_THREADS) louvain_rank_kernel(int32_t* __restrict__ comm, const int32_t* __restrict__ flag,
                                                                  const int32_t* __restrict__ rank, int64_t n, lv_state* st) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        comm[i] = rank[comm[i]];
        if (i == n - 1) st->n_next = rank[i] + flag[i];
    }
}
// the level's map applied to the original vertices' positions in the level
__global__ void __launch_bounds__(LV_THREADS) louvain_compose_kernel(int32_t* __restrict__ of, const int32_t* __restrict__ map, int64_t V) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) of[v] = map[of[v]];
}
// the next level's unmerged entries
__global__ void __launch_bounds__(LV_THREADS) louvain_rekey_kernel(const uint64_t* __restrict__ key, const int64_t* __restrict__ w, int64_t nnz,
                                                                   const int32_t* __restrict__ map, uint64_t* __restrict__ key_out,
                                                                   int64_t* __restrict__ w_out) {
    for (int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; j < nnz; j += (int64_t) gridDim.x * blockDim.x) {
        const uint64_t kk = key[j];
        key_out[j] = ((uint64_t) (uint32_t) map[(uint32_t) (kk >> 32)] << 32) | (uint64_t) (uint32_t) map[(uint32_t) kk];
        w_out[j] = w[j];
    }
}
__global__ void __launch_bounds__(LV_THREADS) louvain_iota_kernel(int32_t* __restrict__ a, int64_t n, int32_t fill, int use_fill) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) a[i] = use_fill ? fill : (int32_t) i;
}
// the smallest member of every community, then every vertex's parent = that member (a forest as gmx_wcc_canon reads it)
__global__ void __launch_bounds__(LV_THREADS) louvain_min_kernel(const int32_t* __restrict__ of, int64_t V, int32_t* __restrict__ minv) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) atomicMin(&minv[of[v]], (int32_t) v);
}
__global__ void __launch_bounds__(LV_THREADS) louvain_parent_kernel(const int32_t* __restrict__ of, const int32_t* __restrict__ minv, int64_t V,
                                                                    int32_t* __restrict__ parent) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) parent[v] = minv[of[v]];
}

// ---------------------------------------------------------------- host
static int lv_grid(int64_t items, int64_t per_block, int max_blocks) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (int) (b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

// key_in / w_in [m] (any order; overwritten) -> the merged level in key / w, *nnz entries, beg[n + 1], k[n].  key_alt / w_alt: scratch [m].
// Synchronises once (the number of merged entries).
static int louvain_contract(uint64_t* key_in, int64_t* w_in, uint64_t* key_alt, int64_t* w_alt, int64_t m, int64_t n, uint64_t* key, int64_t* w,
                            int64_t* beg, int64_t* k, int64_t* count_dev, gmx_pinned<int64_t>& h_count, int64_t* nnz) {
    gmx_ws_scope scope;   // the temporaries of the two rocPRIM calls
    const unsigned int end_bit = 32u + (unsigned int) gmx_bits_for(n);
    size_t sort_bytes = 0, red_bytes = 0;
    GMX_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, key_in, key_alt, w_in, w_alt, (size_t) m, 0u, end_bit, 0));
    GMX_HIP(rocprim::reduce_by_key(nullptr, red_bytes, key_alt, w_alt, (size_t) m, key, w, count_dev, rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), 0));
    wbuf<char> tmp;
    GMX_CHECK(tmp.alloc(sort_bytes > red_bytes ? sort_bytes : red_bytes));
    GMX_HIP(rocprim::radix_sort_pairs((void*) tmp.p, sort_bytes, key_in, key_alt, w_in, w_alt, (size_t) m, 0u, end_bit, 0));
    GMX_HIP(rocprim::reduce_by_key((void*) tmp.p, red_bytes, key_alt, w_alt, (size_t) m, key, w, count_dev, rocprim::plus<int64_t>(), rocprim::equal_to<uint64_t>(), 0));
    GMX_CHECK(gmx_read_back(h_count, (const int64_t*) count_dev));
    *nnz = *h_count.p;
    GMX_HIP(hipMemsetAsync(k, 0, sizeof(int64_t) * (size_t) n, 0));
    hipLaunchKernelGGL(louvain_rows_kernel, dim3(lv_grid(n + 1, LV_THREADS, 4096)), dim3(LV_THREADS), 0, 0, (const uint64_t*) key, *nnz, n, beg);
    hipLaunchKernelGGL(louvain_k_kernel, dim3(lv_grid(*nnz, 8 * LV_THREADS, 4096)), dim3(LV_THREADS), 0, 0, (const uint64_t*) key, (const int64_t*) w, *nnz, k);
    GMX_HIP(hipGetLastError());
    return GMX_OK;
}

extern "C" int gmx_louvain(gmx_graph_t* g, const int32_t* weight_host, int32_t max_levels, int32_t max_rounds, gmx_node_t* comm_host, int32_t* num_comms,
                           int32_t* num_levels, double* modularity, int64_t* intra_out, gmx_stats_t* stats_out) {
    GMX_REQUIRE(g, "NULL argument");
    GMX_REQUIRE(comm_host || g->V == 0, "louvain: comm is NULL");
    GMX_REQUIRE(max_levels >= 0, "louvain: max_levels = %d is negative", (int) max_levels);
    GMX_REQUIRE(max_rounds >= 1, "louvain: max_rounds = %d is below 1", (int) max_rounds);
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V, E = g->E;
    if (num_comms) *num_comms = (int32_t) V;
    if (num_levels) *num_levels = 0;
    if (modularity) *modularity = 0.0;
    if (intra_out) *intra_out = 0;
    stats->vertices_reached = V;
    if (V == 0) return GMX_OK;
    if (E == 0) {   // m2 = 0: nobody has a neighbour
        for (int64_t v = 0; v < V; v++) comm_host[v] = (gmx_node_t) v;
        return GMX_OK;
    }
    // read at every call; no result byte depends on them
    const int64_t wave_min = gmx_env_int("GMX_LOUVAIN_WAVE_MIN", LV_WAVE_MIN, 1, LV_WAVE_MIN_MAX);
    const int64_t block_min = gmx_env_int("GMX_LOUVAIN_BLOCK_MIN", LV_BLOCK_MIN, 1, INT32_MAX);
    int32_t cap = LV_LDS_SLOTS_MIN;   // the power of two at or below the request
    const int64_t want = gmx_env_int("GMX_LOUVAIN_LDS_SLOTS", LV_LDS_SLOTS, LV_LDS_SLOTS_MIN, LV_LDS_SLOTS_MAX);
    while ((int64_t) cap * 2 <= want) cap *= 2;
    const int32_t wcap = cap / LV_WAVE_SHARE;
    const bool phase_log = getenv("GMX_LOUVAIN_PHASES") != nullptr;
    const size_t wave_lds = (size_t) (LV_THREADS / 64) * ((size_t) wcap + (size_t) wcap / 2 + 2) * sizeof(lv_u64);
    const size_t block_lds = ((size_t) cap + (size_t) cap / 2) * sizeof(lv_u64);
    GMX_HIP(hipFuncSetAttribute((const void*) louvain_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) wave_lds));
    GMX_HIP(hipFuncSetAttribute((const void*) louvain_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) block_lds));
    GMX_HIP(hipFuncSetAttribute((const void*) louvain_overflow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) block_lds));

    gmx_ws_scope scope;
    const int64_t M = 2 * E;   // level 0's unmerged entries: every later level has fewer
    wbuf<int32_t> weight, comm, l0, l1, l2, ovf, pend_v, pend_old, pend_new, of, flag, rank, minv, parent, canon, ncomp;
    wbuf<uint64_t> key, key_in, key_alt;
    wbuf<int64_t> w, w_in, w_alt, beg, kk, tot, count;
    wbuf<unsigned int> ctr;
    wbuf<lv_u64> part;
    wbuf<lv_partial> spread;
    wbuf<lv_state> st;
    if (weight_host) GMX_CHECK(weight.alloc(E));
    GMX_CHECK(key.alloc(M));
    GMX_CHECK(key_in.alloc(M));
    GMX_CHECK(key_alt.alloc(M));
    GMX_CHECK(w.alloc(M));
    GMX_CHECK(w_in.alloc(M));
    GMX_CHECK(w_alt.alloc(M));
    GMX_CHECK(beg.alloc(V + 1));
    GMX_CHECK(kk.alloc(V));
    GMX_CHECK(tot.alloc(V));
    GMX_CHECK(count.alloc(1));
    GMX_CHECK(comm.alloc(V));
    GMX_CHECK(l0.alloc(V));
    GMX_CHECK(l1.alloc(V));
    GMX_CHECK(l2.alloc(V));
    GMX_CHECK(ovf.alloc(V));
    GMX_CHECK(pend_v.alloc(V));
    GMX_CHECK(pend_old.alloc(V));
    GMX_CHECK(pend_new.alloc(V));
    GMX_CHECK(of.alloc(V));
    GMX_CHECK(flag.alloc(V));
    GMX_CHECK(rank.alloc(V));
    GMX_CHECK(minv.alloc(V));
    GMX_CHECK(parent.alloc(V));
    GMX_CHECK(canon.alloc(V));
    GMX_CHECK(ncomp.alloc(1));
    GMX_CHECK(ctr.alloc(K_NCTR));
    GMX_CHECK(part.alloc(2 * LV_PARTS));
    GMX_CHECK(spread.alloc((size_t) LV_SPREAD_ROWS * LV_SPREAD));
    GMX_CHECK(st.alloc(1));
    size_t scan_bytes = 0;
    GMX_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag.p, rank.p, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
    wbuf<char> scan_tmp;
    GMX_CHECK(scan_tmp.alloc(scan_bytes));
    gmx_pinned<lv_state> h_st;
    GMX_CHECK(h_st.alloc());
    gmx_pinned<int64_t> h_count;
    GMX_CHECK(h_count.alloc());
    gmx_pinned<int32_t> h_ncomp;
    GMX_CHECK(h_ncomp.alloc());
    gmx_spans tm;
    gmx_phase_clock phase;   // GMX_LOUVAIN_PHASES (synchronises: the profiler's mode only)
    GMX_CHECK(phase.enable(phase_log));

    // ---- the weights: uploaded by the caller's slots, checked and added up by a device pass before anything else
    GMX_HIP(hipMemsetAsync(st.p, 0, sizeof(lv_state), 0));
    int64_t m2 = 2 * E;
    if (weight_host) {
        GMX_CHECK(tm.begin(tm.H2D));
        GMX_HIP(hipMemcpyAsync(weight.p, weight_host, sizeof(int32_t) * (size_t) E, hipMemcpyHostToDevice, 0));
        GMX_CHECK(tm.end(tm.H2D));
        hipLaunchKernelGGL(louvain_weight_kernel, dim3(lv_grid(E, LV_THREADS, 2048)), dim3(LV_THREADS), 0, 0, (const int32_t*) weight.p, E, st.p);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_st, (const lv_state*) st.p));
        GMX_REQUIRE(h_st.p->bad_weight == 0u, "louvain: a weight is below 1");
        m2 = 2 * (int64_t) h_st.p->weight_sum;
    }

    lv_level L{};
    L.beg = beg.p;
    L.key = key.p;
    L.w = w.p;
    L.k = kk.p;
    L.comm = comm.p;
    L.tot = tot.p;
    L.list[0] = l0.p;
    L.list[1] = l1.p;
    L.list[2] = l2.p;
    L.ovf = ovf.p;
    L.pend_v = pend_v.p;
    L.pend_old = pend_old.p;
    L.pend_new = pend_new.p;
    L.ctr = ctr.p;
    L.part = part.p;
    L.spread = spread.p;
    L.st = st.p;
    L.m2 = m2;

    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_HIP(hipMemsetAsync(ctr.p, 0, sizeof(unsigned int) * K_NCTR, 0));
    const int gV = lv_grid(V, LV_THREADS, 4096);
    hipLaunchKernelGGL(louvain_iota_kernel, dim3(gV), dim3(LV_THREADS), 0, 0, of.p, V, 0, 0);
    // ---- level 0: the doubled slot list, merged
    float contract_ms = 0;
    phase.begin();
    hipLaunchKernelGGL(louvain_pairs_kernel, dim3(lv_grid(E, LV_THREADS, 4096)), dim3(LV_THREADS), 0, 0, (const int32_t*) g->begin.p,
                       (const int32_t*) g->node_idx.p, weight_host ? (const int32_t*) weight.p : (const int32_t*) nullptr,
                       (const int32_t*) g->e_idx2idx.p, V, E, key_in.p, w_in.p);
    GMX_HIP(hipGetLastError());
    int64_t n = V, nnz = 0;
    GMX_CHECK(louvain_contract(key_in.p, w_in.p, key_alt.p, w_alt.p, M, n, key.p, w.p, beg.p, kk.p, count.p, h_count, &nnz));
    contract_ms = phase.end();
    L.n = n;
    L.nnz = nnz;
    hipLaunchKernelGGL(louvain_init_kernel, dim3(lv_grid(n, LV_THREADS, 4096)), dim3(LV_THREADS), 0, 0, L);
    hipLaunchKernelGGL(louvain_measure_kernel, dim3(LV_PARTS), dim3(LV_THREADS), 0, 0, L, 1);
    hipLaunchKernelGGL(louvain_judge_kernel, dim3(1), dim3(64), 0, 0, L, 0, 1);
    GMX_HIP(hipGetLastError());

    int32_t levels = 0;
    int64_t rounds = 0, kept_rounds = 0, rollbacks = 0, cuts = 0, moves = 0, examined = 0, overflowed = 0;
    std::string sizes;
    for (int32_t lvl = 0; lvl < max_levels; lvl++) {
        char buf[64];
        snprintf(buf, sizeof(buf), "%s%lld/%lld", lvl ? "," : "", (long long) n, (long long) nnz);
        sizes += buf;
        if (phase_log)
            fprintf(stderr, "gmx louvain level %d: n %lld nnz %lld contract %.3f ms\n", (int) lvl, (long long) n, (long long) nnz, contract_ms);
        const int g_n = lv_grid(n, LV_THREADS, 2048);
        const int g_short = lv_grid(n, 16, 2048);   // 16 rows per workgroup
        const int g_wave = lv_grid(n, 4, 1280);     // a wave per row
        const int g_block = lv_grid(n, 1, 1024);    // a workgroup per row
        const int g_ovf = lv_grid(n * LV_SPREAD, 1, 2048);   // a workgroup per share of an overflowed row
        int64_t level_moves = 0;
        bool ended = false;   // a round kept no move
        for (int32_t r = 0; r < max_rounds && !ended; r++) {
            const uint32_t salt = (uint32_t) r * 0x9E3779B9u;
            float pt[2] = {0, 0};
            for (int half = 0; half < 2; half++) {
                phase.begin();
                hipLaunchKernelGGL(louvain_compact_kernel, dim3(g_n), dim3(LV_THREADS), 0, 0, L, salt, half, wave_min, block_min);
                hipLaunchKernelGGL(louvain_short_kernel, dim3(g_short), dim3(LV_THREADS), 0, 0, L);
                hipLaunchKernelGGL(louvain_wave_kernel, dim3(g_wave), dim3(LV_THREADS), wave_lds, 0, L, wcap);
                hipLaunchKernelGGL(louvain_block_kernel, dim3(g_block), dim3(LV_THREADS), block_lds, 0, L, cap);
                hipLaunchKernelGGL(louvain_overflow_kernel, dim3(g_ovf), dim3(LV_THREADS), block_lds, 0, L, cap);
                hipLaunchKernelGGL(louvain_final_kernel, dim3(LV_SPREAD_ROWS / LV_THREADS), dim3(LV_THREADS), 0, 0, L);
                phase.end(&pt[0]);
                phase.begin();
                hipLaunchKernelGGL(louvain_commit_kernel, dim3(g_n), dim3(LV_THREADS), 0, 0, L);
                hipLaunchKernelGGL(louvain_measure_kernel, dim3(LV_PARTS), dim3(LV_THREADS), 0, 0, L, 0);
                hipLaunchKernelGGL(louvain_judge_kernel, dim3(1), dim3(64), 0, 0, L, 1, half == 0 ? 1 : 0);
                hipLaunchKernelGGL(louvain_undo_kernel, dim3(g_n), dim3(LV_THREADS), 0, 0, L);
                phase.end(&pt[1]);
            }
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_st, (const lv_state*) st.p));   // the round's record
            const lv_state& R = *h_st.p;
            rounds++;
            examined += nnz;
            rollbacks += R.rollbacks;
            overflowed += R.ovf;
            level_moves += R.kept;
            if (phase_log)
                fprintf(stderr, "gmx louvain level %d round %d: kept %u rollbacks %u overflowed %u evaluate %.3f ms judge %.3f ms\n", (int) lvl, (int) r,
                        R.kept, R.rollbacks, R.ovf, pt[0], pt[1]);
            if (R.kept == 0) ended = true;
            else kept_rounds++;
        }
        if (!ended) cuts++;
        if (level_moves == 0) break;
        moves += level_moves;
        levels++;
        // ---- the level's labels in use, renumbered in ascending order; the original vertices follow; the next level
        phase.begin();
        GMX_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t) * (size_t) n, 0));
        hipLaunchKernelGGL(louvain_flag_kernel, dim3(g_n), dim3(LV_THREADS), 0, 0, (const int32_t*) comm.p, n, flag.p);
        GMX_HIP(rocprim::exclusive_scan((void*) scan_tmp.p, scan_bytes, flag.p, rank.p, 0, (size_t) n, rocprim::plus<int32_t>(), 0));
        hipLaunchKernelGGL(louvain_rank_kernel, dim3(g_n), dim3(LV_THREADS), 0, 0, comm.p, (const int32_t*) flag.p, (const int32_t*) rank.p, n, st.p);
        hipLaunchKernelGGL(louvain_compose_kernel, dim3(gV), dim3(LV_THREADS), 0, 0, of.p, (const int32_t*) comm.p, V);
        GMX_HIP(hipGetLastError());
        if (lvl + 1 == max_levels) {
            phase.end();
            break;
        }
        GMX_CHECK(gmx_read_back(h_st, (const lv_state*) st.p));
        const int64_t n_next = h_st.p->n_next;
        hipLaunchKernelGGL(louvain_rekey_kernel, dim3(lv_grid(nnz, LV_THREADS, 4096)), dim3(LV_THREADS), 0, 0, (const uint64_t*) key.p, (const int64_t*) w.p,
                           nnz, (const int32_t*) comm.p, key_in.p, w_in.p);
        GMX_HIP(hipGetLastError());
        int64_t nnz_next = 0;
        GMX_CHECK(louvain_contract(key_in.p, w_in.p, key_alt.p, w_alt.p, nnz, n_next, key.p, w.p, beg.p, kk.p, count.p, h_count, &nnz_next));
        n = n_next;
        nnz = nnz_next;
        L.n = n;
        L.nnz = nnz;
        hipLaunchKernelGGL(louvain_init_kernel, dim3(lv_grid(n, LV_THREADS, 4096)), dim3(LV_THREADS), 0, 0, L);
        GMX_HIP(hipGetLastError());
        contract_ms = phase.end();
    }

    // ---- the numbering: communities by ascending smallest member, as gmx_wcc numbers components
    hipLaunchKernelGGL(louvain_iota_kernel, dim3(gV), dim3(LV_THREADS), 0, 0, minv.p, V, INT32_MAX, 1);
    hipLaunchKernelGGL(louvain_min_kernel, dim3(gV), dim3(LV_THREADS), 0, 0, (const int32_t*) of.p, V, minv.p);
    hipLaunchKernelGGL(louvain_parent_kernel, dim3(gV), dim3(LV_THREADS), 0, 0, (const int32_t*) of.p, (const int32_t*) minv.p, V, parent.p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_wcc_canon(parent.p, V, flag.p, rank.p, canon.p, ncomp.p));
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpyAsync(comm_host, canon.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    GMX_HIP(hipMemcpyAsync(h_ncomp.p, ncomp.p, sizeof(int32_t), hipMemcpyDeviceToHost, 0));
    GMX_HIP(hipMemcpyAsync(h_st.p, st.p, sizeof(lv_state), hipMemcpyDeviceToHost, 0));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    const lv_state& R = *h_st.p;
    const __int128 qnum = (__int128) (((unsigned __int128) (lv_u64) R.q_hi << 64) | (unsigned __int128) R.q_lo);
    const double q = (double) qnum / ((double) m2 * (double) m2);
    if (num_comms) *num_comms = *h_ncomp.p;
    if (num_levels) *num_levels = levels;
    if (modularity) *modularity = q;
    if (intra_out) *intra_out = R.intra;
    stats->iterations = (int32_t) kept_rounds;
    stats->vertices_reached = *h_ncomp.p;
    stats->edges_examined = examined;
    if (getenv("GMX_LOUVAIN_LOG"))
        fprintf(stderr, "gmx louvain: V %lld E %lld weighted %d levels %d rounds %lld rollbacks %lld cuts %lld moves %lld sizes %s comms %d intra %lld overflowed %lld\n",
                (long long) V, (long long) E, weight_host ? 1 : 0, (int) levels, (long long) rounds, (long long) rollbacks, (long long) cuts, (long long) moves,
                sizes.empty() ? "-" : sizes.c_str(), (int) *h_ncomp.p, (long long) R.intra, (long long) overflowed);
    return GMX_OK;
}

void gmx_touch_louvain() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) louvain_init_kernel);
}
