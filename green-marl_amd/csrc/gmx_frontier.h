// gmx_frontier.h -- the merge-path frontier tile: how the queue-driven kernels (top-down BFS level, sssp / sssp_path
// relaxation, avg_teen_cnt without a reverse CSR) expand a queue of vertices.
//
// The host takes the out-degrees of the queue q[0..n), prefix-sums them into off[0..n] (off[n] = m edges) and cuts the
// merged sequence (n row ends, m edges) into tiles of BFS_ITEMS items: gmx_frontier_offsets().  A tile's workgroup finds
// its two diagonals (frontier_tile_search / frontier_tile_split), stages the rows it touches in LDS (frontier_stage),
// finds the row of each of its edges there (frontier_slot), appends what it discovers to an LDS list with one ballot per
// wave (wave_append) and claims the queue tail once (frontier_flush).
//
// Next to the tile, what the round kernels built on it share: the 64-lane reductions (wave_sum / wave_min / wave_max), the
// row of a slot (csr_row_of), the walk of a short queue by one workgroup (tail_rows) and the kernels that stage an edge
// property (gather_by_order_kernel, first_bad_slot_kernel).
#ifndef GMX_FRONTIER_H_
#define GMX_FRONTIER_H_

#include "gmx_internal.h"

#define BFS_THREADS 256
#define BFS_ITEMS 2048   // merge-path items (frontier vertices + their out-edges) per workgroup

// Statistics that thousands of waves add to (edges inspected, vertices found by a bottom-up level) are spread over
// BFS_SHARDS cache lines and summed by the host after the read-back: atomics on ONE line retire at ~90 per
// microsecond device-wide, and two such adds per wave were 0.37 ms of a 0.39 ms bottom-up level at RMAT-20 (and
// ~0.7 ms per bottom-up level at RMAT-26).  Both run on: a level's count is the difference to the previous total.
#define BFS_SHARDS 64
struct bfs_counters {
    unsigned long long next_count;     // top-down: tail of the next queue = vertices discovered in this level
    unsigned long long next_edges;     // their out-edges: the next level's merge-path length and the input of the
                                       // direction decision, known without a pass over the new queue
    unsigned long long pad0[14];
    struct {
        unsigned long long edges;      // edges inspected so far
        unsigned long long found;      // vertices found by bottom-up levels so far
        unsigned long long pad[14];
    } shard[BFS_SHARDS];
};
static inline void bfs_totals(const bfs_counters& h, unsigned long long* edges, unsigned long long* found) {
    unsigned long long e = 0, f = 0;
    for (int i = 0; i < BFS_SHARDS; i++) {
        e += h.shard[i].edges;
        f += h.shard[i].found;
    }
    *edges = e;
    *found = f;
}

static inline int grid_for(int64_t n, int block = BFS_THREADS, int max_blocks = 256 * 8) {
    int64_t b = (n + block - 1) / block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int) b;
}

// ---- host: the offsets of a queue (gmx_bfs.hip)
struct frontier_scan {
    dbuf<int32_t> deg;     // [max_n]
    dbuf<int64_t> off;     // [max_n + 2]
    dbuf<int64_t> split;   // [max_tiles]: rows consumed at every tile boundary (empty: the kernels search themselves)
    dbuf<char> scan_tmp;
    size_t scan_bytes = 0;
};
int gmx_frontier_scan_alloc(frontier_scan* s, size_t max_n, size_t max_tiles);
// q[0..n) -> s->off[0..n] on the default stream.  h_m (pinned, or NULL: nothing is read back and nobody waits): off[n],
// the queue's edges, after a stream synchronisation; with_split (needs h_m): s->split[0..nb] for the nb tiles as well.
int gmx_frontier_offsets(const int32_t* begin, const int32_t* q, int64_t n, frontier_scan* s, int64_t* h_m, bool with_split);
static inline int64_t frontier_tiles(int64_t n, int64_t m) { return (n + m + BFS_ITEMS - 1) / BFS_ITEMS; }

__device__ __forceinline__ void bfs_count(bfs_counters* __restrict__ ctr, unsigned long long edges, unsigned long long found) {
    const int sh = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (BFS_SHARDS - 1);
    if (edges) atomicAdd(&ctr->shard[sh].edges, edges);
    if (found) atomicAdd(&ctr->shard[sh].found, found);
}

// rows consumed at diagonal dk <= n + m of the merged (n row ends, m edges) sequence
__device__ __forceinline__ int64_t frontier_diagonal(const int64_t* __restrict__ off, int64_t n, int64_t m, int64_t dk) {
    int64_t lo = dk > m ? dk - m : 0, hi = dk < n ? dk : n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] <= dk - mid - 1) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// tile blockIdx.x: (rows, edges) consumed at its two diagonals
struct frontier_tile {
    int64_t v0, e0, v1, e1;
};
// ... searched by the workgroup's first two threads (log2(n) dependent loads each: for the kernels that must not pay a
// launch for the split array); s_split: 2 x 2 words of LDS
__device__ __forceinline__ frontier_tile frontier_tile_search(const int64_t* __restrict__ off, int64_t n, int64_t m, int64_t (*s_split)[2]) {
    const int tid = threadIdx.x;
    if (tid < 2) {
        int64_t dk = ((int64_t) blockIdx.x + tid) * BFS_ITEMS;
        if (dk > n + m) dk = n + m;
        const int64_t lo = frontier_diagonal(off, n, m, dk);
        s_split[tid][0] = lo;
        s_split[tid][1] = dk - lo;
    }
    __syncthreads();
    return frontier_tile{s_split[0][0], s_split[0][1], s_split[1][0], s_split[1][1]};
}
// ... read from the split array of gmx_frontier_offsets
__device__ __forceinline__ frontier_tile frontier_tile_split(const int64_t* __restrict__ split, int64_t n, int64_t m) {
    int64_t d0 = (int64_t) blockIdx.x * BFS_ITEMS, d1 = d0 + BFS_ITEMS;
    if (d1 > n + m) d1 = n + m;
    const int64_t v0 = split[blockIdx.x], v1 = split[blockIdx.x + 1];
    return frontier_tile{v0, d0 - v0, v1, d1 - v1};
}

// The rows the tile touches, v0 .. v1 (the last one may be partial, or == n), into s_off[] / s_row[] (BFS_ITEMS + 2 each:
// a tile of BFS_ITEMS row ends, the partial row and the sentinel); payload(i, v, in_range) stages whatever else the kernel
// keeps per row.  Ends with a barrier; returns the number of rows staged.
template <class Payload>
__device__ __forceinline__ int frontier_stage(const frontier_tile& t, const int32_t* __restrict__ begin, const int32_t* __restrict__ cur_q, int64_t n,
                                              const int64_t* __restrict__ off, int64_t m, int64_t* s_off, int32_t* s_row, Payload payload) {
    const int nv = (int) (t.v1 - t.v0) + 1;
    for (int i = threadIdx.x; i < nv; i += BFS_THREADS) {
        const int64_t vi = t.v0 + i;
        s_off[i] = vi <= n ? off[vi < n ? vi : n] : m;
        const int32_t v = vi < n ? cur_q[vi] : 0;
        s_row[i] = vi < n ? begin[v] : 0;
        payload(i, v, vi < n);
    }
    if (threadIdx.x == 0) s_off[nv] = m + 1;   // sentinel
    __syncthreads();
    return nv;
}

// staged row of edge x: the last i with s_off[i] <= x
template <class Off>
__device__ __forceinline__ int frontier_slot(const Off* s_off, int nv, int64_t x) {
    int lo = 0, hi = nv - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t) s_off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the lanes of a wave that have a vertex for a list (in LDS, or a queue in memory) claim its tail together: one atomic
// per wave.  Every lane of the wave must be here; the appending lanes then run also() -- inside the claim's branch: with
// the winners' sum of out-degrees as a statement of its own behind the append, bfs_topdown_kernel took 87 VGPRs for 52.
template <class Count, class Also>
__device__ __forceinline__ void wave_append(bool on, int32_t v, int32_t* list, Count* count, int lane, Also also) {
    const unsigned long long mk = __ballot(on);
    if (mk) {
        const int leader = __ffsll((long long) mk) - 1;
        Count at = 0;
        if (lane == leader) at = atomicAdd(count, (Count) __popcll(mk));
        at = __shfl(at, leader, 64);
        if (on) {
            list[at + __popcll(mk & ((1ULL << lane) - 1))] = v;
            also();
        }
    }
}
template <class Count>
__device__ __forceinline__ void wave_append(bool on, int32_t v, int32_t* list, Count* count, int lane) {
    wave_append(on, v, list, count, lane, [] {});
}

// the workgroup's LDS list goes to the queue: thread 0 claims the tail once (and does what else belongs to the claim:
// with_claim()), everybody copies.  Called by the whole workgroup after the barrier that completes s_list.
template <class WithClaim>
__device__ __forceinline__ void frontier_flush(const int32_t* s_list, unsigned int cnt, unsigned long long* tail, int32_t* __restrict__ q,
                                               unsigned long long* s_base, WithClaim with_claim) {
    if (threadIdx.x == 0) {
        if (cnt) *s_base = atomicAdd(tail, (unsigned long long) cnt);
        with_claim();
    }
    __syncthreads();
    for (unsigned int i = threadIdx.x; i < cnt; i += BFS_THREADS) q[*s_base + i] = s_list[i];
}
__device__ __forceinline__ void frontier_flush(const int32_t* s_list, unsigned int cnt, unsigned long long* tail, int32_t* __restrict__ q,
                                               unsigned long long* s_base) {
    frontier_flush(s_list, cnt, tail, q, s_base, [] {});
}

// ---- 64-lane reductions (T: a 32- or 64-bit word); every lane of the wave must be here, the result is in lane 0
template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    return x;
}
template <class T>
__device__ __forceinline__ T wave_min(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T y = __shfl_down(x, o, 64);
        x = y < x ? y : x;
    }
    return x;
}
template <class T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T y = __shfl_down(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

// the row that holds slot e: the last row that starts at or before it (the empty rows before it start there too)
__device__ __forceinline__ int32_t csr_row_of(const int32_t* __restrict__ begin, int64_t V, uint32_t e) {
    int64_t lo = 0, hi = V - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((uint32_t) begin[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return (int32_t) lo;
}

// ---- the tail walk: the rows of a short queue la[0 .. n) by the waves of ONE workgroup (wave `wave` of `nwaves`, all of
// them here with the same n), 64 rows at a time, a lane per row.  load(have, v, deg) -> P is called by every lane once per
// 64 rows (have: the lane has row v of deg slots) and returns what the row's slots need besides their index.
// slot(on, P, e) is called by the WHOLE wave at every step -- it may ballot, as wave_append does -- with on false in the
// lanes that have no slot e:
//   - a row of at most LANE_MAX slots is walked by its lane: step k takes slot k of every such row, and the loop ends at the
//     first k no lane has a slot for, which the ballot makes the same k in all 64 lanes;
//   - a longer row is walked by the wave, 64 slots a step: its bounds and P come from its lane by __shfl, so the trip count
//     is wave-uniform again.
// Nothing orders the slots of different rows; the caller puts its barrier behind the walk.
template <int LANE_MAX, class Load, class Slot>
__device__ __forceinline__ void tail_rows(const int32_t* la, int64_t n, const int32_t* begin, int lane, int64_t wave, int64_t nwaves, Load load,
                                          Slot slot) {
    for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
        const bool have = base + lane < n;
        const int32_t v = have ? la[base + lane] : 0;
        const int32_t b = have ? begin[v] : 0, e = have ? begin[v + 1] : 0;
        const auto p = load(have, v, e - b);
        const bool by_wave = e - b > LANE_MAX;
        for (int32_t k = 0; k < LANE_MAX; k++) {
            const bool on = !by_wave && b + k < e;
            if (!__ballot(on)) break;   // (wave-uniform)
            slot(on, p, b + k);
        }
        unsigned long long lm = __ballot(by_wave);
        while (lm) {
            const int src = __builtin_ctzll(lm);
            lm &= lm - 1;
            const int32_t wb = __shfl(b, src, 64), we = __shfl(e, src, 64);
            const auto wp = __shfl(p, src, 64);
            for (int32_t x = wb; x < we; x += 64) slot(x + lane < we, wp, x + lane);
        }
    }
}

// ---- an edge property on its way to the device's slots
// dst[i] = src[order[i]]: a property given by uploaded slot brought into the order of the sorted rows; a slot map composed
template <class T>
__global__ void gather_by_order_kernel(const T* __restrict__ src, const int32_t* __restrict__ order, int64_t n, T* __restrict__ dst) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = src[order[i]];
}

// out->bad = E - (the first slot i with !(x[i] >= 0): negative or, for a double, not a number; -0.0 passes), 0: none.
// Ctl: the caller's control block, bad an unsigned 64-bit word of it that starts at 0.  Launched with the unit's own block
// size, which must not exceed BFS_THREADS (the units assert that theirs equals it).
template <class T, class Ctl>
__global__ void __launch_bounds__(BFS_THREADS) first_bad_slot_kernel(const T* __restrict__ x, int64_t E, Ctl* __restrict__ out) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long worst = 0;
    for (; i < E; i += stride)
        if (!(x[i] >= 0)) {
            const unsigned long long w = (unsigned long long) (E - i);
            worst = w > worst ? w : worst;
        }
    worst = wave_max(worst);
    if ((threadIdx.x & 63) == 0 && worst) atomicMax(&out->bad, worst);
}

#endif
