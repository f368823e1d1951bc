// gmx_nbrcount.hip -- avg_teen_cnt and conduct (counts over neighbours with an integer node property) for gfx950.
#include "gmx_frontier.h"

#include <float.h>
#include <limits.h>
#include <string.h>
#include <rocprim/rocprim.hpp>

// ------------------------------------------------------------------ avg_teen_cnt, conduct
// Count-reductions over neighbours with an integer node property (/root/reference/apps/src/avg_teen_cnt.gm,
// conduct.gm).  With the rows to count in at hand (the reverse CSR for avg_teen_cnt, the forward one for conduct) a row
// walks its neighbours and probes the predicate as a bitmap (count_by_bitmap below).  avg_teen_cnt on a forward-only
// upload pushes instead: the vertices that pass the filter are queued (ballot-aggregated append), their out-degrees
// prefix-summed and the edges cut by merge-path as in a top-down BFS level, and every edge does cnt[dst] += 1.
// Integer arithmetic only; the final float is formed on the host from the exact integers with the emitted expression,
// so results are bit-identical.
__global__ void __launch_bounds__(BFS_THREADS)
edge_count_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ node_idx,
                  const int32_t* __restrict__ cur_q, int64_t n, const int64_t* __restrict__ off, int64_t m,
                  int32_t* __restrict__ cnt) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int64_t s_split[2][2];
    const int tid = threadIdx.x;
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, begin, cur_q, n, off, m, s_off, s_row, [](int, int32_t, bool) {});
    for (int64_t x = t.e0 + tid; x < t.e1; x += BFS_THREADS) {
        const int lo = frontier_slot(s_off, nv, x);
        atomicAdd(&cnt[node_idx[(int64_t) s_row[lo] + (x - s_off[lo])]], 1);
    }
}

// filter: 0: 10 <= prop < 20 (teen), 1: prop == num
__global__ void select_queue_kernel(const int32_t* __restrict__ prop, int64_t V, int filter, int32_t num,
                                    int32_t* __restrict__ q, unsigned long long* __restrict__ qcount) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    const int64_t vend = (V + 63) / 64 * 64;
    for (; v < vend; v += stride) {
        bool in = false;
        if (v < V) {
            const int32_t p = prop[v];
            in = filter == 0 ? (p >= 10 && p < 20) : (p == num);
        }
        wave_append(in, (int32_t) v, q, qcount, threadIdx.x & 63);
    }
}

// out[0] += sum of val[v] (or of the out-degree) over the vertices passing the test, out[1] += their number
//   test 0: prop[v] > num   test 1: prop[v] == num   test 2: prop[v] != num
__global__ void filtered_sum_kernel(const int32_t* __restrict__ prop, const int32_t* __restrict__ val, const int32_t* __restrict__ begin,
                                    int64_t V, int test, int32_t num, unsigned long long* __restrict__ out) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long s = 0, c = 0;
    for (; v < V; v += stride) {
        const int32_t p = prop[v];
        const bool ok = test == 0 ? p > num : test == 1 ? p == num : p != num;
        if (ok) {
            s += (unsigned long long) (long long) (val ? val[v] : begin[v + 1] - begin[v]);
            c++;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o, 64);
        c += __shfl_down(c, o, 64);
    }
    // one pair of adds per workgroup (a pair per wave, all on one cache line, was 225 us of adds for a 20 us pass)
    __shared__ unsigned long long s_s[BFS_THREADS / 64], s_c[BFS_THREADS / 64];
    if ((threadIdx.x & 63) == 0) {
        s_s[threadIdx.x >> 6] = s;
        s_c[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long ts = 0, tc = 0;
        for (int i = 0; i < (int) (blockDim.x >> 6); i++) {
            ts += s_s[i];
            tc += s_c[i];
        }
        if (ts) atomicAdd(&out[0], ts);
        if (tc) atomicAdd(&out[1], tc);
    }
}

// queue the vertices passing `filter`, then cnt[dst] += 1 over their out-edges
static int expand_selected(gmx_graph* g, const int32_t* prop, int filter, int32_t num, int32_t* cnt) {
    const int64_t V = g->V;
    dbuf<int32_t> q;
    frontier_scan fs;
    dbuf<unsigned long long> qcount;
    gmx_pinned<int64_t> h_mf;
    GMX_CHECK(q.alloc((size_t) V));
    GMX_CHECK(gmx_frontier_scan_alloc(&fs, (size_t) V, 0));
    GMX_CHECK(qcount.alloc(1));
    GMX_CHECK(h_mf.alloc());
    GMX_HIP(hipMemset(qcount.p, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(select_queue_kernel, dim3(grid_for(V, BFS_THREADS, 256 * 16)), dim3(BFS_THREADS), 0, 0, prop, V, filter, num, q.p, qcount.p);
    unsigned long long nq = 0;
    GMX_HIP(hipMemcpy(&nq, qcount.p, sizeof(nq), hipMemcpyDeviceToHost));
    if (nq == 0) return GMX_OK;
    GMX_CHECK(gmx_frontier_offsets(g->begin.p, q.p, (int64_t) nq, &fs, h_mf.p, false));
    const int64_t m_f = *h_mf.p, nb = frontier_tiles((int64_t) nq, m_f);
    if (nb > 0)
        hipLaunchKernelGGL(edge_count_kernel, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, g->begin.p, g->node_idx.p,
                           (const int32_t*) q.p, (int64_t) nq, (const int64_t*) fs.off.p, m_f, cnt);
    GMX_HIP(hipGetLastError());
    return GMX_OK;
}

// Pull formulation with the predicate as a bitmap (V/8 bytes: resident in every L2): a row walks its neighbour
// list and probes the bitmap -- no atomics, no gathers from a V-sized array.  Rows longer than ROWCNT_LONG are
// left to whole waves.  mode bits: 1 = count the neighbours whose bit is CLEAR (else set); rows are taken only
// if their own bit in `row_bm` is set (row_bm == NULL: all rows).  Per-row counts go to cnt (if given), their
// sum to total (if given).
#define ROWCNT_LONG 256
__global__ void pred_bitmap_kernel(const int32_t* __restrict__ prop, int64_t V, int filter, int32_t num, unsigned long long* __restrict__ bm64) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    const int64_t vend = (V + 63) / 64 * 64;
    for (; v < vend; v += stride) {
        bool in = false;
        if (v < V) {
            const int32_t p = prop[v];
            in = filter == 0 ? (p >= 10 && p < 20) : (p == num);
        }
        const unsigned long long m = __ballot(in);
        if ((threadIdx.x & 63) == 0) bm64[v >> 6] = m;
    }
}

__global__ void __launch_bounds__(BFS_THREADS)
row_count_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V,
                 const uint32_t* __restrict__ row_bm, const uint32_t* __restrict__ probe_bm, int invert,
                 int32_t* __restrict__ cnt, int32_t* __restrict__ long_rows, unsigned long long* __restrict__ nlong,
                 unsigned long long* __restrict__ total) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long acc = 0;
    for (; v < V; v += stride) {
        if (row_bm && !((row_bm[v >> 5] >> (v & 31)) & 1u)) {
            if (cnt) cnt[v] = 0;
            continue;
        }
        const int32_t b = begin[v], e = begin[v + 1];
        if (e - b > ROWCNT_LONG) {
            long_rows[atomicAdd(nlong, 1ULL)] = (int32_t) v;
            continue;
        }
        int32_t c = 0;
        for (int32_t i = b; i < e; i++) {
            const int32_t w = idx[i];
            const unsigned bit = (probe_bm[w >> 5] >> (w & 31)) & 1u;
            c += invert ? (int32_t) (bit ^ 1u) : (int32_t) bit;
        }
        if (cnt) cnt[v] = c;
        acc += (unsigned long long) c;
    }
    if (total) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if ((threadIdx.x & 63) == 0 && acc) atomicAdd(total, acc);
    }
}

__global__ void __launch_bounds__(BFS_THREADS)
row_count_long_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, const int32_t* __restrict__ long_rows,
                      unsigned long long nlong, const uint32_t* __restrict__ probe_bm, int invert,
                      int32_t* __restrict__ cnt, unsigned long long* __restrict__ total) {
    const int lane = threadIdx.x & 63;
    unsigned long long wave = ((unsigned long long) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned long long nwaves = ((unsigned long long) gridDim.x * blockDim.x) >> 6;
    unsigned long long acc = 0;
    for (; wave < nlong; wave += nwaves) {
        const int32_t v = long_rows[wave];
        const int32_t b = begin[v], e = begin[v + 1];
        unsigned long long c = 0;
        for (int32_t i = b + lane; i < e; i += 64) {
            const int32_t w = idx[i];
            const unsigned bit = (probe_bm[w >> 5] >> (w & 31)) & 1u;
            c += invert ? (bit ^ 1u) : bit;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
        if (lane == 0) {
            if (cnt) cnt[v] = (int32_t) c;
            acc += c;
        }
    }
    if (total && lane == 0 && acc) atomicAdd(total, acc);
}

// The same count over the FLAT slot array (round 3): a workgroup takes ROWCNT_ITEMS consecutive items of the merged sequence
// (row ends, slots) -- merge-path over begin[], as in the top-down BFS level -- so that the slots are read coalesced, eight per
// thread and all in flight, whatever the rows look like; a slot finds its row by bisection in the LDS copy of the range's
// begin[] and adds its bit to the row's LDS counter.  With one row per lane (above) every lane walked its own list: 4-byte
// loads, one 64-byte request each -- RMAT-24: avg_teen_cnt 6.1 ms, conduct 5.0 ms for 1 GB of slots.
#define ROWCNT_ITEMS 2048
// rows consumed at the diagonals k * ROWCNT_ITEMS, k = 0 .. nb: one thread per diagonal.  (Searched by the workgroups
// themselves -- two threads, 24 dependent loads over begin[], everybody else at the barrier -- this was 19 of the ~27 us a
// workgroup took.)
__global__ void row_count_split_kernel(const int32_t* __restrict__ begin, int64_t V, int64_t E, int64_t nb, int64_t* __restrict__ split) {
    const int64_t k = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nb) return;
    int64_t dk = k * ROWCNT_ITEMS;
    if (dk > V + E) dk = V + E;
    int64_t lo = dk > E ? dk - E : 0, hi = dk < V ? dk : V;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t) begin[mid + 1] <= dk - mid - 1) lo = mid + 1; else hi = mid;
    }
    split[k] = lo;
}

__global__ void __launch_bounds__(BFS_THREADS)
row_count_flat_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int64_t E, const int64_t* __restrict__ split,
                      const uint32_t* __restrict__ row_bm, const uint32_t* __restrict__ probe_bm, int invert,
                      int32_t* __restrict__ cnt /* zeroed */, unsigned long long* __restrict__ total) {
    __shared__ int32_t s_off[ROWCNT_ITEMS + 2];
    __shared__ int32_t s_cnt[ROWCNT_ITEMS + 2];
    const int tid = threadIdx.x;
    // merge-path split of the diagonals k * ITEMS and (k + 1) * ITEMS: (rows consumed, slots consumed)
    int64_t d0 = (int64_t) blockIdx.x * ROWCNT_ITEMS, d1 = d0 + ROWCNT_ITEMS;
    if (d1 > V + E) d1 = V + E;
    const int64_t v0 = split[blockIdx.x], v1 = split[blockIdx.x + 1], e0 = d0 - v0, e1 = d1 - v1;
    const int nv = (int) (v1 - v0) + 1;   // rows touched: v0 .. v1 (the last one may be partial, or == V)
    for (int i = tid; i < nv; i += BFS_THREADS) {
        const int64_t vi = v0 + i;
        s_off[i] = vi <= V ? begin[vi < V ? vi : V] : (int32_t) E;
        // (the row's own bit, asked once per row, rides in the counter's sign: -1 = this row counts nothing)
        s_cnt[i] = row_bm && vi < V && !((row_bm[vi >> 5] >> (vi & 31)) & 1u) ? -1 : 0;
    }
    if (tid == 0) s_off[nv] = INT_MAX;   // sentinel
    __syncthreads();
    if (e1 > e0) {   // (workgroup-uniform)
        constexpr int K = ROWCNT_ITEMS / BFS_THREADS;
        const int lane = tid & 63;
        int32_t w[K], row[K];
        bool on[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int64_t x = e0 + tid + (int64_t) k * BFS_THREADS;
            on[k] = x < e1;
            const int64_t xc = on[k] ? x : e0;
            row[k] = frontier_slot(s_off, nv, xc);
            on[k] = on[k] && s_cnt[row[k]] >= 0;   // (nobody adds to a row that counts nothing, so the sign stays)
        }
#pragma unroll
        for (int k = 0; k < K; k++) w[k] = on[k] ? idx[e0 + tid + (int64_t) k * BFS_THREADS] : 0;   // (unasked rows' slots are not read)
        uint32_t pw[K];
#pragma unroll
        for (int k = 0; k < K; k++) pw[k] = probe_bm[w[k] >> 5];
#pragma unroll
        for (int k = 0; k < K; k++) {
            // consecutive lanes hold consecutive slots: the lanes of one row are a run, and the run's first lane adds the
            // run's count -- one LDS add per (row, wave, pass) instead of one per slot on the same word
            const bool bit = on[k] && ((((pw[k] >> (w[k] & 31)) & 1u) != 0) != (invert != 0));
            const unsigned long long m = __ballot(bit);
            const int prev = __shfl_up(row[k], 1, 64);
            const unsigned long long heads = __ballot(lane == 0 || prev != row[k]);
            if (m && ((heads >> lane) & 1ull)) {
                const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
                const int len = after ? __builtin_ctzll(after) + 1 : 64 - lane;   // lanes of this run
                const unsigned long long mask = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << lane;
                const int c = __popcll(m & mask);
                if (c) atomicAdd(&s_cnt[row[k]], c);
            }
        }
    }
    __syncthreads();
    unsigned long long acc = 0;
    for (int i = tid; i < nv; i += BFS_THREADS) {
        const int32_t c = s_cnt[i];
        if (c <= 0) continue;
        acc += (unsigned long long) c;
        if (cnt) {
            const int64_t r = v0 + i;
            // a row whose slots all lie in this workgroup's range is written; the (at most two) rows cut by the range add
            const bool whole = (int64_t) s_off[i] >= e0 && i + 1 < nv && (int64_t) s_off[i + 1] <= e1;
            if (whole) cnt[r] = c; else atomicAdd(&cnt[r], c);
        }
    }
    if (total) {   // one add per workgroup, on one of 64 words (131 K workgroups adding to ONE word: ~90 adds per us, 3.7 ms)
        __shared__ unsigned long long s_red[BFS_THREADS / 64];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if ((tid & 63) == 0) s_red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            unsigned long long t = 0;
            for (int i = 0; i < BFS_THREADS / 64; i++) t += s_red[i];
            if (t) atomicAdd(&total[blockIdx.x & 63], t);
        }
    }
}
__global__ void sum_shards_kernel(const unsigned long long* __restrict__ shard, unsigned long long* __restrict__ total) {
    unsigned long long t = shard[threadIdx.x];   // 64 threads
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o, 64);
    if (threadIdx.x == 0 && t) atomicAdd(total, t);
}

// rows (all, or those whose bit is set in row_bm) count their neighbours by the probe bitmap; cnt (if given) is zeroed by the caller
static int count_by_bitmap(const int32_t* begin, const int32_t* idx, int64_t V, int64_t E, const unsigned long long* row_bm,
                           const unsigned long long* probe_bm, int invert, int32_t* cnt, unsigned long long* total) {
    if (getenv("GMX_ROWCNT_PER_ROW")) {   // development option: the one-row-per-lane form
        dbuf<int32_t> long_rows;
        dbuf<unsigned long long> nlong;
        GMX_CHECK(long_rows.alloc((size_t) V));
        GMX_CHECK(nlong.alloc(1));
        GMX_HIP(hipMemsetAsync(nlong.p, 0, sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(row_count_kernel, dim3(grid_for(V, BFS_THREADS, 256 * 32)), dim3(BFS_THREADS), 0, 0, begin, idx, V,
                           (const uint32_t*) row_bm, (const uint32_t*) probe_bm, invert, cnt, long_rows.p, nlong.p, total);
        unsigned long long h = 0;
        GMX_HIP(hipMemcpy(&h, nlong.p, sizeof(h), hipMemcpyDeviceToHost));
        if (h) {
            int64_t wb = (int64_t) ((h * 64 + BFS_THREADS - 1) / BFS_THREADS);
            if (wb > 256 * 32) wb = 256 * 32;
            hipLaunchKernelGGL(row_count_long_kernel, dim3((unsigned) wb), dim3(BFS_THREADS), 0, 0, begin, idx, (const int32_t*) long_rows.p, h,
                               (const uint32_t*) probe_bm, invert, cnt, total);
        }
        GMX_HIP(hipGetLastError());
        return GMX_OK;
    }
    const int64_t nb = (V + E + ROWCNT_ITEMS - 1) / ROWCNT_ITEMS;
    if (nb > 0) {
        dbuf<int64_t> split;
        dbuf<unsigned long long> shard;
        GMX_CHECK(split.alloc((size_t) nb + 1));
        GMX_CHECK(shard.alloc(64));
        GMX_HIP(hipMemsetAsync(shard.p, 0, 64 * sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(row_count_split_kernel, dim3((unsigned) ((nb + 1 + BFS_THREADS - 1) / BFS_THREADS)), dim3(BFS_THREADS), 0, 0, begin, V, E, nb, split.p);
        hipLaunchKernelGGL(row_count_flat_kernel, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, begin, idx, V, E, (const int64_t*) split.p,
                           (const uint32_t*) row_bm, (const uint32_t*) probe_bm, invert, cnt, total ? shard.p : nullptr);
        if (total) hipLaunchKernelGGL(sum_shards_kernel, dim3(1), dim3(64), 0, 0, (const unsigned long long*) shard.p, total);
        GMX_HIP(hipDeviceSynchronize());   // (split and shard are released here)
    }
    GMX_HIP(hipGetLastError());
    return GMX_OK;
}

extern "C" int gmx_avg_teen_cnt(gmx_graph_t* g, const int32_t* age_host, int32_t K, int32_t* teen_cnt_host, float* avg,
                                gmx_stats_t* stats) {
    GMX_REQUIRE(g && avg && (teen_cnt_host || g->V == 0) && (age_host || g->V == 0), "NULL argument");
    if (stats) memset(stats, 0, sizeof(*stats));
    *avg = 0;
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    dbuf<int32_t> age, cnt;
    dbuf<unsigned long long> acc;
    GMX_CHECK(age.alloc((size_t) V));
    GMX_CHECK(cnt.alloc((size_t) V));
    GMX_CHECK(acc.alloc(2));
    gmx_spans tm;
    GMX_HIP(hipMemcpy(age.p, age_host, sizeof(int32_t) * (size_t) V, hipMemcpyHostToDevice));
    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(acc.p, 0, 2 * sizeof(unsigned long long), 0));
    // n.teen_cnt = Count(t: n.InNbrs)(t.age >= 10 && t.age < 20)
    if (g->has_reverse) {   // as written: every row walks its in-neighbours, the filter being a bitmap in the L2
        dbuf<unsigned long long> teen;
        GMX_CHECK(teen.alloc((size_t) ((V + 63) / 64)));
        hipLaunchKernelGGL(pred_bitmap_kernel, dim3(grid_for(V, BFS_THREADS, 256 * 16)), dim3(BFS_THREADS), 0, 0, (const int32_t*) age.p, V, 0, 0, teen.p);
        GMX_CHECK(count_by_bitmap(g->r_begin.p, g->r_node_idx.p, V, g->E, nullptr, teen.p, 0, cnt.p, nullptr));
        GMX_HIP(hipDeviceSynchronize());   // (teen is released at the end of this block)
    } else {                // forward CSR only: one increment per out-edge of a teen (integer atomics: same counts)
        GMX_CHECK(expand_selected(g, age.p, 0, 0, cnt.p));
    }
    // Avg(n: G.Nodes)(n.age > K){n.teen_cnt}: int32 sum, int64 count (gm_syntax_sugar2.cc:264-296)
    hipLaunchKernelGGL(filtered_sum_kernel, dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, (const int32_t*) age.p, (const int32_t*) cnt.p,
                       (const int32_t*) nullptr, V, 0, K, acc.p);
    GMX_CHECK(tm.end(tm.KERNEL));
    unsigned long long h[2];
    GMX_HIP(hipMemcpy(h, acc.p, sizeof(h), hipMemcpyDeviceToHost));
    GMX_HIP(hipMemcpy(teen_cnt_host, cnt.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    const int32_t S = (int32_t) (uint32_t) h[0];          // the emitted sum is an int32 and wraps like one
    const int64_t n = (int64_t) h[1];
    const double a = (0 == n) ? ((float) (0.000000)) : (S / ((double) n));
    *avg = (float) a;
    if (stats) stats->iterations = 1;
    return tm.finish(stats);
}

extern "C" int gmx_conduct(gmx_graph_t* g, const int32_t* member_host, int32_t num, float* result, gmx_stats_t* stats) {
    GMX_REQUIRE(g && result && (member_host || g->V == 0), "NULL argument");
    if (stats) memset(stats, 0, sizeof(*stats));
    *result = 0;
    const int64_t V = g->V;
    unsigned long long h[6] = {0, 0, 0, 0, 0, 0};
    gmx_spans tm;
    if (V > 0) {
        dbuf<int32_t> member;
        dbuf<unsigned long long> acc;   // [0,1] Din + count, [2,3] Dout + count, [4] Cross
        GMX_CHECK(member.alloc((size_t) V));
        GMX_CHECK(acc.alloc(6));
        GMX_HIP(hipMemcpy(member.p, member_host, sizeof(int32_t) * (size_t) V, hipMemcpyHostToDevice));
        GMX_CHECK(tm.begin(tm.KERNEL));
        GMX_HIP(hipMemsetAsync(acc.p, 0, 6 * sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(filtered_sum_kernel, dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, (const int32_t*) member.p, (const int32_t*) nullptr,
                           (const int32_t*) g->begin.p, V, 1, num, acc.p);
        hipLaunchKernelGGL(filtered_sum_kernel, dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, (const int32_t*) member.p, (const int32_t*) nullptr,
                           (const int32_t*) g->begin.p, V, 2, num, acc.p + 2);
        {   // Cross: members count their out-neighbours that are not members (membership as a bitmap in the L2)
            dbuf<unsigned long long> mem_bm;
            GMX_CHECK(mem_bm.alloc((size_t) ((V + 63) / 64)));
            hipLaunchKernelGGL(pred_bitmap_kernel, dim3(grid_for(V, BFS_THREADS, 256 * 16)), dim3(BFS_THREADS), 0, 0, (const int32_t*) member.p, V, 1, num, mem_bm.p);
            GMX_CHECK(count_by_bitmap(g->begin.p, g->node_idx.p, V, g->E, mem_bm.p, mem_bm.p, 1, nullptr, acc.p + 4));
            GMX_HIP(hipDeviceSynchronize());
        }
        GMX_CHECK(tm.end(tm.KERNEL));
        GMX_HIP(hipMemcpy(h, acc.p, sizeof(h), hipMemcpyDeviceToHost));
    }
    const int32_t Din = (int32_t) (uint32_t) h[0], Dout = (int32_t) (uint32_t) h[2], Cross = (int32_t) (uint32_t) h[4];
    const float m = (float) ((Din < Dout) ? Din : Dout);
    if (m == 0) *result = (Cross == 0) ? ((float) (0.000000)) : FLT_MAX;
    else *result = Cross / m;
    if (stats && V > 0) stats->iterations = 1;
    return tm.finish(stats);
}

// (see gmx_touch_bfs)
void gmx_touch_nbrcount() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) pred_bitmap_kernel);
}
