// gmx_sssp.hip -- sssp and sssp_path (shortest paths over out-edges with an integer edge property) for gfx950.
#include "gmx_frontier.h"

#include <limits.h>
#include <string.h>
#include <rocprim/rocprim.hpp>

// ------------------------------------------------------------------ sssp
// The emitted `sssp` (/root/reference/apps/src/sssp.gm:1-30) is hop_dist's loop with an edge property:
//     <s.dist_nxt; s.updated_nxt> min= <n.dist + e.len; True>     e = the out-edge slot being walked
// until nothing changes.  dist[v] is the length of a shortest path over out-edges (INT_MAX: unreachable) --
// unique, so the device is free to relax asynchronously: the updated vertices form a queue, their out-edges
// are cut by merge-path exactly as in the top-down BFS level, every edge does atomicMin(dist[s], dist[n] +
// len[e]) in place, and a vertex whose distance dropped enters the next queue once per round (round stamp).
// Integer only: bit-exact against the CPU result.
__global__ void __launch_bounds__(BFS_THREADS)
sssp_relax_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ node_idx, const int32_t* __restrict__ len,
                  const int32_t* __restrict__ cur_q, int64_t n, const int64_t* __restrict__ off, int64_t m,
                  int32_t round, int32_t* __restrict__ dist, int32_t* __restrict__ stamp, int32_t* __restrict__ next_q,
                  bfs_counters* __restrict__ ctr, const int64_t* __restrict__ split) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_dist[BFS_ITEMS + 2];
    __shared__ int32_t s_win[BFS_ITEMS];   // (one queue-tail claim per workgroup, as in bfs_topdown_kernel)
    __shared__ unsigned int s_nwin;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_nwin = 0;
    const frontier_tile t = frontier_tile_split(split, n, m);
    const int nv = frontier_stage(t, begin, cur_q, n, off, m, s_off, s_row, [&](int i, int32_t v, bool in) {
        s_dist[i] = in ? dist[v] : 0;      // may already be lower than when v was queued: even better
    });
    unsigned long long inspected = 0;
    for (int64_t x = t.e0 + tid; x < t.e1; x += BFS_THREADS) {
        const int lo = frontier_slot(s_off, nv, x);
        const int64_t e = (int64_t) s_row[lo] + (x - s_off[lo]);
        const int32_t s = node_idx[e];
        const int32_t nd = s_dist[lo] + len[e];
        inspected++;
        bool won = false;
        if (nd < dist[s] && nd < atomicMin(&dist[s], nd)) won = atomicExch(&stamp[s], round) != round;
        wave_append(won, s, s_win, &s_nwin, tid & 63);
    }
    inspected = wave_sum(inspected);
    if ((tid & 63) == 0) bfs_count(ctr, inspected, 0);
    __syncthreads();
    const unsigned int nwin = s_nwin;
    if (nwin == 0) return;   // (workgroup-uniform)
    frontier_flush(s_win, nwin, &ctr->next_count, next_q, &s_base);
}

__global__ void sssp_init_kernel(int32_t* __restrict__ dist, int32_t* __restrict__ stamp, int64_t V, int32_t root) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < V; i += stride) {
        dist[i] = (i == root) ? 0 : INT_MAX;
        stamp[i] = -1;
    }
}

// What the two relaxation entries share: the round queues and their stamp, the queue's merge-path offsets, the counters with
// their pinned read-backs, and the edge property on the device.
struct relax_scratch {
    dbuf<int32_t> stamp, q0, q1, len, len_sorted;
    frontier_scan fs;
    dbuf<bfs_counters> ctr;
    gmx_pinned<bfs_counters> h_ctr;   // per-round read-backs through pinned memory (two host round trips per round, dozens of rounds)
    gmx_pinned<int64_t> h_mf;
    const int32_t* len_dev = nullptr;   // the property in the order of the device's slots
    int alloc(const gmx_graph* g) {
        const size_t V = (size_t) g->V;
        GMX_CHECK(stamp.alloc(V));
        GMX_CHECK(q0.alloc(V));
        GMX_CHECK(q1.alloc(V));
        GMX_CHECK(gmx_frontier_scan_alloc(&fs, V, (size_t) ((g->V + g->E) / BFS_ITEMS + 3)));   // one split entry per merge-path diagonal of a round
        GMX_CHECK(ctr.alloc(1));
        GMX_CHECK(len.alloc((size_t) (g->E ? g->E : 1)));
        GMX_CHECK(h_ctr.alloc());
        return h_mf.alloc();
    }
    int upload_len(const gmx_graph* g, const int32_t* len_host) {   // the property is the caller's
        if (g->E) GMX_HIP(hipMemcpy(len.p, len_host, sizeof(int32_t) * (size_t) g->E, hipMemcpyHostToDevice));
        len_dev = len.p;
        return GMX_OK;
    }
    // the rows were sorted on upload: len[] is indexed by the caller's (unsorted) slots, the kernels walk the sorted ones
    int reorder_len(const gmx_graph* g) {
        if (!g->E || !g->e_idx2idx.p) return GMX_OK;
        GMX_CHECK(len_sorted.alloc((size_t) g->E));
        hipLaunchKernelGGL(gather_by_order_kernel<int32_t>, dim3(grid_for(g->E)), dim3(BFS_THREADS), 0, 0, (const int32_t*) len.p,
                           (const int32_t*) g->e_idx2idx.p, g->E, len_sorted.p);
        len_dev = len_sorted.p;
        return GMX_OK;
    }
    // the offsets and tile boundaries of q[0..n): returns the queue's edges
    int offsets(const gmx_graph* g, const int32_t* q, int64_t n, int64_t* m_f) {
        GMX_CHECK(gmx_frontier_offsets(g->begin.p, q, n, &fs, h_mf.p, true));
        *m_f = *h_mf.p;
        return GMX_OK;
    }
};

extern "C" int gmx_sssp(gmx_graph_t* g, gmx_node_t root, const int32_t* len_host, int32_t* dist_host, gmx_stats_t* stats) {
    GMX_REQUIRE(g && dist_host, "NULL argument");
    GMX_REQUIRE(len_host || g->E == 0, "len is NULL");
    if (stats) memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    const bool root_ok = root >= 0 && root < V;
    dbuf<int32_t> dist;
    relax_scratch S;
    GMX_CHECK(dist.alloc((size_t) V));
    GMX_CHECK(S.alloc(g));
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.H2D));
    GMX_CHECK(S.upload_len(g, len_host));
    GMX_CHECK(S.reorder_len(g));
    GMX_CHECK(tm.end(tm.H2D));
    GMX_CHECK(tm.begin(tm.KERNEL));
    hipLaunchKernelGGL(sssp_init_kernel, dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, dist.p, S.stamp.p, V, root_ok ? root : -1);
    int64_t cur_count = 0, requeued = 0;
    unsigned long long edges = 0;
    int32_t round = 0;
    int32_t* cur_q = S.q0.p;
    int32_t* next_q = S.q1.p;
    if (root_ok) {
        GMX_HIP(hipMemcpy(S.q0.p, &root, sizeof(int32_t), hipMemcpyHostToDevice));
        cur_count = 1;
    }
    bfs_counters* ctr = S.ctr.p;
    GMX_HIP(hipMemsetAsync(ctr, 0, sizeof(bfs_counters), 0));
    while (cur_count > 0) {
        GMX_HIP(hipMemsetAsync(&ctr->next_count, 0, sizeof(unsigned long long), 0));   // `edges` keeps accumulating
        int64_t m_f = 0;
        GMX_CHECK(S.offsets(g, cur_q, cur_count, &m_f));
        const int64_t nb = frontier_tiles(cur_count, m_f);
        if (nb > 0)
            hipLaunchKernelGGL(sssp_relax_kernel, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, g->begin.p, g->node_idx.p,
                               S.len_dev, cur_q, cur_count, S.fs.off.p, m_f, round, dist.p, S.stamp.p, next_q, ctr, (const int64_t*) S.fs.split.p);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(S.h_ctr, S.ctr.p));
        const bfs_counters& h = *S.h_ctr.p;
        unsigned long long found_unused = 0;
        cur_count = (int64_t) h.next_count;
        bfs_totals(h, &edges, &found_unused);
        requeued += cur_count;
        int32_t* t = cur_q;
        cur_q = next_q;
        next_q = t;
        round++;
    }
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.finish(stats));
    GMX_HIP(hipMemcpy(dist_host, dist.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    if (stats) {
        stats->iterations = round;
        stats->edges_examined = (int64_t) edges;
        stats->vertices_reached = requeued + (root_ok ? 1 : 0);   // queue entries over all rounds (a vertex may re-enter)
    }
    return GMX_OK;
}

// ------------------------------------------------------------------ sssp_path: the shortest-path tree next to the lengths
// The emitted `sssp_path` (/root/reference/apps/src/sssp_path.gm:1-30) is sssp's loop whose min= also records the winner:
//     <s.dist_nxt; s.updated_nxt, s.prev> min= <n.dist + e.len; True, n>
// Which of several equally short predecessors it records depends on the reference's thread timing.  The device returns a
// fixed member of that set: distance and predecessor slot of a vertex are ONE 64-bit word,
//     key[v] = (dist << 32) | device slot of the in-edge        (root: (0, NIL); unreached: (INT_MAX, NIL))
// and relaxing slot e = n -> s offers (dist[n] + len[e], e) with one 64-bit unsigned atomicMin.  Ties in the distance are
// offered too, so among the candidates at the final distance -- exactly the tight in-edges, each offered after its
// source's last drop (a candidate that equals the final distance of s cannot come from a source above its own final
// distance) -- the smallest slot wins whatever the order.  A zero-length edge may only win when it lowers the distance
// strictly (compare-and-swap): the vertices of a zero-length cycle then take their predecessors in the order in which
// they reached the distance, which has no cycle.  Lengths must be >= 0 (the word orders distances as unsigned).
// The schedule has to keep one invariant: every vertex relaxes all its out-edges at least once after its last drop,
// reading its current distance.  Two schedules do:
//   round queue   gmx_sssp's: a vertex whose distance dropped in round r is relaxed in round r + 1;
//   near / far    a drop below the threshold T goes to the next round's queue, the others to a far pile; when the queue
//                 runs dry T advances by delta (further, when nothing lies below it) and the pile is filtered: entries
//                 whose vertex is below the old T are stale (it was queued when it got there, and relaxed since), the
//                 others go to the queue (below the new T) or stay, each vertex once.
// stamp[v] = 2 * tag + (queued: 1, piled: 0) of the last time v entered either, tags rising from launch to launch.
#define SP_NIL 0xFFFFFFFFu
#define SP_WORD(d, e) (((unsigned long long) (uint32_t) (d) << 32) | (unsigned long long) (uint32_t) (e))
// slots of bfs_counters::pad0 the far pile uses (same cache line as next_count: one claim per workgroup)
#define SP_FAR_TAIL 0   // entries in the pile being written
#define SP_FAR_NEAREST 1   // filter: max over the kept entries of (2^32 - distance); 0 = none kept
#define SP_FAR_SPILL 2   // an entry did not fit (never, by the host's accounting): the call fails instead of writing

__global__ void sp_init_kernel(unsigned long long* __restrict__ key, int32_t* __restrict__ stamp, int64_t V, int32_t root) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < V; i += stride) {
        key[i] = SP_WORD(i == root ? 0 : INT_MAX, SP_NIL);
        stamp[i] = -1;
    }
}

// out[0] = number of negative lengths, out[1] = sum of the lengths (one atomic per workgroup and value)
__global__ void __launch_bounds__(BFS_THREADS)
sp_len_check_kernel(const int32_t* __restrict__ len, int64_t E, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_neg[BFS_THREADS / 64], s_sum[BFS_THREADS / 64];
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long neg = 0, sum = 0;
    for (; i < E; i += stride) {
        const int32_t l = len[i];
        neg += l < 0;
        sum += l < 0 ? 0ull : (unsigned long long) l;
    }
    neg = wave_sum(neg);
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) {
        s_neg[threadIdx.x >> 6] = neg;
        s_sum[threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        neg = sum = 0;
        for (int w = 0; w < BFS_THREADS / 64; w++) {
            neg += s_neg[w];
            sum += s_sum[w];
        }
        if (neg) atomicAdd(&out[0], neg);
        if (sum) atomicAdd(&out[1], sum);
    }
}

// sssp_relax_kernel's shape with the packed word.  NEARFAR: drops to threshold or above go to the far pile.
template <bool NEARFAR>
__global__ void __launch_bounds__(BFS_THREADS)
sp_relax_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ node_idx, const int32_t* __restrict__ len,
                const int32_t* __restrict__ cur_q, int64_t n, const int64_t* __restrict__ off, int64_t m, int32_t tag,
                unsigned long long* key, int32_t* __restrict__ stamp, int32_t* __restrict__ next_q, int32_t* __restrict__ far_q,
                unsigned long long far_cap, uint32_t threshold, bfs_counters* __restrict__ ctr, const int64_t* __restrict__ split) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ uint32_t s_dist[BFS_ITEMS + 2];
    __shared__ int32_t s_win[BFS_ITEMS];   // (one queue-tail claim per workgroup, as in sssp_relax_kernel)
    __shared__ int32_t s_far[NEARFAR ? BFS_ITEMS : 1];
    __shared__ unsigned int s_nwin, s_nfar;
    __shared__ unsigned long long s_base, s_fbase;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_nwin = s_nfar = 0;
    const frontier_tile t = frontier_tile_split(split, n, m);
    const int nv = frontier_stage(t, begin, cur_q, n, off, m, s_off, s_row, [&](int i, int32_t v, bool in) {
        s_dist[i] = in ? (uint32_t) (key[v] >> 32) : 0u;   // the current distance (a later drop queues v again)
    });
    unsigned long long inspected = 0;
    for (int64_t x = t.e0 + tid; x < t.e1; x += BFS_THREADS) {
        const int lo = frontier_slot(s_off, nv, x);
        const int64_t e = (int64_t) s_row[lo] + (x - s_off[lo]);
        const int32_t s = node_idx[e];
        const int32_t l = len[e];
        const uint32_t nd = s_dist[lo] + (uint32_t) l;
        const unsigned long long cand = SP_WORD(nd, e);
        inspected++;
        // <s.dist_nxt; s.updated_nxt, s.prev> min= <n.dist + e.len; True, n>   (sssp_path.gm:21)
        unsigned long long cur = key[s];   // (a stale copy is only higher: the atomic decides)
        bool dropped = false;
        if (l > 0) {
            if (cand < cur) dropped = (uint32_t) (atomicMin(&key[s], cand) >> 32) > nd;   // equal distance: a smaller slot, no new work
        } else {
            while ((uint32_t) (cur >> 32) > nd) {   // zero length: only a strictly lower distance
                const unsigned long long seen = atomicCAS(&key[s], cur, cand);
                if (seen == cur) {
                    dropped = true;
                    break;
                }
                cur = seen;
            }
        }
        bool to_queue = false, to_pile = false;
        if (dropped) {
            const bool near = !NEARFAR || nd < threshold;
            const int32_t mark = 2 * tag + (near ? 1 : 0);
            const bool first = atomicMax(&stamp[s], mark) < mark;   // (piled and then queued in one launch: both)
            to_queue = first && near;
            to_pile = first && !near;
        }
        wave_append(to_queue, s, s_win, &s_nwin, lane);
        if (NEARFAR) wave_append(to_pile, s, s_far, &s_nfar, lane);
    }
    inspected = wave_sum(inspected);
    if (lane == 0) bfs_count(ctr, inspected, 0);
    __syncthreads();
    const unsigned int nwin = s_nwin, nfar = NEARFAR ? s_nfar : 0u;
    if (nwin == 0 && nfar == 0) return;   // (workgroup-uniform)
    frontier_flush(s_win, nwin, &ctr->next_count, next_q, &s_base, [&] {   // (both tails are claimed before the one barrier)
        if (nfar) s_fbase = atomicAdd(&ctr->pad0[SP_FAR_TAIL], (unsigned long long) nfar);
    });
    if (NEARFAR && nfar) {
        if (s_fbase + nfar <= far_cap) {
            for (unsigned int i = tid; i < nfar; i += BFS_THREADS) far_q[s_fbase + i] = s_far[i];
        } else if (tid == 0) {
            ctr->pad0[SP_FAR_SPILL] = 1ull;
        }
    }
}

// The far pile when the threshold moves from t_old to t_new (or, with t_new == t_old, when the pile is only to be made
// smaller): see the schedule above.  near_q takes at most one entry per vertex, far_out at most min(n, V).
__global__ void __launch_bounds__(BFS_THREADS)
sp_refilter_kernel(const int32_t* __restrict__ far_in, int64_t n, const unsigned long long* __restrict__ key, int32_t* __restrict__ stamp,
                   int32_t tag, uint32_t t_old, uint32_t t_new, int32_t* __restrict__ near_q, int32_t* __restrict__ far_out,
                   bfs_counters* __restrict__ ctr) {
    __shared__ int32_t s_win[BFS_ITEMS];
    __shared__ int32_t s_far[BFS_ITEMS];
    __shared__ unsigned int s_nwin, s_nfar;
    __shared__ unsigned long long s_base, s_fbase, s_nearest;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_nwin = s_nfar = 0;
        s_nearest = 0;
    }
    __syncthreads();
    unsigned long long nearest = 0;
    const int64_t i0 = (int64_t) blockIdx.x * BFS_ITEMS;
    for (int k = 0; k < BFS_ITEMS / BFS_THREADS; k++) {   // (every lane runs every step: whole waves at the ballots)
        const int64_t i = i0 + tid + (int64_t) k * BFS_THREADS;
        bool to_queue = false, to_pile = false;
        int32_t v = 0;
        if (i < n) {
            v = far_in[i];
            const uint32_t d = (uint32_t) (key[v] >> 32);
            if (d >= t_old) {
                const bool near = d < t_new;
                const int32_t mark = 2 * tag + (near ? 1 : 0);
                const bool first = atomicMax(&stamp[v], mark) < mark;
                to_queue = first && near;
                to_pile = first && !near;
                if (to_pile) {
                    const unsigned long long inv = 0x100000000ull - (unsigned long long) d;
                    nearest = inv > nearest ? inv : nearest;
                }
            }
        }
        wave_append(to_queue, v, s_win, &s_nwin, lane);
        wave_append(to_pile, v, s_far, &s_nfar, lane);
    }
    nearest = wave_max(nearest);
    if (lane == 0 && nearest) atomicMax(&s_nearest, nearest);
    __syncthreads();
    const unsigned int nwin = s_nwin, nfar = s_nfar;
    if (nwin == 0 && nfar == 0) return;   // (workgroup-uniform)
    frontier_flush(s_win, nwin, &ctr->next_count, near_q, &s_base, [&] {   // (both tails are claimed before the one barrier)
        if (nfar) {
            s_fbase = atomicAdd(&ctr->pad0[SP_FAR_TAIL], (unsigned long long) nfar);
            atomicMax(&ctr->pad0[SP_FAR_NEAREST], s_nearest);
        }
    });
    for (unsigned int i = tid; i < nfar; i += BFS_THREADS) far_out[s_fbase + i] = s_far[i];
}

// one thread per vertex splits the word: dist, the predecessor slot as an UPLOADED slot, and the row that holds it
__global__ void sp_finish_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ begin,
                                 const int32_t* __restrict__ e_idx2idx /* NULL: the device slots are the uploaded ones */, int64_t V,
                                 int32_t* __restrict__ dist, int32_t* __restrict__ prev_node, int32_t* __restrict__ prev_edge) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; v < V; v += stride) {
        const unsigned long long k = key[v];
        const uint32_t e = (uint32_t) k;
        dist[v] = (int32_t) (k >> 32);
        int32_t pn = -1, pe = -1;
        if (e != SP_NIL) {
            pn = csr_row_of(begin, V, e);
            pe = e_idx2idx ? e_idx2idx[e] : (int32_t) e;
        }
        prev_node[v] = pn;
        prev_edge[v] = pe;
    }
}

// GMX_SSSP_PATH_SCHEDULE = round | nearfar (read at every call); GMX_SSSP_DELTA = the near / far threshold step
static bool sp_use_nearfar() {
    const char* s = getenv("GMX_SSSP_PATH_SCHEDULE");
    if (s && !strcmp(s, "nearfar")) return true;
    if (s && !strcmp(s, "round")) return false;
    return false;
}

extern "C" int gmx_sssp_path(gmx_graph_t* g, gmx_node_t root, const int32_t* len_host, int32_t* dist_host, gmx_node_t* prev_node_host,
                             gmx_edge_t* prev_edge_host, gmx_stats_t* stats) {
    GMX_REQUIRE(g && dist_host && prev_node_host, "NULL argument");
    GMX_REQUIRE(len_host || g->E == 0, "len is NULL");
    if (stats) memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    const bool root_ok = root >= 0 && root < V;
    const bool nearfar = sp_use_nearfar();
    const size_t far_cap = nearfar ? 2 * (size_t) V : 0;   // a launch adds at most V entries to a pile of at most V
    dbuf<unsigned long long> key, chk;
    dbuf<int32_t> far0, far1, out;
    relax_scratch S;
    GMX_CHECK(key.alloc((size_t) V));
    GMX_CHECK(chk.alloc(2));
    GMX_CHECK(S.alloc(g));
    GMX_CHECK(out.alloc(3 * (size_t) V));
    if (nearfar) {
        GMX_CHECK(far0.alloc(far_cap));
        GMX_CHECK(far1.alloc(far_cap));
    }
    gmx_spans tm;
    // the property: copied in, checked on the device copy (negative lengths are refused), brought into the order of the
    // sorted rows when the upload sorted them
    GMX_CHECK(tm.begin(tm.H2D));
    unsigned long long h_chk[2] = {0, 0};
    GMX_CHECK(S.upload_len(g, len_host));
    if (E) {
        GMX_HIP(hipMemsetAsync(chk.p, 0, 2 * sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(sp_len_check_kernel, dim3(grid_for(E)), dim3(BFS_THREADS), 0, 0, (const int32_t*) S.len.p, E, chk.p);
        GMX_HIP(hipGetLastError());
        GMX_HIP(hipMemcpy(h_chk, chk.p, sizeof(h_chk), hipMemcpyDeviceToHost));
        GMX_REQUIRE(h_chk[0] == 0, "len holds %llu negative value(s): gmx_sssp_path needs len >= 0", h_chk[0]);
    }
    GMX_CHECK(S.reorder_len(g));
    GMX_CHECK(tm.end(tm.H2D));
    // near / far: delta = 32 * mean length / mean out-degree (a queue round then holds about a wave's worth of edges per
    // vertex of the band), at least 1
    uint32_t delta = 1;
    if (nearfar) {
        double dl = E ? 32.0 * ((double) h_chk[1] / (double) E) / ((double) E / (double) V) : 1.0;
        const char* s = getenv("GMX_SSSP_DELTA");
        if (s && atof(s) >= 1.0) dl = atof(s);
        delta = dl < 1.0 ? 1u : dl > 1073741824.0 ? (1u << 30) : (uint32_t) dl;
    }
    const uint32_t T_ALL = 0x80000000u;   // above every distance
    uint32_t T = nearfar ? delta : T_ALL;
    GMX_CHECK(tm.begin(tm.KERNEL));
    hipLaunchKernelGGL(sp_init_kernel, dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, key.p, S.stamp.p, V, root_ok ? root : -1);
    int64_t cur_count = 0, queued = 0, far_n = 0;
    unsigned long long edges = 0;
    int32_t rounds = 0, tag = 0;
    int32_t* cur_q = S.q0.p;
    int32_t* next_q = S.q1.p;
    int32_t* far_cur = far0.p;
    int32_t* far_alt = far1.p;
    if (root_ok) {
        GMX_HIP(hipMemcpy(S.q0.p, &root, sizeof(int32_t), hipMemcpyHostToDevice));
        cur_count = queued = 1;
    }
    bfs_counters* ctr = S.ctr.p;
    const bfs_counters* h_ctr = S.h_ctr.p;
    GMX_HIP(hipMemsetAsync(ctr, 0, sizeof(bfs_counters), 0));
    // filter the pile far_cur[0 .. far_n) into cur_q (which is empty, or untouched when t_new == t_old) and far_alt
    auto refilter = [&](uint32_t t_old, uint32_t t_new, int64_t* near_n, uint32_t* nearest) -> int {
        GMX_HIP(hipMemsetAsync(&ctr->next_count, 0, (2 + SP_FAR_NEAREST + 1) * sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(sp_refilter_kernel, dim3((unsigned) ((far_n + BFS_ITEMS - 1) / BFS_ITEMS)), dim3(BFS_THREADS), 0, 0,
                           (const int32_t*) far_cur, far_n, (const unsigned long long*) key.p, S.stamp.p, tag, t_old, t_new, cur_q, far_alt, ctr);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(S.h_ctr, S.ctr.p));
        tag++;
        *near_n = (int64_t) h_ctr->next_count;
        far_n = (int64_t) h_ctr->pad0[SP_FAR_TAIL];
        *nearest = h_ctr->pad0[SP_FAR_NEAREST] ? (uint32_t) (0x100000000ull - h_ctr->pad0[SP_FAR_NEAREST]) : 0u;
        int32_t* t = far_cur;
        far_cur = far_alt;
        far_alt = t;
        return GMX_OK;
    };
    for (;;) {
        while (cur_count > 0) {
            if (nearfar && far_n > V) {   // room for this round's (at most V) new entries: drop the stale ones and the repeats
                int64_t none = 0;
                uint32_t unused = 0;
                GMX_CHECK(refilter(T, T, &none, &unused));
                GMX_REQUIRE(none == 0 && far_n <= V, "gmx_sssp_path: far pile accounting");
            }
            GMX_HIP(hipMemsetAsync(&ctr->next_count, 0, sizeof(unsigned long long), 0));   // (`edges` and the pile's tail run on)
            int64_t m_f = 0;
            GMX_CHECK(S.offsets(g, cur_q, cur_count, &m_f));
            const int64_t nb = frontier_tiles(cur_count, m_f);
            if (nb > 0) {
                if (nearfar)
                    hipLaunchKernelGGL(sp_relax_kernel<true>, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, g->begin.p, g->node_idx.p, S.len_dev,
                                       cur_q, cur_count, S.fs.off.p, m_f, tag, key.p, S.stamp.p, next_q, far_cur, (unsigned long long) far_cap, T,
                                       ctr, (const int64_t*) S.fs.split.p);
                else
                    hipLaunchKernelGGL(sp_relax_kernel<false>, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, g->begin.p, g->node_idx.p, S.len_dev,
                                       cur_q, cur_count, S.fs.off.p, m_f, tag, key.p, S.stamp.p, next_q, (int32_t*) nullptr, 0ull, T, ctr,
                                       (const int64_t*) S.fs.split.p);
            }
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(S.h_ctr, S.ctr.p));
            const bfs_counters& h = *h_ctr;
            unsigned long long found_unused = 0;
            cur_count = (int64_t) h.next_count;
            far_n = (int64_t) h.pad0[SP_FAR_TAIL];
            GMX_REQUIRE(h.pad0[SP_FAR_SPILL] == 0 && far_n <= (int64_t) far_cap, "gmx_sssp_path: far pile overflow");
            bfs_totals(h, &edges, &found_unused);
            queued += cur_count;
            int32_t* t = cur_q;
            cur_q = next_q;
            next_q = t;
            rounds++;
            tag++;
        }
        if (far_n == 0) break;
        // the queue ran dry: advance the threshold; when nothing lies below the new one, to just above the nearest entry
        uint32_t nearest = 0;
        const uint32_t t_old = T;
        T = T > T_ALL - delta ? T_ALL : T + delta;
        GMX_CHECK(refilter(t_old, T, &cur_count, &nearest));
        if (cur_count == 0 && far_n > 0) {
            const uint64_t up = ((uint64_t) nearest / delta + 1) * (uint64_t) delta;
            const uint32_t t_prev = T;
            T = up > T_ALL ? T_ALL : (uint32_t) up;
            GMX_CHECK(refilter(t_prev, T, &cur_count, &nearest));
            GMX_REQUIRE(cur_count > 0, "gmx_sssp_path: threshold accounting");
        }
        queued += cur_count;
    }
    hipLaunchKernelGGL(sp_finish_kernel, dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, (const unsigned long long*) key.p, (const int32_t*) g->begin.p,
                       (const int32_t*) g->e_idx2idx.p, V, out.p, out.p + V, out.p + 2 * V);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.sync(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(dist_host, out.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_HIP(hipMemcpy(prev_node_host, out.p + V, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    if (prev_edge_host) GMX_HIP(hipMemcpy(prev_edge_host, out.p + 2 * V, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));
    if (stats) {
        stats->iterations = rounds;
        stats->edges_examined = (int64_t) edges;
        stats->vertices_reached = queued;   // queue entries over all rounds (a vertex may re-enter), the root's included
    }
    return GMX_OK;
}

// (see gmx_touch_bfs)
void gmx_touch_sssp() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) sssp_init_kernel);
}
