// gmx_sssp_f64.hip -- sssp_path_adj (a route query root -> end with Double edge costs and a predecessor node and edge per
// vertex) for gfx950.
//
// Replaces the body of apps/src/sssp_path_adj.gm:1-33:
//     G.dist = G.dist_nxt = (G == root) ? 0 : +INF;  G.updated = G.updated_nxt = (G == root);  G.prev_node = G.prev_edge = NIL;
//     While (!fin) {
//         Foreach (n: G.Nodes)(n.updated && n.dist < end.dist) Foreach (s: n.Nbrs) { e = s.ToEdge();
//             If (n.dist + e.edge_cost < end.dist) <s.dist_nxt; s.updated_nxt, s.prev_node, s.prev_edge> min= <n.dist + e.edge_cost; True, n, e>; }
//         G.dist = G.dist_nxt;  G.updated = G.updated_nxt;  G.updated_nxt = False;  fin = !Exist(n: G.Nodes){n.updated}; }
// as ONE thread runs it (+INF is DBL_MAX, gm_cpp_gen.cc:1790).  end.dist is the value at the round's start, so what a
// vertex at or beyond end's distance ends up with depends on the rounds: the rounds are kept, synchronously, and with them
// all three arrays are those of the one-thread run byte for byte (gmx.h, DESIGN.md 4.2b'').  Per round, for every vertex
// whose dist_nxt dropped: the new distance is the minimum of the round's offers, the predecessor the offer of smallest
// uploaded slot among those equal to that minimum; a vertex that did not drop keeps its predecessor.
//   - a distance is a non-negative double (DBL_MAX included): its bit pattern orders as an unsigned 64-bit word, so the
//     minimum is a 64-bit atomicMin, tried only after a load says it would lower the word;
//   - the word is full, so the winner is a second word per vertex, (round << 32) | ~uploaded slot under a 64-bit atomicMax:
//     an older round's word loses by itself, nothing is cleared between rounds, and the offer that replaces an older round's
//     word is the one that puts its vertex on the list of the dropped;
//   - a round is three launches over lists, none over V or E: offer (the rows of the queue, merge-path tiles of
//     gmx_frontier.h), winner (the same tiles again: the minimum is only final behind the launch boundary) and commit (the
//     dropped: dist = dist_nxt, the winner word split into prev_node / prev_edge, and the vertex queued when it is below the
//     next round's bound dist_nxt[end] and has a row).  The bound is read on the device;
//   - once the queued rows hold few slots one workgroup runs rounds in one launch (spf_tail_kernel) until the queue grows
//     past the threshold again.
// The only arithmetic is dist[n] + cost[e] in double (-ffp-contract=off; there is nothing to contract): exact parity.
#include "gmx_frontier.h"

#include <float.h>

#define SPF_THREADS 256          // = BFS_THREADS (frontier_flush copies with that stride)
static_assert(SPF_THREADS == BFS_THREADS, "frontier_flush and first_bad_slot_kernel are built for BFS_THREADS");
#define SPF_CHUNK 2048           // list entries a workgroup of the commit kernel compacts in LDS
#define SPF_TAIL_THREADS 1024
#define SPF_TAIL 4096            // GMX_SSSP_F64_TAIL: the tail launch takes over while the queued rows hold at most this many slots
#define SPF_TAIL_LANE 8          // the tail reads a row of at most this many slots with one lane, a longer one with a wave
#define SPF_MAX_BITS 0x7FEFFFFFFFFFFFFFull   // DBL_MAX

typedef unsigned long long spf_word;

struct spf_counters {
    spf_word ntouch;         // vertices that dropped in the round (tail of `touched`)
    spf_word nnext;          // tail of the next queue
    spf_word mnext;          // its rows' slots
    spf_word tail_rounds;    // what the last tail launch ran: rounds, the slots of their queues, the vertices that dropped
    spf_word tail_slots;
    spf_word tail_touched;
    spf_word bad;            // E - (first slot whose cost is negative or NaN); 0: none
    spf_word pad[9];
};

struct spf_state {
    const int32_t* begin;
    const int32_t* node_idx;
    const double* cost;      // by device slot
    const int32_t* order;    // device slot -> uploaded slot (e_idx2idx), NULL: the same
    spf_word* dist;          // [V] bit patterns
    spf_word* dnxt;          // [V]
    spf_word* win;           // [V] (round << 32) | ~uploaded slot of the round's winning offer
    int32_t* prev_node;
    int32_t* prev_edge;
    int32_t* touched;        // [V] the vertices that dropped in the round, each once
    spf_counters* ctr;
    int64_t V;
    int32_t end;             // -1: no target
};

// dist, dist_nxt and the winner words are read and written through device-scope accesses everywhere: in the tail launch
// they pass between the waves of one workgroup behind a barrier only
__device__ __forceinline__ spf_word spf_load(const spf_word* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void spf_store(spf_word* p, spf_word v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double spf_dist(const spf_state& S, int32_t v) { return __longlong_as_double((long long) spf_load(&S.dist[v])); }
// end.dist as the round finds it
__device__ __forceinline__ double spf_bound(const spf_state& S) { return S.end >= 0 ? spf_dist(S, S.end) : DBL_MAX; }

// ------------------------------------------------------------------ round pieces (shared by the grid kernels and the tail)
// slot e = n -> s of a queued n at distance d: s.dist_nxt min= d + cost[e], below the bound B only
__device__ __forceinline__ void spf_offer(const spf_state& S, bool on, double d, int32_t e, double B) {
    if (!on) return;
    const double c = d + S.cost[e];
    if (!(c < B)) return;
    const int32_t s = S.node_idx[e];
    const spf_word bits = (spf_word) __double_as_longlong(c);
    if (bits < spf_load(&S.dnxt[s])) atomicMin(&S.dnxt[s], bits);
}

// the same slot once every offer of round r is in: an offer that equals the minimum of a vertex that dropped competes with
// its uploaded slot.  Returns whether it was the first of the round at *s (which then goes on the list of the dropped).
__device__ __forceinline__ bool spf_winner(const spf_state& S, bool on, double d, int32_t e, double B, int32_t r, int32_t* s_out) {
    if (!on) return false;
    const double c = d + S.cost[e];
    if (!(c < B)) return false;
    const int32_t s = S.node_idx[e];
    const spf_word bits = (spf_word) __double_as_longlong(c);
    if (bits != spf_load(&S.dnxt[s]) || !(bits < spf_load(&S.dist[s]))) return false;
    const uint32_t slot = (uint32_t) (S.order ? S.order[e] : e);
    const spf_word key = ((spf_word) (uint32_t) r << 32) | (spf_word) (uint32_t) ~slot;
    *s_out = s;
    if (spf_load(&S.win[s]) < key) return (int32_t) (atomicMax(&S.win[s], key) >> 32) < r;   // replaced an older round's word
    return false;
}

// v dropped in the round: commit it.  Returns the slots of its row when the next round walks it (bn: the bit pattern of the
// next round's bound), else 0.
__device__ __forceinline__ int32_t spf_commit(const spf_state& S, int32_t v, spf_word bn) {
    const spf_word nd = spf_load(&S.dnxt[v]);
    spf_store(&S.dist[v], nd);
    const uint32_t slot = ~(uint32_t) spf_load(&S.win[v]);
    S.prev_edge[v] = (int32_t) slot;
    S.prev_node[v] = csr_row_of(S.begin, S.V, slot);
    return nd < bn ? S.begin[v + 1] - S.begin[v] : 0;
}
__device__ __forceinline__ spf_word spf_next_bound(const spf_state& S) { return S.end >= 0 ? spf_load(&S.dnxt[S.end]) : SPF_MAX_BITS; }

// ------------------------------------------------------------------ grid kernels
// the first queue: the root, unless it is `end` (0 < 0 fails) or has no row
__global__ void __launch_bounds__(SPF_THREADS) spf_init_kernel(spf_state S, int32_t root, int32_t* __restrict__ q) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    if (i == 0) {
        const int32_t deg = root >= 0 && root != S.end ? S.begin[root + 1] - S.begin[root] : 0;
        if (deg > 0) q[0] = root;
        S.ctr->ntouch = root >= 0 ? 1 : 0;
        S.ctr->nnext = deg > 0 ? 1 : 0;
        S.ctr->mnext = (spf_word) deg;
    }
    for (; i < S.V; i += stride) {
        const spf_word d = i == root ? 0ull : SPF_MAX_BITS;
        S.dist[i] = d;
        S.dnxt[i] = d;
        S.win[i] = 0;
        S.prev_node[i] = -1;
        S.prev_edge[i] = -1;
    }
}

// the rows of the queue q[0 .. n), m slots in all, cut into merge-path tiles: the offers of round r, or (WINNER) their winners
template <bool WINNER>
__global__ void __launch_bounds__(BFS_THREADS) spf_walk_kernel(spf_state S, const int32_t* __restrict__ q, int64_t n, const int64_t* __restrict__ off,
                                                               int64_t m, int32_t r) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ double s_d[BFS_ITEMS + 2];
    __shared__ int64_t s_split[2][2];
    __shared__ int32_t s_win[WINNER ? BFS_ITEMS : 1];
    __shared__ unsigned int s_nwin;
    __shared__ spf_word s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_nwin = 0;
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.begin, q, n, off, m, s_off, s_row, [&](int i, int32_t v, bool in) { s_d[i] = in ? spf_dist(S, v) : 0.0; });
    const double B = spf_bound(S);
    for (int64_t base = t.e0; base < t.e1; base += BFS_THREADS) {   // (workgroup-uniform trip count)
        const int64_t x = base + tid;
        const bool on = x < t.e1;
        double d = 0.0;
        int32_t e = 0;
        if (on) {
            const int lo = frontier_slot(s_off, nv, x);
            d = s_d[lo];
            e = (int32_t) ((int64_t) s_row[lo] + (x - s_off[lo]));
        }
        if (WINNER) {
            int32_t s = 0;
            const bool touch = spf_winner(S, on, d, e, B, r, &s);
            wave_append(touch, s, s_win, &s_nwin, lane);
        } else {
            spf_offer(S, on, d, e, B);
        }
    }
    if (WINNER) {
        __syncthreads();
        frontier_flush(s_win, s_nwin, &S.ctr->ntouch, S.touched, &s_base);
    }
}

// touched[0 .. ctr->ntouch), a workgroup per SPF_CHUNK entries; launched for an upper bound of the count
__global__ void __launch_bounds__(SPF_THREADS) spf_commit_kernel(spf_state S, int32_t* __restrict__ next) {
    __shared__ int32_t s_win[SPF_CHUNK];
    __shared__ unsigned int s_nwin;
    __shared__ spf_word s_deg, s_base;
    const int64_t n = (int64_t) S.ctr->ntouch;
    if ((int64_t) blockIdx.x * SPF_CHUNK >= n) return;   // (workgroup-uniform)
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_nwin = 0;
        s_deg = 0;
    }
    __syncthreads();
    const spf_word bn = spf_next_bound(S);
    spf_word deg = 0;
    for (int k = 0; k < SPF_CHUNK / SPF_THREADS; k++) {
        const int64_t i = (int64_t) blockIdx.x * SPF_CHUNK + k * SPF_THREADS + tid;
        int32_t v = 0, dg = 0;
        if (i < n) {
            v = S.touched[i];
            dg = spf_commit(S, v, bn);
        }
        deg += (spf_word) dg;
        wave_append(dg > 0, v, s_win, &s_nwin, lane);
    }
    deg = wave_sum(deg);
    if (lane == 0 && deg) atomicAdd(&s_deg, deg);
    __syncthreads();
    frontier_flush(s_win, s_nwin, &S.ctr->nnext, next, &s_base, [&] {
        if (s_deg) atomicAdd(&S.ctr->mnext, s_deg);
    });
}

// ------------------------------------------------------------------ the tail: one workgroup runs rounds in one launch
// la[0 .. n): the queue of round r, m slots in its rows.  Runs rounds until nothing dropped, the queue is empty, or its rows
// hold more than tail_from slots (the grid takes over again); leaves the last round's counts, the queue in la or lb by the
// parity of the rounds run.  The lists are plain stores of this workgroup, visible to its waves behind the barrier.  The
// rows are walked by tail_rows (gmx_frontier.h).  Every round but the last lowers a distance, each a bounded loop: no waiting on anybody.
__global__ void __launch_bounds__(SPF_TAIL_THREADS) spf_tail_kernel(spf_state S, int32_t* la, int32_t* lb, int64_t n, int64_t m, int32_t r,
                                                                    int64_t tail_from) {
    __shared__ unsigned int s_ntouch, s_nnext;
    __shared__ spf_word s_mnext;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = blockDim.x >> 6;
    if (tid == 0) {
        s_ntouch = 0;
        s_nnext = 0;
        s_mnext = 0;
    }
    __syncthreads();
    spf_word slots = 0, dropped = 0;
    int64_t nt = 0;
    int32_t rounds = 0;
    for (;;) {
        const double B = spf_bound(S);
        for (int pass = 0; pass < 2; pass++) {   // the offers, a barrier, their winners
            const auto slot = [&](bool on, double d, int32_t e) {
                if (pass == 0) {
                    spf_offer(S, on, d, e, B);
                } else {
                    int32_t s = 0;
                    const bool touch = spf_winner(S, on, d, e, B, r, &s);
                    wave_append(touch, s, S.touched, &s_ntouch, lane);
                }
            };
            const auto load = [&](bool have, int32_t v, int32_t) { return have ? spf_dist(S, v) : 0.0; };
            tail_rows<SPF_TAIL_LANE>(la, n, S.begin, lane, wave, nwaves, load, slot);
            __syncthreads();
        }
        nt = (int64_t) s_ntouch;
        const spf_word bn = spf_next_bound(S);
        spf_word deg = 0;
        for (int64_t base = tid - lane; base < nt; base += blockDim.x) {
            const int64_t i = base + lane;
            int32_t v = 0, dg = 0;
            if (i < nt) {
                v = S.touched[i];
                dg = spf_commit(S, v, bn);
            }
            deg += (spf_word) dg;
            wave_append(dg > 0, v, lb, &s_nnext, lane);
        }
        deg = wave_sum(deg);
        if (lane == 0 && deg) atomicAdd(&s_mnext, deg);
        __syncthreads();
        slots += (spf_word) m;
        dropped += (spf_word) nt;
        rounds++;
        n = (int64_t) s_nnext;
        m = (int64_t) s_mnext;
        __syncthreads();
        if (tid == 0) {
            s_ntouch = 0;
            s_nnext = 0;
            s_mnext = 0;
        }
        int32_t* x = la; la = lb; lb = x;
        r++;
        __syncthreads();
        if (nt == 0 || n == 0 || m > tail_from) break;   // (workgroup-uniform)
    }
    if (tid == 0) {
        S.ctr->ntouch = (spf_word) nt;
        S.ctr->nnext = (spf_word) n;
        S.ctr->mnext = (spf_word) m;
        S.ctr->tail_rounds = (spf_word) rounds;
        S.ctr->tail_slots = slots;
        S.ctr->tail_touched = dropped;
    }
}

// ------------------------------------------------------------------ host
// What a call needs besides the graph, kept on the graph for the next call (gmx_internal.h: spf_cache): every word a call
// reads is written by its own init launch first, so nothing passes from one call to the next.
struct spf_scratch {
    dbuf<spf_word> dist, dnxt, win;
    dbuf<int32_t> prev_node, prev_edge, touched, q0, q1;
    dbuf<double> cost, cost_sorted;
    dbuf<spf_counters> ctr;
    frontier_scan fs;
    gmx_pinned<spf_counters> h_ctr;
    int alloc(const gmx_graph* g) {
        const size_t V = (size_t) g->V, E = (size_t) g->E;
        GMX_CHECK(dist.alloc(V));
        GMX_CHECK(dnxt.alloc(V));
        GMX_CHECK(win.alloc(V));
        GMX_CHECK(prev_node.alloc(V));
        GMX_CHECK(prev_edge.alloc(V));
        GMX_CHECK(touched.alloc(V));
        GMX_CHECK(q0.alloc(V));
        GMX_CHECK(q1.alloc(V));
        GMX_CHECK(cost.alloc(E));
        if (g->e_idx2idx.p) GMX_CHECK(cost_sorted.alloc(E));
        GMX_CHECK(ctr.alloc(1));
        GMX_CHECK(gmx_frontier_scan_alloc(&fs, V, 0));
        return h_ctr.alloc(1);
    }
};
void gmx_spf_scratch_free(spf_scratch* s) { delete s; }

extern "C" int gmx_sssp_path_f64(gmx_graph_t* g, gmx_node_t root, gmx_node_t end, const double* cost_host, double* dist_host,
                                 gmx_node_t* prev_node_host, gmx_edge_t* prev_edge_host, gmx_stats_t* stats) {
    GMX_REQUIRE(g && dist_host && prev_node_host, "NULL argument");
    if (stats) memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    GMX_REQUIRE(cost_host || E == 0, "sssp_path_f64: cost is NULL");
    GMX_REQUIRE(end == -1 || (end >= 0 && end < V), "sssp_path_f64: end = %d is neither -1 (no target) nor a vertex of [0, %lld)", (int) end, (long long) V);
    const bool root_ok = root >= 0 && root < V;
    const int64_t tail_from = gmx_env_int("GMX_SSSP_F64_TAIL", SPF_TAIL, 0, INT32_MAX);   // read at every call; the result does not depend on it
    const int64_t log = gmx_env_int("GMX_SSSP_F64_LOG", 0, 0, INT32_MAX);                 // 1: one line per call; 2: a line per grid round and tail launch before it

    if (!g->spf_cache) {
        spf_scratch* fresh = new spf_scratch;
        const int rc = fresh->alloc(g);
        if (rc != GMX_OK) {
            delete fresh;
            return rc;
        }
        g->spf_cache = fresh;
    }
    spf_scratch& W = *g->spf_cache;
    gmx_spans tm;

    spf_state S;
    S.begin = g->begin.p;
    S.node_idx = g->node_idx.p;
    S.cost = W.cost.p;
    S.order = g->e_idx2idx.p;
    S.dist = W.dist.p;
    S.dnxt = W.dnxt.p;
    S.win = W.win.p;
    S.prev_node = W.prev_node.p;
    S.prev_edge = W.prev_edge.p;
    S.touched = W.touched.p;
    S.ctr = W.ctr.p;
    S.V = V;
    S.end = end;
    spf_counters* h = W.h_ctr.p;

    // the property: copied in, checked on the device copy, brought into the order of the sorted rows when the upload sorted them
    GMX_CHECK(tm.begin(tm.H2D));
    GMX_HIP(hipMemsetAsync(W.ctr.p, 0, sizeof(spf_counters), 0));
    if (E) {
        GMX_HIP(hipMemcpyAsync(W.cost.p, cost_host, sizeof(double) * (size_t) E, hipMemcpyHostToDevice, 0));
        hipLaunchKernelGGL((first_bad_slot_kernel<double, spf_counters>), dim3(grid_for(E, SPF_THREADS)), dim3(SPF_THREADS), 0, 0, (const double*) W.cost.p, E, W.ctr.p);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(W.h_ctr, W.ctr.p));
        if (h->bad) {
            const int64_t at = E - (int64_t) h->bad;
            gmx_set_error("sssp_path_f64: cost[%lld] = %g is negative or not a number: every cost must be >= 0", (long long) at, cost_host[at]);
            return GMX_ERR_ARG;
        }
        if (g->e_idx2idx.p) {
            hipLaunchKernelGGL(gather_by_order_kernel<double>, dim3(grid_for(E, SPF_THREADS)), dim3(SPF_THREADS), 0, 0, (const double*) W.cost.p,
                               (const int32_t*) g->e_idx2idx.p, E, W.cost_sorted.p);
            S.cost = W.cost_sorted.p;
        }
    }
    GMX_CHECK(tm.end(tm.H2D));

    GMX_CHECK(tm.begin(tm.KERNEL));
    const double t_start = gmx_tick::now();
    int32_t* la = W.q0.p;   // the queue of the next round
    int32_t* lb = W.q1.p;
    hipLaunchKernelGGL(spf_init_kernel, dim3(grid_for(V, SPF_THREADS)), dim3(SPF_THREADS), 0, 0, S, root_ok ? root : -1, la);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_read_back(W.h_ctr, W.ctr.p));
    int64_t n = (int64_t) h->nnext, m = (int64_t) h->mnext;
    int64_t queued = (int64_t) h->ntouch, grid_slots = 0, tail_slots = 0;
    int32_t rounds = 0, grid_rounds = 0, tail_rounds = 0, tail_launches = 0;
    double tail_ms = 0;
    if (root_ok && n == 0) rounds = 1;   // the root is `end` or has no row: the one round offers nothing
    while (n > 0) {
        const double t_round0 = gmx_tick::now();
        if (tail_from > 0 && m <= tail_from) {   // one workgroup, until the queue outgrows it
            hipLaunchKernelGGL(spf_tail_kernel, dim3(1), dim3(SPF_TAIL_THREADS), 0, 0, S, la, lb, n, m, rounds + 1, tail_from);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(W.h_ctr, W.ctr.p));
            const int32_t ran = (int32_t) h->tail_rounds;
            rounds += ran;
            tail_rounds += ran;
            tail_launches++;
            tail_slots += (int64_t) h->tail_slots;
            queued += (int64_t) h->tail_touched;
            if (ran & 1) { int32_t* x = la; la = lb; lb = x; }
            tail_ms += (gmx_tick::now() - t_round0) * 1e3;
            if (log >= 2)
                fprintf(stderr, "gmx sssp_path_f64 tail launch %d: from round %d, %d rounds, slots %llu dropped %llu ms %.3f\n", tail_launches,
                        rounds - ran + 1, ran, h->tail_slots, h->tail_touched, (gmx_tick::now() - t_round0) * 1e3);
        } else {
            GMX_HIP(hipMemsetAsync(&W.ctr.p->ntouch, 0, 3 * sizeof(spf_word), 0));   // ntouch, nnext, mnext
            GMX_CHECK(gmx_frontier_offsets(g->begin.p, la, n, &W.fs, nullptr, false));
            const int64_t nb = frontier_tiles(n, m);
            hipLaunchKernelGGL(spf_walk_kernel<false>, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, S, (const int32_t*) la, n, (const int64_t*) W.fs.off.p, m, rounds + 1);
            hipLaunchKernelGGL(spf_walk_kernel<true>, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, S, (const int32_t*) la, n, (const int64_t*) W.fs.off.p, m, rounds + 1);
            const int64_t most = m < V ? m : V;   // a slot drops at most one vertex
            hipLaunchKernelGGL(spf_commit_kernel, dim3((unsigned) ((most + SPF_CHUNK - 1) / SPF_CHUNK)), dim3(SPF_THREADS), 0, 0, S, lb);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(W.h_ctr, W.ctr.p));
            rounds++;
            grid_rounds++;
            grid_slots += m;
            queued += (int64_t) h->ntouch;
            { int32_t* x = la; la = lb; lb = x; }
            if (log >= 2)
                fprintf(stderr, "gmx sssp_path_f64 round %d: queue %lld slots %lld dropped %llu queued %llu ms %.3f\n", rounds, (long long) n, (long long) m,
                        h->ntouch, h->nnext, (gmx_tick::now() - t_round0) * 1e3);
        }
        if (h->ntouch == 0) break;   // nothing dropped: the loop's last round
        n = (int64_t) h->nnext;
        m = (int64_t) h->mnext;
        if (n == 0) rounds++;        // vertices dropped, none of them below the bound with a row: one more round, which offers nothing
    }
    GMX_CHECK(tm.end(tm.KERNEL));
    const double t_end = gmx_tick::now();

    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpyAsync(dist_host, W.dist.p, sizeof(double) * (size_t) V, hipMemcpyDeviceToHost, 0));
    GMX_HIP(hipMemcpyAsync(prev_node_host, W.prev_node.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    if (prev_edge_host) GMX_HIP(hipMemcpyAsync(prev_edge_host, W.prev_edge.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));   // (the downloads have landed)
    if (stats) {
        stats->iterations = rounds;
        stats->edges_examined = grid_slots + tail_slots;
        stats->vertices_reached = queued;
    }
    if (log >= 1)   // one line per call (tools/spf_prof.py and the tests parse it)
        fprintf(stderr, "gmx sssp_path_f64: V %lld E %lld root %d end %d; tail %lld; rounds %d: %d grid + %d tail in %d launches; queued %lld; "
                        "slots %lld grid + %lld tail; ms %.3f grid + %.3f tail\n",
                (long long) V, (long long) E, (int) root, (int) end, (long long) tail_from, rounds, grid_rounds, tail_rounds, tail_launches,
                (long long) queued, (long long) grid_slots, (long long) tail_slots, (t_end - t_start) * 1e3 - tail_ms, tail_ms);
    return GMX_OK;
}

void gmx_touch_spf() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) spf_tail_kernel);
}
