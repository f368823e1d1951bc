// gmx_kcore.hip -- k-core decomposition on gfx950: synchronous peeling in queue rounds.  The reference has no such program;
// the definition, the schedule that fixes layer[] and the statistics are the contract at gmx_kcore in gmx.h.
//
// One word deg[v] per vertex: the counted slots of v whose other end is still live.  It only ever falls, by atomic
// decrements of 1, so every value is returned to exactly one decrement: the one that sees k + 1 removes the vertex.
//   degrees   row lengths of begin / r_begin minus the self-loop slots (counted by one pass over the forward rows); mode IN
//             without a reverse CSR: a histogram of node_idx instead.
//   level     k = the smallest degree of a live vertex.  kcore_min_kernel reduces it over the live list, kcore_scan_kernel
//             then cuts the list in three: entries removed in an earlier round (deg <= the previous k) are dropped, deg <= k
//             goes to the queue with core = k and layer = the round, the rest is the next list.  The minimum cannot be taken
//             by the scan of the level before: that scan runs before the level's rounds lower the degrees, and a minimum
//             over the values the decrements return also holds those of vertices that the same level goes on to remove.
//   round     the rows of the queue segment [qs, qe) go through the merge-path tile (gmx_frontier.h): a plain load of the
//             other end's degree, the atomic only while that is above k, and the decrement that returns k + 1 appends.  A
//             vertex is queued once in the whole run, so ONE array q[V] holds every round's segment behind the other, and
//             in the end a degeneracy ordering.  A stale degree is a larger one: it costs an atomic, never a removal.
//   tail      while the queue's rows hold at most GMX_KCORE_TAIL slots (and, at a level's start, the list at most as many
//             entries) one workgroup runs rounds and level scans with a barrier between them and hands back otherwise.
// The schedule does not depend on the order of the decrements: whether a vertex reaches k within a round does not, and
// core, layer and the segment bounds follow from that alone.  Only the order inside a segment and inside the list varies.
#include "gmx_frontier.h"

#define KC_THREADS BFS_THREADS
#define KC_TAIL_THREADS 1024
#define KC_TAIL 1024         // GMX_KCORE_TAIL: the tail launch takes over while the queue to expand holds at most this many slots
#define KC_TAIL_LANE 8       // the tail reads a row of at most this many slots with one lane, a longer one with a wave
#define KC_NONE 0xFFFFFFFFu  // the minimum over no vertex

typedef unsigned long long kc_word;

struct kc_ctl {
    kc_word qtail;       // tail of q[]: vertices removed so far
    kc_word slots[2];    // row slots (forward, reverse) of q[0, qtail)
    kc_word nkeep;       // tail of the list the scan writes
    kc_word overflow;    // a degree above INT32_MAX
    // what the tail hands back
    long long t_qs, t_qe, t_nlist, t_levels, t_rounds, t_scanned, t_walked, t_level_q0, t_m[2];
    int32_t t_k, t_state, t_swapped, t_pad;
    unsigned int maxdec, pad0;
    kc_word pad1[15];
    struct {
        unsigned int mindeg;
        unsigned int pad[31];
    } shard[BFS_SHARDS];
};
enum { KC_DONE = 0, KC_BOUNDARY = 1, KC_MIDLEVEL = 2 };

struct kc_state {
    const int32_t* beg[2];   // the rows a removal walks: forward (IN), reverse (OUT), both (BOTH)
    const int32_t* idx[2];
    int ndir;
    int32_t* deg;
    int32_t* core;
    int32_t* layer;          // or NULL
    int32_t* q;
    kc_ctl* ctl;
    int64_t V;
};

__device__ __forceinline__ int32_t kc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int kc_shard() { return (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (BFS_SHARDS - 1); }

// ---- degrees
// one pass over the forward slots, BFS_ITEMS at a time; the row of a slot is searched between the rows of the chunk's first
// and last slot.  HIST: deg[w]++ for every slot u -> w with u != w (mode IN without a reverse CSR); else self[u]++ for u -> u.
template <bool HIST>
__global__ void __launch_bounds__(KC_THREADS) kcore_slots_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int64_t E,
                                                                 int32_t* __restrict__ out) {
    __shared__ int32_t s_row[2];
    for (int64_t c0 = (int64_t) blockIdx.x * BFS_ITEMS; c0 < E; c0 += (int64_t) gridDim.x * BFS_ITEMS) {
        const int64_t c1 = c0 + BFS_ITEMS < E ? c0 + BFS_ITEMS : E;
        if (threadIdx.x < 2) s_row[threadIdx.x] = csr_row_of(begin, V, (uint32_t) (threadIdx.x ? c1 - 1 : c0));
        __syncthreads();
        const int32_t r0 = s_row[0], r1 = s_row[1];
        for (int64_t e = c0 + threadIdx.x; e < c1; e += KC_THREADS) {
            const int32_t w = idx[e];
            int32_t lo = r0, hi = r1;
            while (lo < hi) {
                const int32_t mid = (int32_t) (((int64_t) lo + hi + 1) >> 1);
                if ((int64_t) begin[mid] <= e) lo = mid; else hi = mid - 1;
            }
            if (HIST ? w != lo : w == lo) atomicAdd(&out[HIST ? w : lo], 1);
        }
        __syncthreads();
    }
}
// deg[v] = in-slots (in != NULL) + out-slots (out != NULL) - the self-loop slots, which are in both
__global__ void __launch_bounds__(KC_THREADS) kcore_degree_kernel(const int32_t* __restrict__ in, const int32_t* __restrict__ out, const int32_t* __restrict__ self,
                                                                  int64_t V, int32_t* __restrict__ deg, kc_ctl* __restrict__ ctl) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        int64_t d = 0;
        if (in) d += (int64_t) in[v + 1] - in[v] - self[v];
        if (out) d += (int64_t) out[v + 1] - out[v] - self[v];
        if (d > INT32_MAX) {
            ctl->overflow = 1;
            d = INT32_MAX;
        }
        deg[v] = (int32_t) d;
    }
}

// ---- a level's start on the grid
// the smallest degree above kprev among list[0, n) (list == NULL: the vertices 0 .. n-1) into the sharded words
__global__ void __launch_bounds__(KC_THREADS) kcore_min_kernel(const int32_t* __restrict__ list, int64_t n, const int32_t* __restrict__ deg, int32_t kprev,
                                                               kc_ctl* __restrict__ ctl) {
    unsigned int mn = KC_NONE;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const int32_t d = deg[list ? list[i] : (int32_t) i];
        if (d > kprev) mn = min(mn, (unsigned int) d);
    }
    mn = wave_min(mn);
    if ((threadIdx.x & 63) == 0 && mn != KC_NONE) atomicMin(&ctl->shard[kc_shard()].mindeg, mn);
}

// what belongs to queueing v in round `layer` of level k; returns nothing, adds v's row slots to m[]
__device__ __forceinline__ void kc_remove(const kc_state& S, int32_t v, int32_t k, int32_t layer, kc_word* m) {
    S.core[v] = k;
    if (S.layer) S.layer[v] = layer;
    for (int d = 0; d < S.ndir; d++) {
        const int32_t len = S.beg[d][v + 1] - S.beg[d][v];
        if (len) atomicAdd(&m[d], (kc_word) len);
    }
}

// list[0, n) -> dropped (deg <= kprev: removed by a round of the level before), queued (deg <= k) or kept (out[]); a
// workgroup collects BFS_ITEMS entries in LDS and claims each tail once
__global__ void __launch_bounds__(KC_THREADS) kcore_scan_kernel(kc_state S, const int32_t* __restrict__ list, int64_t n, int32_t kprev, int32_t k, int32_t round,
                                                                int32_t* __restrict__ out) {
    __shared__ int32_t s_keep[BFS_ITEMS], s_q[BFS_ITEMS];
    __shared__ unsigned int s_nkeep, s_nq;
    __shared__ kc_word s_m[2], s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t t0 = (int64_t) blockIdx.x * BFS_ITEMS; t0 < n; t0 += (int64_t) gridDim.x * BFS_ITEMS) {
        if (tid == 0) {
            s_nkeep = s_nq = 0;
            s_m[0] = s_m[1] = 0;
        }
        __syncthreads();
        for (int j = 0; j < BFS_ITEMS / KC_THREADS; j++) {
            const int64_t i = t0 + j * KC_THREADS + tid;
            const int32_t v = i < n ? (list ? list[i] : (int32_t) i) : 0;
            const int32_t d = i < n ? S.deg[v] : kprev;
            wave_append(d > kprev && d <= k, v, s_q, &s_nq, lane, [&] { kc_remove(S, v, k, round, s_m); });
            wave_append(d > k, v, s_keep, &s_nkeep, lane);
        }
        __syncthreads();
        frontier_flush(s_keep, s_nkeep, &S.ctl->nkeep, out, &s_base);
        __syncthreads();
        frontier_flush(s_q, s_nq, &S.ctl->qtail, S.q, &s_base, [&] {
            for (int d = 0; d < S.ndir; d++)
                if (s_m[d]) atomicAdd(&S.ctl->slots[d], s_m[d]);
        });
        __syncthreads();
    }
}

// ---- a round on the grid: one merge-path tile of the rows (direction dir) of queue[0, n) at level k
__global__ void __launch_bounds__(KC_THREADS) kcore_round_kernel(kc_state S, int dir, const int32_t* __restrict__ queue, int64_t n, const int64_t* __restrict__ off,
                                                                 int64_t m, int32_t k, int32_t next_round) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_v[BFS_ITEMS + 2];
    __shared__ int32_t s_list[BFS_ITEMS];
    __shared__ int64_t s_split[2][2];
    __shared__ unsigned int s_n;
    __shared__ kc_word s_m[2], s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_n = 0;
        s_m[0] = s_m[1] = 0;
    }
    const int32_t* __restrict__ idx = S.idx[dir];
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.beg[dir], queue, n, off, m, s_off, s_row, [&](int i, int32_t v, bool) { s_v[i] = v; });
    if (t.e1 <= t.e0) return;   // (workgroup-uniform)
    constexpr int K = BFS_ITEMS / KC_THREADS;
    int32_t w[K], d[K];
    bool act[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int64_t x = t.e0 + tid + (int64_t) j * KC_THREADS;
        const int64_t xc = x < t.e1 ? x : t.e0;   // (loads stay unconditional: a slot that exists)
        const int lo = frontier_slot(s_off, nv, xc);
        w[j] = idx[(int64_t) s_row[lo] + (xc - s_off[lo])];
        act[j] = x < t.e1 && w[j] != s_v[lo];
    }
#pragma unroll
    for (int j = 0; j < K; j++) d[j] = S.deg[w[j]];
#pragma unroll
    for (int j = 0; j < K; j++) {
        bool last = false;
        if (act[j] && d[j] > k) last = atomicSub(&S.deg[w[j]], 1) == k + 1;
        wave_append(last, w[j], s_list, &s_n, lane, [&] { kc_remove(S, w[j], k, next_round, s_m); });
    }
    __syncthreads();
    frontier_flush(s_list, s_n, &S.ctl->qtail, S.q, &s_base, [&] {
        for (int dd = 0; dd < S.ndir; dd++)
            if (s_m[dd]) atomicAdd(&S.ctl->slots[dd], s_m[dd]);
    });
}

// ---- the tail: one workgroup goes on from the host's state -- the list la[0, nlist) (identity: the vertices themselves),
// the level k, the queue segment [qs, qe) of round `round` whose rows hold m0 + m1 slots -- until nobody is live (KC_DONE),
// a level would start on a list of more than tail_from entries (KC_BOUNDARY) or a queue's rows hold more than tail_from
// slots (KC_MIDLEVEL).  deg[] is read with agent-scope loads: the values come from atomics, and the level scan must see
// them as they are.  q[], the lists, core and layer are plain stores of this workgroup, read behind its barrier.
__global__ void __launch_bounds__(KC_TAIL_THREADS) kcore_tail_kernel(kc_state S, int32_t* la, int32_t* lb, int identity, int64_t nlist, int32_t k,
                                                                     int32_t round, int64_t qs, int64_t qe, int64_t level_q0, int64_t m0, int64_t m1,
                                                                     int64_t tail_from) {
    __shared__ unsigned int s_tail, s_keep, s_min;
    __shared__ kc_word s_m[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = blockDim.x >> 6;
    if (tid == 0) {
        s_tail = (unsigned int) qe;
        s_keep = 0;
        s_min = KC_NONE;
        s_m[0] = s_m[1] = 0;
    }
    __syncthreads();
    kc_word walked = 0;
    kc_word tot[2] = {0, 0};   // row slots of what this launch queued
    long long levels = 0, rounds = 0, scanned = 0;
    int swapped = 0, state = KC_DONE;
    for (;;) {
        if (qs == qe) {   // a level starts
            if (nlist == 0) break;
            if (nlist > tail_from) {
                state = KC_BOUNDARY;
                break;
            }
            unsigned int mn = KC_NONE;
            for (int64_t i = tid; i < nlist; i += KC_TAIL_THREADS) {
                const int32_t d = kc_load(&S.deg[identity ? (int32_t) i : la[i]]);
                if (d > k) mn = min(mn, (unsigned int) d);
            }
            mn = wave_min(mn);
            if (lane == 0 && mn != KC_NONE) atomicMin(&s_min, mn);
            __syncthreads();
            const unsigned int knew = s_min;
            if (knew == KC_NONE) {   // every entry was removed by the last rounds (workgroup-uniform)
                nlist = 0;
                break;
            }
            for (int64_t base = tid - lane; base < nlist; base += KC_TAIL_THREADS) {
                const int64_t i = base + lane;
                const int32_t v = i < nlist ? (identity ? (int32_t) i : la[i]) : 0;
                const int32_t d = i < nlist ? kc_load(&S.deg[v]) : k;
                wave_append(d > k && d <= (int32_t) knew, v, S.q, &s_tail, lane, [&] { kc_remove(S, v, (int32_t) knew, round, s_m); });
                wave_append(d > (int32_t) knew, v, lb, &s_keep, lane);
            }
            __syncthreads();
            levels++;
            scanned += nlist;
            nlist = (int64_t) s_keep;
            k = (int32_t) knew;
            level_q0 = qs;
            int32_t* x = la; la = lb; lb = x;
            swapped ^= 1;
            identity = 0;
        } else {   // a round
            if (m0 + m1 > tail_from) {
                state = KC_MIDLEVEL;
                break;
            }
            const auto load = [&](bool, int32_t v, int32_t len) {
                walked += (kc_word) len;
                return v;
            };
            for (int dir = 0; dir < S.ndir; dir++) {
                const int32_t* __restrict__ idx = S.idx[dir];
                const auto slot = [&](bool on, int32_t u, int32_t e) {
                    const int32_t w = on ? idx[e] : u;
                    bool last = false;
                    if (w != u && kc_load(&S.deg[w]) > k) last = atomicSub(&S.deg[w], 1) == k + 1;
                    wave_append(last, w, S.q, &s_tail, lane, [&] { kc_remove(S, w, k, round + 1, s_m); });
                };
                tail_rows<KC_TAIL_LANE>(S.q + qs, qe - qs, S.beg[dir], lane, wave, nwaves, load, slot);
            }
            __syncthreads();
            rounds++;
            round++;
            qs = qe;
        }
        // behind either step's barrier: the queue's new end and the slots of its rows
        qe = (int64_t) s_tail;
        m0 = (int64_t) s_m[0];
        m1 = (int64_t) s_m[1];
        tot[0] += (kc_word) m0;
        tot[1] += (kc_word) m1;
        __syncthreads();
        if (tid == 0) {
            s_keep = 0;
            s_min = KC_NONE;
            s_m[0] = s_m[1] = 0;
        }
        __syncthreads();
    }
    walked = wave_sum(walked);
    if (lane == 0 && walked) atomicAdd((kc_word*) &S.ctl->t_walked, walked);
    if (tid == 0) {
        kc_ctl* c = S.ctl;
        c->qtail = (kc_word) s_tail;
        c->slots[0] += tot[0];
        c->slots[1] += tot[1];
        c->t_qs = qs;
        c->t_qe = qe;
        c->t_nlist = nlist;
        c->t_levels = levels;
        c->t_rounds = rounds;
        c->t_scanned = scanned;
        c->t_level_q0 = level_q0;
        c->t_m[0] = m0;
        c->t_m[1] = m1;
        c->t_k = k;
        c->t_state = state;
        c->t_swapped = swapped;
    }
}

// the largest number of decrements one vertex received (GMX_KCORE_PHASES): deg0 is the copy taken before the first level
__global__ void __launch_bounds__(KC_THREADS) kcore_maxdec_kernel(const int32_t* __restrict__ deg0, const int32_t* __restrict__ deg, int64_t V,
                                                                  kc_ctl* __restrict__ ctl) {
    int32_t mx = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) mx = max(mx, deg0[v] - deg[v]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctl->maxdec, (unsigned int) mx);
}

// ------------------------------------------------------------------ host
extern "C" int gmx_kcore(gmx_graph_t* g, int mode, int32_t* core_host, int32_t* layer_host, int32_t* max_core, gmx_stats_t* stats_out) {
    GMX_REQUIRE(core_host, "NULL argument");
    GMX_REQUIRE(g, "NULL argument");
    GMX_REQUIRE(mode >= GMX_KCORE_IN && mode <= GMX_KCORE_BOTH, "kcore: mode %d is none of GMX_KCORE_IN, _OUT, _BOTH", mode);
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    if (max_core) *max_core = 0;
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    if (mode != GMX_KCORE_IN && !g->has_reverse) {
        gmx_set_error("kcore: modes OUT and BOTH need the reverse CSR");
        return GMX_ERR_STATE;
    }
    const int64_t tail_from = gmx_env_int("GMX_KCORE_TAIL", KC_TAIL, 0, INT64_MAX);   // read at every call; the result does not depend on it
    const bool phase_log = getenv("GMX_KCORE_PHASES") != nullptr;                       // per-phase times for tools/kcore_prof.py

    gmx_ws_scope scope;
    wbuf<int32_t> deg, core, layer, q, l0, l1, deg0;
    wbuf<kc_ctl> ctl;
    GMX_CHECK(deg.alloc(V));
    GMX_CHECK(core.alloc(V));
    if (layer_host) GMX_CHECK(layer.alloc(V));
    GMX_CHECK(q.alloc(V));
    GMX_CHECK(l0.alloc(V));
    GMX_CHECK(l1.alloc(V));
    if (phase_log) GMX_CHECK(deg0.alloc(V));
    GMX_CHECK(ctl.alloc(1));
    int32_t* selfcnt = l0.p;   // (the first scan reads the identity and writes l1: l0 is free until the second)

    kc_state S;
    S.ndir = mode == GMX_KCORE_BOTH ? 2 : 1;
    S.beg[0] = mode == GMX_KCORE_OUT ? g->r_begin.p : g->begin.p;
    S.idx[0] = mode == GMX_KCORE_OUT ? g->r_node_idx.p : g->node_idx.p;
    S.beg[1] = mode == GMX_KCORE_BOTH ? g->r_begin.p : S.beg[0];
    S.idx[1] = mode == GMX_KCORE_BOTH ? g->r_node_idx.p : S.idx[0];
    S.deg = deg.p;
    S.core = core.p;
    S.layer = layer_host ? layer.p : nullptr;
    S.q = q.p;
    S.ctl = ctl.p;
    S.V = V;

    frontier_scan fs[2];
    for (int d = 0; d < S.ndir; d++) GMX_CHECK(gmx_frontier_scan_alloc(&fs[d], (size_t) V, 0));
    gmx_pinned<kc_ctl> h_ctl;
    GMX_CHECK(h_ctl.alloc());
    const kc_ctl* h = h_ctl.p;
    gmx_spans tm;
    const int gv = grid_for(V);
    float ph_ms[4] = {0, 0, 0, 0};   // degrees, scans, grid rounds, tail (GMX_KCORE_PHASES): device time around every step;
    gmx_phase_clock phase;           // each step ends in a read-back, so the clock's wait costs no overlap
    GMX_CHECK(phase.enable(phase_log));

    // ---- degrees
    GMX_CHECK(tm.begin(tm.KERNEL));
    phase.begin();
    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(kc_ctl), 0));
    if (mode == GMX_KCORE_IN && !g->has_reverse) {
        GMX_HIP(hipMemsetAsync(deg.p, 0, sizeof(int32_t) * (size_t) V, 0));
        if (E > 0)
            hipLaunchKernelGGL(kcore_slots_kernel<true>, dim3(grid_for(E, BFS_ITEMS)), dim3(KC_THREADS), 0, 0, (const int32_t*) g->begin.p,
                               (const int32_t*) g->node_idx.p, V, E, deg.p);
    } else {
        GMX_HIP(hipMemsetAsync(selfcnt, 0, sizeof(int32_t) * (size_t) V, 0));
        if (E > 0)
            hipLaunchKernelGGL(kcore_slots_kernel<false>, dim3(grid_for(E, BFS_ITEMS)), dim3(KC_THREADS), 0, 0, (const int32_t*) g->begin.p,
                               (const int32_t*) g->node_idx.p, V, E, selfcnt);
        hipLaunchKernelGGL(kcore_degree_kernel, dim3(gv), dim3(KC_THREADS), 0, 0, mode != GMX_KCORE_OUT ? (const int32_t*) g->r_begin.p : (const int32_t*) nullptr,
                           mode != GMX_KCORE_IN ? (const int32_t*) g->begin.p : (const int32_t*) nullptr, (const int32_t*) selfcnt, V, deg.p, ctl.p);
    }
    GMX_HIP(hipGetLastError());
    if (phase_log) GMX_HIP(hipMemcpyAsync(deg0.p, deg.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToDevice, 0));
    GMX_CHECK(gmx_read_back(h_ctl, (const kc_ctl*) ctl.p));
    GMX_REQUIRE(!h->overflow, "kcore: a vertex has more than INT32_MAX counted slots");
    phase.end(&ph_ms[0]);

    // ---- levels and rounds
    int32_t* la = l0.p;   // the live list (identity: the vertices 0 .. V-1, nothing stored yet)
    int32_t* lb = l1.p;
    bool identity = true;
    int64_t nlist = V, qs = 0, qe = 0, level_q0 = 0;
    int64_t at_qs[2] = {0, 0}, at_qe[2] = {0, 0};   // row slots of q[0, qs) and q[0, qe)
    int64_t levels = 0, scanned = 0, grid_rounds = 0, tail_rounds = 0, walked = 0;
    int32_t k = -1, round = 0;
    for (;;) {
        const bool boundary = qs == qe;
        if (boundary && nlist == 0) break;
        const int64_t m[2] = {at_qe[0] - at_qs[0], at_qe[1] - at_qs[1]};
        if (tail_from > 0 && (boundary ? nlist : m[0] + m[1]) <= tail_from) {
            phase.begin();
            hipLaunchKernelGGL(kcore_tail_kernel, dim3(1), dim3(KC_TAIL_THREADS), 0, 0, S, la, lb, identity ? 1 : 0, nlist, k, round, qs, qe, level_q0, m[0], m[1],
                               tail_from);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, (const kc_ctl*) ctl.p));
            phase.end(&ph_ms[3]);
            if (h->t_levels) identity = false;
            if (h->t_swapped) std::swap(la, lb);
            levels += h->t_levels;
            scanned += h->t_scanned;
            tail_rounds += h->t_rounds;
            round += (int32_t) h->t_rounds;
            qs = h->t_qs;
            qe = h->t_qe;
            nlist = h->t_nlist;
            level_q0 = h->t_level_q0;
            k = h->t_k;
            for (int d = 0; d < 2; d++) {
                at_qe[d] = (int64_t) h->slots[d];
                at_qs[d] = at_qe[d] - h->t_m[d];
            }
            if (h->t_state == KC_DONE) break;
            continue;   // KC_BOUNDARY / KC_MIDLEVEL: the step it stopped at is too large for one workgroup and runs on the grid
        }
        if (qs == qe) {   // a level starts: its k, then the scan
            phase.begin();
            GMX_HIP(hipMemsetAsync(&ctl.p->shard[0], 0xff, sizeof(ctl.p->shard), 0));
            GMX_HIP(hipMemsetAsync(&ctl.p->nkeep, 0, sizeof(kc_word), 0));
            hipLaunchKernelGGL(kcore_min_kernel, dim3(grid_for(nlist)), dim3(KC_THREADS), 0, 0,
                               identity ? (const int32_t*) nullptr : (const int32_t*) la, nlist, (const int32_t*) deg.p, k, ctl.p);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, (const kc_ctl*) ctl.p));
            unsigned int mn = KC_NONE;
            for (int i = 0; i < BFS_SHARDS; i++) mn = std::min(mn, h->shard[i].mindeg);
            if (mn == KC_NONE) {   // every entry was removed by the last rounds
                nlist = 0;
                phase.end(&ph_ms[1]);
                break;
            }
            hipLaunchKernelGGL(kcore_scan_kernel, dim3(grid_for(nlist, BFS_ITEMS)), dim3(KC_THREADS), 0, 0, S,
                               identity ? (const int32_t*) nullptr : (const int32_t*) la, nlist, k, (int32_t) mn, round, lb);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, (const kc_ctl*) ctl.p));
            phase.end(&ph_ms[1]);
            levels++;
            scanned += nlist;
            k = (int32_t) mn;
            nlist = (int64_t) h->nkeep;
            std::swap(la, lb);
            identity = false;
            level_q0 = qs;
            qe = (int64_t) h->qtail;
            for (int d = 0; d < 2; d++) at_qe[d] = (int64_t) h->slots[d];
        } else {   // a round
            phase.begin();
            const int64_t n = qe - qs;
            for (int d = 0; d < S.ndir; d++) {
                if (m[d] == 0) continue;
                GMX_CHECK(gmx_frontier_offsets(S.beg[d], q.p + qs, n, &fs[d], nullptr, false));
                hipLaunchKernelGGL(kcore_round_kernel, dim3((unsigned) frontier_tiles(n, m[d])), dim3(KC_THREADS), 0, 0, S, d, (const int32_t*) (q.p + qs), n,
                                   (const int64_t*) fs[d].off.p, m[d], k, round + 1);
                walked += m[d];
            }
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, (const kc_ctl*) ctl.p));
            phase.end(&ph_ms[2]);
            grid_rounds++;
            round++;
            qs = qe;
            qe = (int64_t) h->qtail;
            for (int d = 0; d < 2; d++) {
                at_qs[d] = at_qe[d];
                at_qe[d] = (int64_t) h->slots[d];
            }
        }
    }
    if (phase_log) {
        hipLaunchKernelGGL(kcore_maxdec_kernel, dim3(gv), dim3(KC_THREADS), 0, 0, (const int32_t*) deg0.p, (const int32_t*) deg.p, V, ctl.p);
        GMX_HIP(hipGetLastError());
    }
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(gmx_read_back(h_ctl, (const kc_ctl*) ctl.p));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(core_host, core.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    if (layer_host) GMX_HIP(hipMemcpy(layer_host, layer.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    if ((int64_t) h->qtail != V) {
        gmx_set_error("kcore: %lld of %lld vertices were removed", (long long) h->qtail, (long long) V);
        return GMX_ERR_HIP;
    }
    walked += h->t_walked;
    const int64_t top = V - level_q0;   // the last level's removals: the vertices of the largest core
    if (max_core) *max_core = k;
    stats->iterations = round;
    stats->vertices_reached = top;
    stats->edges_examined = walked;
    if (phase_log)
        fprintf(stderr, "gmx kcore phases: degrees %.3f ms, scans %.3f ms, grid %.3f ms, tail %.3f ms, max_decrements %u\n", ph_ms[0], ph_ms[1], ph_ms[2], ph_ms[3],
                h->maxdec);
    if (getenv("GMX_KCORE_LOG"))
        fprintf(stderr,
                "gmx kcore: V %lld E %lld mode %d reverse %d levels %lld rounds %d scanned %lld grid_rounds %lld tail_rounds %lld slots %lld max_core %d top %lld\n",
                (long long) V, (long long) E, mode, g->has_reverse ? 1 : 0, (long long) levels, (int) round, (long long) scanned, (long long) grid_rounds,
                (long long) tail_rounds, (long long) walked, (int) k, (long long) top);
    return GMX_OK;
}

void gmx_touch_kcore() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) kcore_tail_kernel);
}
