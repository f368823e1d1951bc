// gmx_bicc.hip -- bridges, articulation points, biconnected components and 2-edge-connected components on gfx950.  The
// reference has no such program; the graph read, the numbering rules and the statistics are the contract at gmx_biconnected
// in gmx.h.  The scheme is a spanning forest and one walk per non-tree slot:
//   forest    the roots are the smallest vertex of every weak component (gmx_wcc_forest).  One level-synchronous BFS from all
//             of them over out-rows and in-rows through the merge-path tile (gmx_frontier.h): level[w] is claimed by a CAS
//             from -1, par[w] is the atomicMin over every claimant of the previous level, so the tree does not depend on
//             the order of the claims.  A vertex is queued once, so ONE array q[V] holds every level behind the other.
//   tail      while a level's rows hold at most GMX_BICC_TAIL slots one workgroup runs the levels with a barrier between
//             them: a cycle of 4096 has 2048 levels of two vertices.
//   walks     a non-root x stands for the tree edge e(x) = {par[x], x}.  cls[V] is a union-find forest over those, hooked
//             by id with wcc_hook and under its memory rule.  Every forward slot u -> w that is no self loop and no tree
//             slot walks: cursors x = u, y = w; while they differ the one of the greater level (x on a tie) has its edge
//             linked with the walk's first edge and moves up.  ONLY the deeper cursor moves, and there is no exit on equal
//             classes: mid-walk a class is connected only through the non-tree edge, and such an exit joins too little.
//   jumps     skip[v] = t says "all tree edges on the path from v up to its ancestor t are in one class".  A cursor at v
//             moves to skip[v] where that differs from v.  A jump may overshoot the lowest common ancestor; the other cursor
//             then climbs over edges that the fact already puts into the class of a cycle edge, so no two blocks are joined
//             that should stay apart.  After the cursors met at M a second climb from either end writes skip[v] = M where M
//             is higher than what v holds.  Racing writers all write true facts, facts never become false, so a stale read
//             costs steps only; every loop strictly lowers a level, so it ends within the forest's depth whatever it reads.
//   finish    cls compressed.  A tree edge is a bridge when nobody else is in its class.  A non-root p is an articulation
//             point when a child's class differs from its own, a root when its children span two classes.  A slot's block
//             is the class of its child end (tree slot) or of its deeper end; the ids are the ranks of the blocks' smallest
//             uploaded slots.  tecc: wcc_hook over the ends of every non-bridge slot, then gmx_wcc's finish.
// Host round trips: those of gmx_wcc_forest, one per BFS level on the grid and per tail launch, the results.
#include "gmx_frontier.h"

#include <rocprim/rocprim.hpp>

#define BICC_THREADS BFS_THREADS
#define BICC_TAIL_THREADS 1024
#define BICC_TAIL 1024        // GMX_BICC_TAIL: the tail launch takes over while the level's rows hold at most this many slots
#define BICC_TAIL_LANE 8      // the tail reads a row of at most this many slots with one lane, a longer one with a wave
#define BICC_WALKS 1048576    // GMX_BICC_WALKS: forward slots per walk launch
#define BICC_NONE INT32_MAX

typedef unsigned long long bicc_word;

struct bicc_ctl {
    bicc_word qtail;      // tail of q[]: vertices with a level
    bicc_word slots[2];   // row slots (forward, reverse) of q[0, qtail)
    // what the tail hands back
    long long t_qs, t_qe, t_levels, t_m[2];
    int32_t t_level, t_pad;
    int32_t nblocks, nbridges, nartic, ntecc;
    bicc_word pad0[6];
    struct {
        bicc_word walks, steps, jumps, links;
        bicc_word pad[12];
    } shard[BFS_SHARDS];
};

struct bicc_state {
    const int32_t* beg[2];   // forward, reverse
    const int32_t* idx[2];
    int32_t* level;
    int32_t* par;
    int32_t* q;
    bicc_ctl* ctl;
};

__device__ __forceinline__ int bicc_shard() { return (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (BFS_SHARDS - 1); }

// ---- forest
// roots (root[v] == v) get level 0 and go to the queue; cls and skip start as the identity
__global__ void __launch_bounds__(BICC_THREADS) bicc_init_kernel(bicc_state S, const int32_t* __restrict__ root, int64_t V, int32_t* __restrict__ cls,
                                                                 int32_t* __restrict__ skip) {
    __shared__ int32_t s_list[BFS_ITEMS];
    __shared__ unsigned int s_n;
    __shared__ bicc_word s_m[2], s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t t0 = (int64_t) blockIdx.x * BFS_ITEMS; t0 < V; t0 += (int64_t) gridDim.x * BFS_ITEMS) {
        if (tid == 0) {
            s_n = 0;
            s_m[0] = s_m[1] = 0;
        }
        __syncthreads();
        for (int k = 0; k < BFS_ITEMS / BICC_THREADS; k++) {
            const int64_t v = t0 + k * BICC_THREADS + tid;
            const bool is_root = v < V && root[v] == (int32_t) v;
            if (v < V) {
                S.level[v] = is_root ? 0 : -1;
                S.par[v] = is_root ? (int32_t) v : BICC_NONE;
                cls[v] = (int32_t) v;
                skip[v] = (int32_t) v;
            }
            wave_append(is_root, (int32_t) v, s_list, &s_n, lane, [&] {
                for (int d = 0; d < 2; d++) {
                    const int32_t len = S.beg[d][v + 1] - S.beg[d][v];
                    if (len) atomicAdd(&s_m[d], (bicc_word) len);
                }
            });
        }
        __syncthreads();
        frontier_flush(s_list, s_n, &S.ctl->qtail, S.q, &s_base, [&] {
            for (int d = 0; d < 2; d++)
                if (s_m[d]) atomicAdd(&S.ctl->slots[d], s_m[d]);
        });
        __syncthreads();
    }
}

// the slot u -> w (or w -> u) seen from u of level L: true when this call gave w its level.  lw: level[w] as loaded (a
// stale -1 is settled by the CAS; any other value is final).  Every claimant of level L + 1 offers itself as the parent.
__device__ __forceinline__ bool bicc_claim(const bicc_state& S, int32_t u, int32_t w, int32_t lw, int32_t L) {
    bool claimed = false;
    if (lw == -1) {
        lw = atomicCAS(&S.level[w], -1, L + 1);
        claimed = lw == -1;
        if (claimed) lw = L + 1;
    }
    if (lw == L + 1) atomicMin(&S.par[w], u);
    return claimed;
}
__device__ __forceinline__ void bicc_queued(const bicc_state& S, int32_t w, bicc_word* m) {
    for (int d = 0; d < 2; d++) {
        const int32_t len = S.beg[d][w + 1] - S.beg[d][w];
        if (len) atomicAdd(&m[d], (bicc_word) len);
    }
}

// a level on the grid: one merge-path tile of the rows (direction dir) of queue[0, n), whose vertices have level L
__global__ void __launch_bounds__(BICC_THREADS) bicc_level_kernel(bicc_state S, int dir, const int32_t* __restrict__ queue, int64_t n,
                                                                  const int64_t* __restrict__ off, int64_t m, int32_t L) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_v[BFS_ITEMS + 2];
    __shared__ int32_t s_list[BFS_ITEMS];
    __shared__ int64_t s_split[2][2];
    __shared__ unsigned int s_n;
    __shared__ bicc_word s_m[2], s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_n = 0;
        s_m[0] = s_m[1] = 0;
    }
    const int32_t* __restrict__ idx = S.idx[dir];
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.beg[dir], queue, n, off, m, s_off, s_row, [&](int i, int32_t v, bool) { s_v[i] = v; });
    if (t.e1 <= t.e0) return;   // (workgroup-uniform)
    constexpr int K = BFS_ITEMS / BICC_THREADS;
    int32_t u[K], w[K], lw[K];
    bool act[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int64_t x = t.e0 + tid + (int64_t) j * BICC_THREADS;
        const int64_t xc = x < t.e1 ? x : t.e0;   // (loads stay unconditional: a slot that exists)
        const int lo = frontier_slot(s_off, nv, xc);
        u[j] = s_v[lo];
        w[j] = idx[(int64_t) s_row[lo] + (xc - s_off[lo])];
        act[j] = x < t.e1 && w[j] != u[j];
    }
#pragma unroll
    for (int j = 0; j < K; j++) lw[j] = S.level[w[j]];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const bool claimed = act[j] && bicc_claim(S, u[j], w[j], lw[j], L);
        wave_append(claimed, w[j], s_list, &s_n, lane, [&] { bicc_queued(S, w[j], s_m); });
    }
    __syncthreads();
    frontier_flush(s_list, s_n, &S.ctl->qtail, S.q, &s_base, [&] {
        for (int d = 0; d < 2; d++)
            if (s_m[d]) atomicAdd(&S.ctl->slots[d], s_m[d]);
    });
}

// the tail: one workgroup goes on from the host's state -- the queue segment [qs, qe) of level L whose rows hold m0 + m1
// slots -- until a level finds nobody (qs == qe) or a level's rows hold more than tail_from slots.  level[] is read with
// agent-scope loads; q[] is this workgroup's plain stores, read behind its barrier.
__global__ void __launch_bounds__(BICC_TAIL_THREADS) bicc_tail_kernel(bicc_state S, int64_t qs, int64_t qe, int32_t L, int64_t m0, int64_t m1,
                                                                      int64_t tail_from) {
    __shared__ unsigned int s_tail;
    __shared__ bicc_word s_m[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = blockDim.x >> 6;
    if (tid == 0) {
        s_tail = (unsigned int) qe;
        s_m[0] = s_m[1] = 0;
    }
    __syncthreads();
    bicc_word tot[2] = {0, 0};   // row slots of what this launch queued
    long long levels = 0;
    while (qs < qe && m0 + m1 <= tail_from) {
        const auto load = [&](bool, int32_t v, int32_t) { return v; };
        for (int dir = 0; dir < 2; dir++) {
            const int32_t* __restrict__ idx = S.idx[dir];
            const auto slot = [&](bool on, int32_t u, int32_t e) {
                const int32_t w = on ? idx[e] : u;
                const bool claimed = w != u && bicc_claim(S, u, w, wcc_load(&S.level[w]), L);
                wave_append(claimed, w, S.q, &s_tail, lane, [&] { bicc_queued(S, w, s_m); });
            };
            tail_rows<BICC_TAIL_LANE>(S.q + qs, qe - qs, S.beg[dir], lane, wave, nwaves, load, slot);
        }
        __syncthreads();
        levels++;
        L++;
        qs = qe;
        qe = (int64_t) s_tail;
        m0 = (int64_t) s_m[0];
        m1 = (int64_t) s_m[1];
        tot[0] += (bicc_word) m0;
        tot[1] += (bicc_word) m1;
        __syncthreads();
        if (tid == 0) s_m[0] = s_m[1] = 0;
        __syncthreads();
    }
    if (tid == 0) {
        bicc_ctl* c = S.ctl;
        c->qtail = (bicc_word) s_tail;
        c->slots[0] += tot[0];
        c->slots[1] += tot[1];
        c->t_qs = qs;
        c->t_qe = qe;
        c->t_levels = levels;
        c->t_m[0] = m0;
        c->t_m[1] = m1;
        c->t_level = L;
    }
}

// ---- the forward slots [s0, s1) in device order, BFS_ITEMS at a time: f(e, u) for slot e of row u.  The row of a slot is
// searched between the rows of the chunk's first and last slot.  The whole workgroup calls this; f holds no collective.
template <class F>
__device__ __forceinline__ void bicc_slots(const int32_t* __restrict__ begin, int64_t V, int64_t s0, int64_t s1, int32_t* s_row, F f) {
    for (int64_t c0 = s0 + (int64_t) blockIdx.x * BFS_ITEMS; c0 < s1; c0 += (int64_t) gridDim.x * BFS_ITEMS) {
        const int64_t c1 = c0 + BFS_ITEMS < s1 ? c0 + BFS_ITEMS : s1;
        if (threadIdx.x < 2) s_row[threadIdx.x] = csr_row_of(begin, V, (uint32_t) (threadIdx.x ? c1 - 1 : c0));
        __syncthreads();
        const int32_t r0 = s_row[0], r1 = s_row[1];
        for (int64_t e = c0 + threadIdx.x; e < c1; e += BICC_THREADS) {
            int32_t lo = r0, hi = r1;
            while (lo < hi) {
                const int32_t mid = (int32_t) (((int64_t) lo + hi + 1) >> 1);
                if ((int64_t) begin[mid] <= e) lo = mid; else hi = mid - 1;
            }
            f(e, lo);
        }
        __syncthreads();
    }
}

// ---- walks
// a vertex that was the root of x's class when it was read; the vertices passed are pointed at their grandparents
// (atomicMin: ancestors descend towards the root, so no late write undoes a better one).  Agent-scope loads throughout.
__device__ __forceinline__ int32_t bicc_find(int32_t* __restrict__ cls, int32_t x) {
    int32_t p = wcc_load(&cls[x]);
    if (p == x) return x;
    for (;;) {
        const int32_t gp = wcc_load(&cls[p]);
        if (gp == p) return p;
        atomicMin(&cls[x], gp);
        x = p;
        p = gp;
    }
}

__global__ void __launch_bounds__(BICC_THREADS) bicc_walk_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int64_t s0,
                                                                 int64_t s1, const int32_t* __restrict__ level, const int32_t* __restrict__ par,
                                                                 int32_t* __restrict__ cls, int32_t* skip, int use_skip, bicc_ctl* __restrict__ ctl) {
    __shared__ int32_t s_row[2];
    bicc_word walks = 0, steps = 0, jumps = 0, links = 0;
    bicc_slots(begin, V, s0, s1, s_row, [&](int64_t e, int32_t u) {
        const int32_t w = idx[e];
        if (w == u || par[u] == w || par[w] == u) return;
        walks++;
        int32_t x = u, y = w, lx = level[u], ly = level[w];
        int32_t c0 = -1;   // a vertex of the class of the walk's first edge
        while (x != y) {
            const bool dx = lx >= ly;
            const int32_t d = dx ? x : y, ld = dx ? lx : ly;
            if (ld <= 0) break;   // (two cursors of one tree meet at its root at the latest)
            const int32_t a = bicc_find(cls, d);
            if (c0 < 0) c0 = a;
            else if (a != c0) {
                links++;
                wcc_hook(cls, a, c0);
                c0 = a < c0 ? a : c0;
            }
            steps++;
            int32_t nx = par[d], ln = ld - 1;
            if (use_skip) {
                const int32_t s = wcc_load(&skip[d]);
                if (s != d) {
                    nx = s;
                    ln = level[s];
                    jumps++;
                }
            }
            if (dx) {
                x = nx;
                lx = ln;
            } else {
                y = nx;
                ly = ln;
            }
        }
        if (use_skip && x == y) {   // the facts: every tree edge from u, and from w, up to M = x is in one class now
            const int32_t M = x, lM = lx;
            for (int side = 0; side < 2; side++) {
                int32_t v = side ? w : u, lv = level[v];
                while (lv > lM) {
                    const int32_t s = wcc_load(&skip[v]);
                    const bool jump = s != v;
                    const int32_t ls = jump ? level[s] : lv;
                    if (ls > lM) __hip_atomic_store(&skip[v], M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // M is higher than what v holds
                    v = jump ? s : par[v];
                    lv = jump ? ls : lv - 1;
                }
            }
        }
    });
    walks = wave_sum(walks);
    steps = wave_sum(steps);
    jumps = wave_sum(jumps);
    links = wave_sum(links);
    if ((threadIdx.x & 63) == 0 && walks) {
        const int sh = bicc_shard();
        atomicAdd(&ctl->shard[sh].walks, walks);
        atomicAdd(&ctl->shard[sh].steps, steps);
        if (jumps) atomicAdd(&ctl->shard[sh].jumps, jumps);
        if (links) atomicAdd(&ctl->shard[sh].links, links);
    }
}

// ---- finish (cls is compressed: cls[v] = the root of v's class; cls[root of the forest] stays itself and means nothing)
// shared[c] = 1 when another tree edge is in the class of root c; lo / hi start as the empty range
__global__ void __launch_bounds__(BICC_THREADS) bicc_mark_kernel(const int32_t* __restrict__ cls, const int32_t* __restrict__ level, int64_t V,
                                                                 int32_t* __restrict__ shared, int32_t* __restrict__ lo, int32_t* __restrict__ hi) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const int32_t c = cls[v];
        if (level[v] > 0 && c != (int32_t) v) shared[c] = 1;
        lo[v] = BICC_NONE;
        hi[v] = -1;
    }
}
// isbr[v]: the tree edge e(v) is a bridge.  artic[p] for a non-root p with a child of another class; the classes of a root's
// children go into lo / hi of the root.
__global__ void __launch_bounds__(BICC_THREADS) bicc_vertex_kernel(const int32_t* __restrict__ cls, const int32_t* __restrict__ level,
                                                                   const int32_t* __restrict__ par, const int32_t* __restrict__ shared, int64_t V,
                                                                   int32_t* __restrict__ isbr, uint8_t* artic, int32_t* lo, int32_t* hi,
                                                                   bicc_ctl* __restrict__ ctl) {
    int32_t nb = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const bool child = level[v] > 0;
        const int32_t c = cls[v];
        const bool br = child && c == (int32_t) v && !shared[v];
        isbr[v] = br ? 1 : 0;
        nb += br ? 1 : 0;
        if (child) {
            const int32_t p = par[v];
            if (level[p] > 0) {
                if (cls[p] != c) artic[p] = 1;
            } else {
                atomicMin(&lo[p], c);
                atomicMax(&hi[p], c);
            }
        }
    }
    nb = wave_sum(nb);
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(&ctl->nbridges, nb);
}
__global__ void __launch_bounds__(BICC_THREADS) bicc_artic_kernel(const int32_t* __restrict__ level, const int32_t* __restrict__ lo,
                                                                  const int32_t* __restrict__ hi, int64_t V, uint8_t* __restrict__ artic,
                                                                  bicc_ctl* __restrict__ ctl) {
    int32_t na = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        if (level[v] == 0 && hi[v] > lo[v]) artic[v] = 1;
        na += artic[v];
    }
    na = wave_sum(na);
    if ((threadIdx.x & 63) == 0 && na) atomicAdd(&ctl->nartic, na);
}

__global__ void __launch_bounds__(BICC_THREADS) bicc_fill_kernel(int32_t* __restrict__ a, int64_t n, int32_t x) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) a[i] = x;
}

// the slot u -> w: its tree edge's child end when it is a tree slot (else -1), and the vertex whose class is its block
__device__ __forceinline__ void bicc_slot_ends(const int32_t* __restrict__ level, const int32_t* __restrict__ par, int32_t u, int32_t w, int32_t* child,
                                               int32_t* deep) {
    *child = par[u] == w ? u : (par[w] == u ? w : -1);
    *deep = *child >= 0 ? *child : (level[u] >= level[w] ? u : w);
}
// first[c] = the smallest uploaded slot of the block with class root c (order: uploaded slot of a device slot, or NULL)
__global__ void __launch_bounds__(BICC_THREADS) bicc_first_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int64_t E,
                                                                  const int32_t* __restrict__ order, const int32_t* __restrict__ level,
                                                                  const int32_t* __restrict__ par, const int32_t* __restrict__ cls,
                                                                  int32_t* __restrict__ first) {
    __shared__ int32_t s_row[2];
    bicc_slots(begin, V, 0, E, s_row, [&](int64_t e, int32_t u) {
        const int32_t w = idx[e];
        if (w == u) return;
        int32_t child, deep;
        bicc_slot_ends(level, par, u, w, &child, &deep);
        const int32_t us = order ? order[e] : (int32_t) e;
        const int32_t c = cls[deep];
        if (first[c] > us) atomicMin(&first[c], us);
    });
}
__global__ void __launch_bounds__(BICC_THREADS) bicc_flag_kernel(const int32_t* __restrict__ first, int64_t V, int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x)
        if (first[v] != BICC_NONE) flag[first[v]] = 1;
}
// the edge results by uploaded slot; rank: the exclusive scan of flag (both NULL with block_out)
__global__ void __launch_bounds__(BICC_THREADS) bicc_out_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int64_t E,
                                                                const int32_t* __restrict__ order, const int32_t* __restrict__ level,
                                                                const int32_t* __restrict__ par, const int32_t* __restrict__ cls,
                                                                const int32_t* __restrict__ isbr, const int32_t* __restrict__ first,
                                                                const int32_t* __restrict__ flag, const int32_t* __restrict__ rank,
                                                                uint8_t* __restrict__ bridge_out, int32_t* __restrict__ block_out, bicc_ctl* __restrict__ ctl) {
    __shared__ int32_t s_row[2];
    bicc_slots(begin, V, 0, E, s_row, [&](int64_t e, int32_t u) {
        const int32_t w = idx[e];
        const int32_t us = order ? order[e] : (int32_t) e;
        int32_t child = -1, deep = -1;
        if (w != u) bicc_slot_ends(level, par, u, w, &child, &deep);
        if (bridge_out) bridge_out[us] = child >= 0 && isbr[child] ? 1 : 0;
        if (block_out) {
            block_out[us] = deep >= 0 ? rank[first[cls[deep]]] : -1;
            if (e == E - 1) ctl->nblocks = rank[E - 1] + flag[E - 1];
        }
    });
}
// tecc: the ends of every slot that is no self loop and no bridge are linked in t[]
__global__ void __launch_bounds__(BICC_THREADS) bicc_tecc_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int64_t E,
                                                                 const int32_t* __restrict__ par, const int32_t* __restrict__ isbr, int32_t* __restrict__ t) {
    __shared__ int32_t s_row[2];
    bicc_slots(begin, V, 0, E, s_row, [&](int64_t e, int32_t u) {
        const int32_t w = idx[e];
        if (w == u) return;
        const int32_t child = par[u] == w ? u : (par[w] == u ? w : -1);
        if (child >= 0 && isbr[child]) return;
        wcc_hook(t, t[u], t[w]);
    });
}

// ------------------------------------------------------------------ host
extern "C" int gmx_biconnected(gmx_graph_t* g, uint8_t* bridge_host, uint8_t* artic_host, int32_t* block_host, int32_t* tecc_host, int64_t* num_blocks,
                               int64_t* num_bridges, int64_t* num_artic, int64_t* num_tecc, gmx_stats_t* stats_out) {
    GMX_REQUIRE(g, "NULL argument");
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    if (num_blocks) *num_blocks = 0;
    if (num_bridges) *num_bridges = 0;
    if (num_artic) *num_artic = 0;
    if (num_tecc) *num_tecc = 0;
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    if (!g->has_reverse) {
        gmx_set_error("biconnected: needs the reverse CSR");
        return GMX_ERR_STATE;
    }
    // read at every call; no result byte depends on them
    const int64_t tail_from = gmx_env_int("GMX_BICC_TAIL", BICC_TAIL, 0, INT64_MAX);
    const int use_skip = gmx_env_int("GMX_BICC_SKIP", 1, 0, 1) != 0 ? 1 : 0;
    const int64_t per_launch = gmx_env_int("GMX_BICC_WALKS", BICC_WALKS, 0, INT64_MAX);
    const bool phase_log = getenv("GMX_BICC_PHASES") != nullptr;   // per-phase times for tools/bicc_prof.py
    const bool want_tecc = tecc_host || num_tecc;
    const bool want_block = (block_host || num_blocks) && E > 0;
    const bool want_artic = artic_host || num_artic;
    const bool want_bridge = bridge_host || num_bridges || want_tecc;
    const bool want_vertex = want_artic || want_bridge;

    gmx_ws_scope scope;
    wbuf<int32_t> root, level, par, cls, skip, q, shared, isbr, lo, hi, first, flag, rank, block, tecc_parent, tecc;
    wbuf<uint8_t> artic, bridge;
    wbuf<bicc_ctl> ctl;
    wbuf<char> scan_tmp;
    GMX_CHECK(root.alloc(V));
    GMX_CHECK(level.alloc(V));
    GMX_CHECK(par.alloc(V));
    GMX_CHECK(cls.alloc(V));
    GMX_CHECK(skip.alloc(V));
    GMX_CHECK(q.alloc(V));
    GMX_CHECK(ctl.alloc(1));
    if (want_vertex) {
        GMX_CHECK(shared.alloc(V));
        GMX_CHECK(isbr.alloc(V));
        GMX_CHECK(lo.alloc(V));
        GMX_CHECK(hi.alloc(V));
        GMX_CHECK(artic.alloc(V));
    }
    size_t scan_bytes = 0;
    const int64_t FR = std::max(V, E);   // flag / rank serve the block ranks (E words) and gmx_wcc_canon (V words)
    if (want_block || want_tecc) {
        GMX_CHECK(flag.alloc(FR));
        GMX_CHECK(rank.alloc(FR));
    }
    if (want_block) {
        GMX_CHECK(first.alloc(V));
        GMX_CHECK(block.alloc(E));
        GMX_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag.p, rank.p, 0, (size_t) E, rocprim::plus<int32_t>(), 0));
        GMX_CHECK(scan_tmp.alloc(scan_bytes));
    }
    if (bridge_host && E > 0) GMX_CHECK(bridge.alloc(E));
    if (want_tecc) {
        GMX_CHECK(tecc_parent.alloc(V));
        GMX_CHECK(tecc.alloc(V));
    }
    frontier_scan fs[2];
    for (int d = 0; d < 2; d++) GMX_CHECK(gmx_frontier_scan_alloc(&fs[d], (size_t) V, 0));
    gmx_pinned<bicc_ctl> h_ctl;
    GMX_CHECK(h_ctl.alloc());
    const bicc_ctl* h = h_ctl.p;

    bicc_state S;
    S.beg[0] = g->begin.p;
    S.idx[0] = g->node_idx.p;
    S.beg[1] = g->r_begin.p;
    S.idx[1] = g->r_node_idx.p;
    S.level = level.p;
    S.par = par.p;
    S.q = q.p;
    S.ctl = ctl.p;
    const int32_t* begin = g->begin.p;
    const int32_t* idx = g->node_idx.p;
    const int32_t* order = g->e_idx2idx.p;   // uploaded slot of a device slot, or NULL: the same
    const int gv = grid_for(V), ge = grid_for(E, BFS_ITEMS);
    gmx_spans tm;
    float ph_ms[3] = {0, 0, 0};   // forest, walks, finish (GMX_BICC_PHASES)
    gmx_phase_clock phase;
    GMX_CHECK(phase.enable(phase_log));

    // ---- forest
    GMX_CHECK(tm.begin(tm.KERNEL));
    phase.begin();
    GMX_CHECK(gmx_wcc_forest(g, root.p));
    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(bicc_ctl), 0));
    hipLaunchKernelGGL(bicc_init_kernel, dim3(grid_for(V, BFS_ITEMS)), dim3(BICC_THREADS), 0, 0, S, (const int32_t*) root.p, V, cls.p, skip.p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_read_back(h_ctl, (const bicc_ctl*) ctl.p));
    const int64_t roots = (int64_t) h->qtail;
    int64_t qs = 0, qe = roots, grid_levels = 0, tail_levels = 0;
    int64_t at_qs[2] = {0, 0}, at_qe[2] = {(int64_t) h->slots[0], (int64_t) h->slots[1]};   // row slots of q[0, qs) and q[0, qe)
    int32_t L = 0;
    while (qs < qe) {
        const int64_t m[2] = {at_qe[0] - at_qs[0], at_qe[1] - at_qs[1]};
        if (tail_from > 0 && m[0] + m[1] <= tail_from) {
            hipLaunchKernelGGL(bicc_tail_kernel, dim3(1), dim3(BICC_TAIL_THREADS), 0, 0, S, qs, qe, L, m[0], m[1], tail_from);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, (const bicc_ctl*) ctl.p));
            tail_levels += h->t_levels;
            qs = h->t_qs;
            qe = h->t_qe;
            L = h->t_level;
            for (int d = 0; d < 2; d++) {
                at_qe[d] = (int64_t) h->slots[d];
                at_qs[d] = at_qe[d] - h->t_m[d];
            }
            continue;   // done (qs == qe), or a level too large for one workgroup: it runs on the grid
        }
        const int64_t n = qe - qs;
        for (int d = 0; d < 2; d++) {
            if (m[d] == 0) continue;
            GMX_CHECK(gmx_frontier_offsets(S.beg[d], q.p + qs, n, &fs[d], nullptr, false));
            hipLaunchKernelGGL(bicc_level_kernel, dim3((unsigned) frontier_tiles(n, m[d])), dim3(BICC_THREADS), 0, 0, S, d, (const int32_t*) (q.p + qs), n,
                               (const int64_t*) fs[d].off.p, m[d], L);
        }
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctl, (const bicc_ctl*) ctl.p));
        grid_levels++;
        L++;
        qs = qe;
        qe = (int64_t) h->qtail;
        for (int d = 0; d < 2; d++) {
            at_qs[d] = at_qe[d];
            at_qe[d] = (int64_t) h->slots[d];
        }
    }
    phase.end(&ph_ms[0]);
    if (qe != V) {
        gmx_set_error("biconnected: %lld of %lld vertices were reached", (long long) qe, (long long) V);
        return GMX_ERR_HIP;
    }

    // ---- walks
    phase.begin();
    const int64_t per = per_launch > 0 ? per_launch : E;
    for (int64_t s0 = 0; s0 < E; s0 += per) {
        const int64_t s1 = E - s0 < per ? E : s0 + per;
        hipLaunchKernelGGL(bicc_walk_kernel, dim3(grid_for(s1 - s0, BFS_ITEMS)), dim3(BICC_THREADS), 0, 0, begin, idx, V, s0, s1, (const int32_t*) level.p,
                           (const int32_t*) par.p, cls.p, skip.p, use_skip, ctl.p);
    }
    GMX_HIP(hipGetLastError());
    phase.end(&ph_ms[1]);

    // ---- finish
    phase.begin();
    GMX_CHECK(gmx_wcc_compress(cls.p, V));
    if (want_vertex) {
        GMX_HIP(hipMemsetAsync(shared.p, 0, sizeof(int32_t) * (size_t) V, 0));
        GMX_HIP(hipMemsetAsync(artic.p, 0, (size_t) V, 0));
        hipLaunchKernelGGL(bicc_mark_kernel, dim3(gv), dim3(BICC_THREADS), 0, 0, (const int32_t*) cls.p, (const int32_t*) level.p, V, shared.p, lo.p, hi.p);
        hipLaunchKernelGGL(bicc_vertex_kernel, dim3(gv), dim3(BICC_THREADS), 0, 0, (const int32_t*) cls.p, (const int32_t*) level.p, (const int32_t*) par.p,
                           (const int32_t*) shared.p, V, isbr.p, artic.p, lo.p, hi.p, ctl.p);
        hipLaunchKernelGGL(bicc_artic_kernel, dim3(gv), dim3(BICC_THREADS), 0, 0, (const int32_t*) level.p, (const int32_t*) lo.p, (const int32_t*) hi.p, V,
                           artic.p, ctl.p);
    }
    if (want_block) {
        hipLaunchKernelGGL(bicc_fill_kernel, dim3(gv), dim3(BICC_THREADS), 0, 0, first.p, V, (int32_t) BICC_NONE);
        GMX_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t) * (size_t) E, 0));
    }
    GMX_HIP(hipGetLastError());
    if (want_block) {
        hipLaunchKernelGGL(bicc_first_kernel, dim3(ge), dim3(BICC_THREADS), 0, 0, begin, idx, V, E, order, (const int32_t*) level.p, (const int32_t*) par.p,
                           (const int32_t*) cls.p, first.p);
        hipLaunchKernelGGL(bicc_flag_kernel, dim3(gv), dim3(BICC_THREADS), 0, 0, (const int32_t*) first.p, V, flag.p);
        GMX_HIP(rocprim::exclusive_scan((void*) scan_tmp.p, scan_bytes, flag.p, rank.p, 0, (size_t) E, rocprim::plus<int32_t>(), 0));
    }
    if (E > 0 && (bridge_host || want_block))
        hipLaunchKernelGGL(bicc_out_kernel, dim3(ge), dim3(BICC_THREADS), 0, 0, begin, idx, V, E, order, (const int32_t*) level.p, (const int32_t*) par.p,
                           (const int32_t*) cls.p, (const int32_t*) isbr.p, (const int32_t*) first.p, (const int32_t*) flag.p, (const int32_t*) rank.p,
                           bridge_host ? bridge.p : (uint8_t*) nullptr, want_block ? block.p : (int32_t*) nullptr, ctl.p);
    GMX_HIP(hipGetLastError());
    if (want_tecc) {
        hipLaunchKernelGGL(iota_kernel, dim3(gv), dim3(BFS_THREADS), 0, 0, tecc_parent.p, V);
        if (E > 0)
            hipLaunchKernelGGL(bicc_tecc_kernel, dim3(ge), dim3(BICC_THREADS), 0, 0, begin, idx, V, E, (const int32_t*) par.p, (const int32_t*) isbr.p,
                               tecc_parent.p);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_wcc_canon(tecc_parent.p, V, flag.p, rank.p, tecc.p, &ctl.p->ntecc));
    }
    phase.end(&ph_ms[2]);
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(gmx_read_back(h_ctl, (const bicc_ctl*) ctl.p));
    GMX_CHECK(tm.begin(tm.D2H));
    if (bridge_host && E > 0) GMX_HIP(hipMemcpy(bridge_host, bridge.p, (size_t) E, hipMemcpyDeviceToHost));
    if (artic_host) GMX_HIP(hipMemcpy(artic_host, artic.p, (size_t) V, hipMemcpyDeviceToHost));
    if (block_host && E > 0) GMX_HIP(hipMemcpy(block_host, block.p, sizeof(int32_t) * (size_t) E, hipMemcpyDeviceToHost));
    if (tecc_host) GMX_HIP(hipMemcpy(tecc_host, tecc.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    bicc_word walks = 0, steps = 0, jumps = 0, links = 0;
    for (int i = 0; i < BFS_SHARDS; i++) {
        walks += h->shard[i].walks;
        steps += h->shard[i].steps;
        jumps += h->shard[i].jumps;
        links += h->shard[i].links;
    }
    if (num_blocks) *num_blocks = h->nblocks;
    if (num_bridges) *num_bridges = h->nbridges;
    if (num_artic) *num_artic = h->nartic;
    if (num_tecc) *num_tecc = h->ntecc;
    stats->iterations = (int32_t) (grid_levels + tail_levels);
    stats->vertices_reached = V - roots;
    stats->edges_examined = (int64_t) steps;
    if (phase_log) fprintf(stderr, "gmx bicc phases: forest %.3f ms, walks %.3f ms, finish %.3f ms\n", ph_ms[0], ph_ms[1], ph_ms[2]);
    if (getenv("GMX_BICC_LOG"))
        fprintf(stderr,
                "gmx bicc: V %lld E %lld levels %lld roots %lld tree %lld walks %llu steps %llu jumps %llu links %llu grid_levels %lld tail_levels %lld blocks "
                "%d bridges %d artic %d tecc %d\n",
                (long long) V, (long long) E, (long long) (grid_levels + tail_levels), (long long) roots, (long long) (V - roots), walks, steps, jumps, links,
                (long long) grid_levels, (long long) tail_levels, want_block || E == 0 ? (int) h->nblocks : -1, want_bridge ? (int) h->nbridges : -1,
                want_artic ? (int) h->nartic : -1, want_tecc ? (int) h->ntecc : -1);
    return GMX_OK;
}

void gmx_touch_bicc() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) bicc_tail_kernel);
}
