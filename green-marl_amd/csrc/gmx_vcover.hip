// gmx_vcover.hip -- v_cover (greedy vertex cover by heaviest edge) for gfx950.
//
// Replaces the body of apps/src/v_cover.gm:
//     G.Deg = G.Degree() + G.InDegree();  G.Covered = False;  G.select = False;  remain = 2 E;
//     While (remain > 0) {
//         <max_val; from, to, e> = arg-max of s.Deg + t.Deg over the edges s -> t with !(s.Covered && t.Covered);
//         remain -= max_val;  from.Deg = to.Deg = 0;  e.select = True;  from.Covered = to.Covered = True; }
//     Return Count(t: G.Nodes)(t.Covered);
// as ONE thread runs it: among the edges of maximal key the lowest forward slot wins (gmx.h).  One arg-max over E edges per
// selected edge is replaced by an exact reformulation with O(E) work in total:
//   - keys only fall, and only when an endpoint is covered.  An edge that is the best edge (key descending, slot ascending)
//     of each of its UNCOVERED endpoints is chosen by the loop before anything that could change its key: all such edges
//     are picked in one parallel round;
//   - the loop's pick order is the picks sorted by (key descending, slot ascending); `remain` is replayed over that order
//     and the picks behind the first remain <= 0 are dropped (only self-loop picks make the cut fire);
//   - the best edge of an uncovered u is the first entry with an uncovered other end of u's incident list sorted by
//     (Deg0[other] descending, slot ascending) -- a cursor that only moves forward -- or, with the list exhausted, u's
//     lowest incident slot.  u is evaluated again only when the other end of its best edge was covered by another edge;
//     those vertices are found by walking the lists of the newly covered vertices, each list once in the whole run.
// Plan (graph preprocessing, cached on the graph, outside kernel_ms): Deg0, the list offsets (begin + r_begin), the lists as
// (other endpoint, UPLOADED slot) and per vertex the list position of its lowest slot.  The round kernels never see a
// device slot.
// A round: activate (newly covered queue -> next active list, merge-path tiles of gmx_frontier.h), evaluate (cursor and
// best word of every active vertex), pick (record, cover, queue).  "Covered" is the round a vertex was covered in, so a
// pick kernel reads the state before its own round whatever its neighbours write.  Once few vertices are active one
// workgroup runs the rounds to the end (vc_tail_kernel).  Integer only: exact.
#include "gmx_frontier.h"

#include <limits.h>
#include <rocprim/rocprim.hpp>

#define VC_THREADS 256
#define VC_TAIL_THREADS 1024
#define VC_TAIL 2048     // GMX_VC_TAIL: the tail launch takes over once a round had at most this many active vertices
#define VC_WAVE 128      // GMX_VC_WAVE: a wave advances the cursor of a list with at least this many entries left
#define VC_CHUNKS 4      // 64-entry pieces of a list a wave keeps in flight while it advances a cursor
#define VC_INF INT_MAX

enum { VC_NACT, VC_NCOV, VC_MCOV, VC_NPICK, VC_SELF, VC_SKIPS, VC_EVALS, VC_WALKS, VC_ACTSUM, VC_KEPT, VC_COVERED, VC_NCTR = 16 };

struct vc_plan {
    int64_t V = 0, E = 0, L = 0;
    double build_ms = 0;
    dbuf<int32_t> deg0;   // [V]      out-degree + in-degree
    dbuf<int32_t> off;    // [V + 1]  list offsets
    dbuf<int32_t> low;    // [V]      list position of the lowest incident slot (-1: no edges)
    dbuf<int2> ent;       // [L]      x = other endpoint, y = uploaded slot
};

void gmx_vc_plan_free(vc_plan* p) { delete p; }

struct vc_state {
    const int32_t* deg0;
    const int32_t* off;
    const int32_t* low;
    const int2* ent;
    int32_t* cov;                   // [V] round the vertex was covered in, VC_INF: uncovered
    int32_t* stamp;                 // [V] last round the vertex was active in
    int32_t* cur;                   // [V] cursor into the list
    int32_t* bent;                  // [V] list position of the best edge
    unsigned long long* best;       // [V] key << 32 | ~slot
    unsigned long long* pickword;   // [V] best word of every pick
    int2* pickuv;                   // [V] its endpoints
    unsigned long long* ctr;        // [VC_NCTR]
    int64_t V;
    int32_t wave_min;
};

// ------------------------------------------------------------------ plan kernels
__global__ void vc_degree_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ r_begin, int64_t V,
                                 int32_t* __restrict__ deg0, int32_t* __restrict__ off) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; v <= V; v += stride) {
        off[v] = begin[v] + r_begin[v];
        if (v < V) deg0[v] = (begin[v + 1] - begin[v]) + (r_begin[v + 1] - r_begin[v]);
    }
}

// Both list entries of every slot, written at the position of its UPLOADED slot: the stable sort by (owner, Deg0[other]
// descending) that follows then leaves equal keys in ascending uploaded slot.
__global__ void vc_entries_kernel(const uint64_t* __restrict__ fwd, const int32_t* __restrict__ order, const int32_t* __restrict__ deg0,
                                  int64_t E, uint64_t* __restrict__ keys, uint64_t* __restrict__ vals) {
    int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; e < E; e += stride) {
        const uint64_t k = fwd[e];
        const uint64_t s = k >> 32, d = k & 0xffffffffu;
        const uint64_t u = order ? (uint64_t) (uint32_t) order[e] : (uint64_t) e;
        keys[2 * u] = (s << 32) | (uint64_t) (0xffffffffu - (uint32_t) deg0[d]);
        vals[2 * u] = (u << 32) | d;
        keys[2 * u + 1] = (d << 32) | (uint64_t) (0xffffffffu - (uint32_t) deg0[s]);
        vals[2 * u + 1] = (u << 32) | s;
    }
}

// a wave per vertex: the list position of its lowest slot (the first of a self loop's two entries)
__global__ void vc_low_kernel(const int32_t* __restrict__ off, const int2* __restrict__ ent, int64_t V, int32_t* __restrict__ low) {
    const int lane = threadIdx.x & 63;
    int64_t v = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t stride = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (; v < V; v += stride) {
        const int32_t b = off[v], e = off[v + 1];
        unsigned long long m = ~0ULL;
        for (int32_t i = b + lane; i < e; i += 64) {
            const unsigned long long w = ((unsigned long long) (uint32_t) ent[i].y << 32) | (uint32_t) i;
            m = w < m ? w : m;
        }
        m = wave_min(m);
        if (lane == 0) low[v] = b < e ? (int32_t) (uint32_t) m : -1;
    }
}

// ------------------------------------------------------------------ round pieces (shared by the grid kernels and the tail)
__global__ void vc_init_kernel(vc_state S) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; v < S.V; v += stride) {
        S.cov[v] = VC_INF;
        S.stamp[v] = 1;          // round 1: every vertex with an edge is active
        S.cur[v] = S.off[v];
    }
}

// Lane `lane` of a whole wave; on: it has active vertex act[i] (act NULL: vertex i, round 1).  The cursor skips covered
// other ends: a lane by itself, or -- lists of at least wave_min entries -- the wave, a ballot per 64 entries.
__device__ __forceinline__ void vc_eval(const vc_state& S, const int32_t* act, int64_t i, bool on, int lane,
                                        unsigned long long& skips, unsigned long long& evals) {
    int32_t u = 0, c = 0, end = 0;
    if (on) {
        u = act ? act[i] : (int32_t) i;
        if (!act && S.deg0[u] == 0) on = false;
    }
    if (on) {
        c = S.cur[u];
        end = S.off[u + 1];
    }
    const int32_t c0 = c;
    const bool by_wave = on && end - c >= S.wave_min;
    if (on && !by_wave)
        while (c < end && S.cov[S.ent[c].x] != VC_INF) c++;
    unsigned long long m = __ballot(by_wave);
    while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        int32_t b = __shfl(c, src, 64);
        const int32_t e = __shfl(end, src, 64);
        int32_t found = e;
        for (; b < e && found == e; b += 64 * VC_CHUNKS) {   // VC_CHUNKS x 64 entries in flight: a step is two dependent loads
            int32_t x[VC_CHUNKS];
            bool hit[VC_CHUNKS];
#pragma unroll
            for (int k = 0; k < VC_CHUNKS; k++) {
                const int32_t idx = b + 64 * k + lane;
                x[k] = idx < e ? S.ent[idx].x : -1;
            }
#pragma unroll
            for (int k = 0; k < VC_CHUNKS; k++) hit[k] = x[k] >= 0 && S.cov[x[k]] == VC_INF;   // (a self loop: uncovered while its vertex is)
#pragma unroll
            for (int k = VC_CHUNKS - 1; k >= 0; k--) {
                const unsigned long long h = __ballot(hit[k]);
                if (h) found = b + 64 * k + __builtin_ctzll(h);   // (the lowest chunk with a hit is written last)
            }
        }
        if (lane == src) c = found;
    }
    if (on) {
        const int32_t b = c < end ? c : S.low[u];
        const int2 en = S.ent[b];
        const uint32_t key = (uint32_t) S.deg0[u] + (c < end ? (uint32_t) S.deg0[en.x] : 0u);
        S.cur[u] = c;
        S.bent[u] = b;
        S.best[u] = ((unsigned long long) key << 32) | (unsigned long long) (0xffffffffu - (uint32_t) en.y);
        skips += (unsigned long long) (c - c0);
        evals++;
    }
}

// The best edge of an active vertex is picked when its other end is the vertex itself, was covered before this round, or
// has the same best edge; of two active ends the lower id records it.  Whoever records covers both ends and queues them.
__device__ __forceinline__ void vc_pick(const vc_state& S, const int32_t* act, int64_t i, bool on, int lane, int32_t r, int32_t* newq) {
    int32_t u = 0, x = 0;
    unsigned long long w = 0;
    bool rec = false, addx = false, self = false;
    if (on) {
        u = act ? act[i] : (int32_t) i;
        if (!act && S.deg0[u] == 0) on = false;
    }
    if (on) {
        x = S.ent[S.bent[u]].x;
        w = S.best[u];
        if (x == u) {
            rec = self = true;
        } else if (S.cov[x] < r) {
            rec = true;
        } else if (S.best[x] == w) {
            rec = addx = !(S.stamp[x] == r && x < u);
        }
    }
    const unsigned long long mk = __ballot(rec);
    if (!mk) return;   // (wave-uniform)
    const int leader = __builtin_ctzll(mk);
    unsigned long long at = 0;
    if (lane == leader) at = atomicAdd(&S.ctr[VC_NPICK], (unsigned long long) __popcll(mk));
    at = __shfl(at, leader, 64);
    unsigned long long len = 0;
    if (rec) {
        at += __popcll(mk & ((1ULL << lane) - 1));
        S.pickword[at] = w;
        S.pickuv[at] = make_int2(u, x);
        S.cov[u] = r;
        len = (unsigned long long) S.deg0[u];
        if (addx) {
            S.cov[x] = r;
            len += (unsigned long long) S.deg0[x];
        }
    }
    wave_append(rec, u, newq, &S.ctr[VC_NCOV], lane);
    wave_append(addx, x, newq, &S.ctr[VC_NCOV], lane);
    len = wave_sum(len);
    if (lane == 0) atomicAdd(&S.ctr[VC_MCOV], len);
    if (__ballot(self) && lane == leader) S.ctr[VC_SELF] = 1;
}

// entry `en` of the list of a newly covered vertex: its other end is active in round r if it is uncovered and its best
// edge is this one
__device__ __forceinline__ bool vc_wakes(const vc_state& S, int2 en, int32_t r) {
    const int32_t w = en.x;
    if (S.cov[w] != VC_INF) return false;
    if ((uint32_t) S.best[w] != 0xffffffffu - (uint32_t) en.y) return false;
    return atomicExch(&S.stamp[w], r) != r;
}

__device__ __forceinline__ void vc_count(const vc_state& S, int which, unsigned long long n, int lane) {
    n = wave_sum(n);
    if (lane == 0 && n) atomicAdd(&S.ctr[which], n);
}

// ------------------------------------------------------------------ grid kernels
// act[0 .. *nptr) (nptr NULL: n); launched for an upper bound of the count
__global__ void __launch_bounds__(VC_THREADS) vc_eval_kernel(vc_state S, const int32_t* act, const unsigned long long* nptr, int64_t n) {
    if (nptr) n = (int64_t) *nptr;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long skips = 0, evals = 0;
    for (int64_t base = (int64_t) blockIdx.x * blockDim.x + threadIdx.x - lane; base < n; base += stride)
        vc_eval(S, act, base + lane, base + lane < n, lane, skips, evals);
    vc_count(S, VC_SKIPS, skips, lane);
    vc_count(S, VC_EVALS, evals, lane);
}

__global__ void __launch_bounds__(VC_THREADS) vc_pick_kernel(vc_state S, const int32_t* act, const unsigned long long* nptr, int64_t n,
                                                             int32_t r, int32_t* newq) {
    if (nptr) n = (int64_t) *nptr;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t base = (int64_t) blockIdx.x * blockDim.x + threadIdx.x - lane; base < n; base += stride)
        vc_pick(S, act, base + lane, base + lane < n, lane, r, newq);
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&S.ctr[VC_ACTSUM], (unsigned long long) n);
}

// the lists of the newly covered vertices q[0 .. n), m entries in all, cut into merge-path tiles
__global__ void __launch_bounds__(BFS_THREADS) vc_activate_kernel(vc_state S, const int32_t* __restrict__ q, int64_t n,
                                                                  const int64_t* __restrict__ off, int64_t m, int32_t r, int32_t* __restrict__ act) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int64_t s_split[2][2];
    __shared__ int32_t s_win[BFS_ITEMS];
    __shared__ unsigned int s_nwin;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_nwin = 0;
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.off, q, n, off, m, s_off, s_row, [](int, int32_t, bool) {});
    unsigned long long walks = 0;
    for (int64_t x = t.e0 + tid; x < t.e1; x += BFS_THREADS) {
        const int lo = frontier_slot(s_off, nv, x);
        const int2 en = S.ent[(int64_t) s_row[lo] + (x - s_off[lo])];
        walks++;
        wave_append(vc_wakes(S, en, r), en.x, s_win, &s_nwin, tid & 63);
    }
    vc_count(S, VC_WALKS, walks, tid & 63);
    __syncthreads();
    const unsigned int nwin = s_nwin;
    if (nwin == 0) return;   // (workgroup-uniform)
    frontier_flush(s_win, nwin, &S.ctr[VC_NACT], act, &s_base);
}

// ------------------------------------------------------------------ the tail: one workgroup runs the rounds to the end
// The workgroup's waves share one CU and its L1: the barrier's workgroup-scope release / acquire makes one wave's stores
// visible to the others, and a device-scope fence (an L2 write-back per call) is not needed between the phases of a round.
__device__ __forceinline__ void vc_tail_sync() { __syncthreads(); }
__device__ __forceinline__ int64_t vc_tail_take(const vc_state& S, int which, unsigned long long* s_n) {
    vc_tail_sync();
    if (threadIdx.x == 0) *s_n = atomicExch(&S.ctr[which], 0ULL);
    vc_tail_sync();
    return (int64_t) *s_n;
}

// qa[0 .. nnew): covered in round r - 1 and not expanded yet (first: nothing has run, round r = 1 starts with every vertex).
// out[0] = rounds run here.  At most V rounds, each a bounded loop: no waiting on anybody.
__global__ void __launch_bounds__(VC_TAIL_THREADS) vc_tail_kernel(vc_state S, int32_t* act, int32_t* qa, int32_t* qb, int64_t nnew, int first,
                                                                  int32_t r, int32_t* out) {
    __shared__ unsigned long long s_n;
    const int lane = threadIdx.x & 63;
    const int64_t wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    int32_t rounds = 0;
    unsigned long long skips = 0, evals = 0, walks = 0, actsum = 0;
    for (;;) {
        int64_t nact = S.V;
        const int32_t* a = nullptr;
        if (!first) {
            for (int64_t i = wave; i < nnew; i += nwaves) {
                const int32_t v = qa[i];
                const int32_t b = S.off[v], e = S.off[v + 1];
                for (int32_t base = b; base < e; base += 64) {
                    const int32_t idx = base + lane;
                    int2 en = make_int2(0, 0);
                    bool won = false;
                    if (idx < e) {
                        en = S.ent[idx];
                        won = vc_wakes(S, en, r);
                    }
                    wave_append(won, en.x, act, &S.ctr[VC_NACT], lane);
                }
                if (lane == 0) walks += (unsigned long long) (e - b);
            }
            nact = vc_tail_take(S, VC_NACT, &s_n);
            if (nact == 0) break;
            a = act;
        }
        first = 0;
        if (threadIdx.x == 0) actsum += (unsigned long long) nact;
        for (int64_t base = threadIdx.x - lane; base < nact; base += blockDim.x) vc_eval(S, a, base + lane, base + lane < nact, lane, skips, evals);
        vc_tail_sync();
        for (int64_t base = threadIdx.x - lane; base < nact; base += blockDim.x) vc_pick(S, a, base + lane, base + lane < nact, lane, r, qb);
        nnew = vc_tail_take(S, VC_NCOV, &s_n);
        rounds++;
        r++;
        int32_t* t = qa; qa = qb; qb = t;
        if (nnew == 0) break;
    }
    vc_count(S, VC_SKIPS, skips, lane);
    vc_count(S, VC_EVALS, evals, lane);
    vc_count(S, VC_WALKS, walks, lane);
    if (threadIdx.x == 0) {
        atomicAdd(&S.ctr[VC_ACTSUM], actsum);
        out[0] = rounds;
    }
}

// ------------------------------------------------------------------ finish
__global__ void vc_key_kernel(const unsigned long long* __restrict__ word, int64_t n, unsigned long long* __restrict__ key) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < n; i += stride) key[i] = word[i] >> 32;
}

// pre[i] = sum of the keys before sorted pick i: the pick runs while 2 E - pre[i] > 0
__global__ void vc_kept_kernel(const unsigned long long* __restrict__ pre, int64_t n, unsigned long long remain0, vc_state S) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long k = 0;
    for (; i < n; i += stride) k += pre[i] < remain0 ? 1 : 0;
    vc_count(S, VC_KEPT, k, threadIdx.x & 63);
}

// the kept picks (word >= least): their slots are selected, their endpoints counted once (stamp -1)
__global__ void vc_select_kernel(vc_state S, int64_t n, unsigned long long least, uint8_t* __restrict__ select) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long c = 0;
    for (; i < n; i += stride) {
        const unsigned long long w = S.pickword[i];
        if (w < least) continue;
        select[0xffffffffu - (uint32_t) w] = 1;
        const int2 uv = S.pickuv[i];
        if (atomicExch(&S.stamp[uv.x], -1) != -1) c++;
        if (atomicExch(&S.stamp[uv.y], -1) != -1) c++;
    }
    vc_count(S, VC_COVERED, c, threadIdx.x & 63);
}

// ------------------------------------------------------------------ host
static int vc_grid(int64_t n) {
    const int64_t b = (n + VC_THREADS - 1) / VC_THREADS;
    return (int) (b < 1 ? 1 : b > 256 * 8 ? 256 * 8 : b);
}

static int vc_build_plan(const gmx_graph* g, vc_plan** out) {
    const int64_t V = g->V, E = g->E, L = 2 * E;
    hipStream_t s = 0;
    gmx_tick tick("v_cover plan");
    const double t0 = gmx_tick::now();
    vc_plan* p = new vc_plan();
    struct guard {
        vc_plan* p;
        ~guard() { delete p; }
    } gd{p};
    p->V = V;
    p->E = E;
    p->L = L;
    GMX_CHECK(p->deg0.alloc((size_t) V));
    GMX_CHECK(p->off.alloc((size_t) V + 1));
    GMX_CHECK(p->low.alloc((size_t) V));
    GMX_CHECK(p->ent.alloc((size_t) L));
    gmx_ws_scope scope;
    wbuf<uint64_t> fwd, ka, kb, va;
    if (fwd.alloc((size_t) E) || ka.alloc((size_t) L) || kb.alloc((size_t) L) || va.alloc((size_t) L)) {
        const std::string why = gmx_last_error();
        gmx_set_error("v_cover: the plan's sort buffers need %zu bytes (%lld list entries): %s", (size_t) (E + 3 * L) * sizeof(uint64_t),
                      (long long) L, why.c_str());
        return GMX_ERR_NOMEM;
    }
    hipLaunchKernelGGL(vc_degree_kernel, dim3(vc_grid(V + 1)), dim3(VC_THREADS), 0, s, (const int32_t*) g->begin.p, (const int32_t*) g->r_begin.p, V,
                       p->deg0.p, p->off.p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_keys_from_csr(g->begin.p, g->node_idx.p, V, E, false, nullptr, fwd.p, s));
    hipLaunchKernelGGL(vc_entries_kernel, dim3(vc_grid(E)), dim3(VC_THREADS), 0, s, (const uint64_t*) fwd.p, (const int32_t*) g->e_idx2idx.p,
                       (const int32_t*) p->deg0.p, E, ka.p, va.p);
    GMX_HIP(hipGetLastError());
    tick.mark("entries");
    {
        const unsigned end_bit = 32 + (unsigned) gmx_bits_for(V);
        size_t tb = 0;
        uint64_t* sorted = (uint64_t*) p->ent.p;   // x = low half = other endpoint, y = high half = slot
        GMX_HIP(rocprim::radix_sort_pairs(nullptr, tb, ka.p, kb.p, va.p, sorted, (size_t) L, 0u, end_bit, s));
        wbuf<char> tmp;
        GMX_CHECK(tmp.alloc(tb));
        GMX_HIP(rocprim::radix_sort_pairs((void*) tmp.p, tb, ka.p, kb.p, va.p, sorted, (size_t) L, 0u, end_bit, s));
    }
    tick.mark("sort");
    hipLaunchKernelGGL(vc_low_kernel, dim3(vc_grid(V * 64)), dim3(VC_THREADS), 0, s, (const int32_t*) p->off.p, (const int2*) p->ent.p, V, p->low.p);
    GMX_HIP(hipGetLastError());
    GMX_HIP(hipStreamSynchronize(s));
    tick.mark("lowest slots");
    p->build_ms = (gmx_tick::now() - t0) * 1e3;
    gd.p = nullptr;
    *out = p;
    return GMX_OK;
}

extern "C" int gmx_v_cover(gmx_graph_t* g, uint8_t* select_host, int32_t* covered, gmx_stats_t* stats) {
    GMX_REQUIRE(g && covered, "NULL argument");
    GMX_REQUIRE(select_host || g->E == 0, "select is NULL");
    if (stats) memset(stats, 0, sizeof(*stats));
    *covered = 0;
    const int64_t V = g->V, E = g->E;
    if (V == 0 || E == 0) return GMX_OK;
    if (!g->has_reverse) {
        gmx_set_error("v_cover: the graph was uploaded with GMX_GRAPH_NO_REVERSE; Deg = Degree() + InDegree() needs the reverse CSR");
        return GMX_ERR_STATE;
    }
    GMX_REQUIRE(E < (1LL << 30), "v_cover: %lld edges: the incident lists keep 32-bit offsets (below 2^30 edges)", (long long) E);
    // knobs, read at every call; the result does not depend on them
    const int64_t tail_from = gmx_env_int("GMX_VC_TAIL", VC_TAIL, 0, INT32_MAX);
    const int64_t wave_min = gmx_env_int("GMX_VC_WAVE", VC_WAVE, 0, INT32_MAX);
    bool built = false;
    if (!g->vc_cache) {
        GMX_CHECK(vc_build_plan(g, &g->vc_cache));
        built = true;
    }
    const vc_plan* p = g->vc_cache;

    dbuf<int32_t> cov, stamp, cur, bent, act, q0, q1, tail_out;
    dbuf<unsigned long long> best, pickword, ctr;
    dbuf<int2> pickuv;
    dbuf<uint8_t> select;
    frontier_scan fs;
    gmx_pinned<unsigned long long> h_ctr;
    GMX_CHECK(cov.alloc((size_t) V));
    GMX_CHECK(stamp.alloc((size_t) V));
    GMX_CHECK(cur.alloc((size_t) V));
    GMX_CHECK(bent.alloc((size_t) V));
    GMX_CHECK(act.alloc((size_t) V));
    GMX_CHECK(q0.alloc((size_t) V));
    GMX_CHECK(q1.alloc((size_t) V));
    GMX_CHECK(tail_out.alloc(1));
    GMX_CHECK(best.alloc((size_t) V));
    GMX_CHECK(pickword.alloc((size_t) V));
    GMX_CHECK(pickuv.alloc((size_t) V));
    GMX_CHECK(ctr.alloc(VC_NCTR));
    GMX_CHECK(select.alloc((size_t) E));
    GMX_CHECK(gmx_frontier_scan_alloc(&fs, (size_t) V, 0));
    GMX_CHECK(h_ctr.alloc(VC_NCTR));
    gmx_spans tm;

    vc_state S;
    S.deg0 = p->deg0.p;
    S.off = p->off.p;
    S.low = p->low.p;
    S.ent = p->ent.p;
    S.cov = cov.p;
    S.stamp = stamp.p;
    S.cur = cur.p;
    S.bent = bent.p;
    S.best = best.p;
    S.pickword = pickword.p;
    S.pickuv = pickuv.p;
    S.ctr = ctr.p;
    S.V = V;
    S.wave_min = (int32_t) wave_min;
    unsigned long long* h = h_ctr.p;

    GMX_CHECK(tm.begin(tm.KERNEL));
    const double t_start = gmx_tick::now();
    GMX_HIP(hipMemsetAsync(ctr.p, 0, VC_NCTR * sizeof(unsigned long long), 0));
    GMX_HIP(hipMemsetAsync(select.p, 0, (size_t) E, 0));
    hipLaunchKernelGGL(vc_init_kernel, dim3(vc_grid(V)), dim3(VC_THREADS), 0, 0, S);
    GMX_HIP(hipGetLastError());
    int32_t* qa = q0.p;   // covered in the last round, not expanded yet
    int32_t* qb = q1.p;
    int32_t round = 0, tail_rounds = 0;
    int64_t last_active = V, ncov = 0, mcov = 0;
    unsigned long long actsum = 0;
    double tail_ms = 0;
    for (;;) {
        const bool first = round == 0;
        if (tail_from > 0 && last_active <= tail_from) {   // the rest in one workgroup
            const double t_tail0 = gmx_tick::now();
            GMX_HIP(hipMemsetAsync(&ctr.p[VC_NACT], 0, 3 * sizeof(unsigned long long), 0));   // the tail claims its lists from zero
            hipLaunchKernelGGL(vc_tail_kernel, dim3(1), dim3(VC_TAIL_THREADS), 0, 0, S, act.p, qa, qb, ncov, first ? 1 : 0, round + 1, tail_out.p);
            GMX_HIP(hipGetLastError());
            GMX_HIP(hipMemcpy(&tail_rounds, tail_out.p, sizeof(int32_t), hipMemcpyDeviceToHost));
            GMX_CHECK(gmx_read_back(h_ctr, ctr.p, VC_NCTR));
            tail_ms = (gmx_tick::now() - t_tail0) * 1e3;
            break;
        }
        const unsigned long long* nptr = nullptr;
        int64_t bound = V;
        if (!first) {
            GMX_HIP(hipMemsetAsync(&ctr.p[VC_NACT], 0, 3 * sizeof(unsigned long long), 0));   // VC_NACT, VC_NCOV, VC_MCOV
            GMX_CHECK(gmx_frontier_offsets(p->off.p, qa, ncov, &fs, nullptr, false));
            const int64_t nb = frontier_tiles(ncov, mcov);
            hipLaunchKernelGGL(vc_activate_kernel, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, S, (const int32_t*) qa, ncov,
                               (const int64_t*) fs.off.p, mcov, round + 1, act.p);
            GMX_HIP(hipGetLastError());
            nptr = &ctr.p[VC_NACT];
            bound = mcov < V ? mcov : V;   // a walked entry wakes at most one vertex
        }
        const int32_t* a = first ? nullptr : act.p;
        hipLaunchKernelGGL(vc_eval_kernel, dim3(vc_grid(bound)), dim3(VC_THREADS), 0, 0, S, a, nptr, V);
        hipLaunchKernelGGL(vc_pick_kernel, dim3(vc_grid(bound)), dim3(VC_THREADS), 0, 0, S, a, nptr, V, round + 1, qb);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctr, ctr.p, VC_NCTR));
        last_active = (int64_t) (h[VC_ACTSUM] - actsum);
        actsum = h[VC_ACTSUM];
        if (last_active == 0) break;   // nothing woke up: the round did not take place
        round++;
        ncov = (int64_t) h[VC_NCOV];
        mcov = (int64_t) h[VC_MCOV];
        int32_t* t = qa; qa = qb; qb = t;
        if (ncov == 0) break;
    }
    const double t_rounds = gmx_tick::now();
    const int64_t picks = (int64_t) h[VC_NPICK];
    // finish: only self-loop picks take more from `remain` than from the degree sum, so without one nothing is cut
    int64_t kept = picks;
    unsigned long long least = 0;
    if (h[VC_SELF] && picks > 0) {
        gmx_ws_scope scope;
        wbuf<unsigned long long> wa, wb, key, pre;
        wbuf<char> tmp, tmp2;
        GMX_CHECK(wa.alloc((size_t) picks));
        GMX_CHECK(wb.alloc((size_t) picks));
        GMX_CHECK(key.alloc((size_t) picks));
        GMX_CHECK(pre.alloc((size_t) picks));
        GMX_HIP(hipMemcpyAsync(wa.p, pickword.p, sizeof(unsigned long long) * (size_t) picks, hipMemcpyDeviceToDevice, 0));
        rocprim::double_buffer<unsigned long long> db(wa.p, wb.p);
        size_t tb = 0;
        GMX_HIP(rocprim::radix_sort_keys_desc(nullptr, tb, db, (size_t) picks, 0u, 64u, 0));
        GMX_CHECK(tmp.alloc(tb));
        GMX_HIP(rocprim::radix_sort_keys_desc((void*) tmp.p, tb, db, (size_t) picks, 0u, 64u, 0));
        const unsigned long long* sorted = db.current();
        hipLaunchKernelGGL(vc_key_kernel, dim3(vc_grid(picks)), dim3(VC_THREADS), 0, 0, sorted, picks, key.p);
        GMX_HIP(hipGetLastError());
        size_t sb = 0;
        GMX_HIP(rocprim::exclusive_scan(nullptr, sb, key.p, pre.p, 0ULL, (size_t) picks, rocprim::plus<unsigned long long>(), 0));
        GMX_CHECK(tmp2.alloc(sb));
        GMX_HIP(rocprim::exclusive_scan((void*) tmp2.p, sb, key.p, pre.p, 0ULL, (size_t) picks, rocprim::plus<unsigned long long>(), 0));
        hipLaunchKernelGGL(vc_kept_kernel, dim3(vc_grid(picks)), dim3(VC_THREADS), 0, 0, (const unsigned long long*) pre.p, picks,
                           2ULL * (unsigned long long) E, S);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctr, ctr.p, VC_NCTR));
        kept = (int64_t) h[VC_KEPT];   // (the sums never fall: the kept picks are the first `kept` of the order; at least one)
        GMX_HIP(hipMemcpy(&least, sorted + (kept - 1), sizeof(least), hipMemcpyDeviceToHost));
    }
    if (picks > 0) {
        hipLaunchKernelGGL(vc_select_kernel, dim3(vc_grid(picks)), dim3(VC_THREADS), 0, 0, S, picks, least, select.p);
        GMX_HIP(hipGetLastError());
    }
    GMX_CHECK(gmx_read_back(h_ctr, ctr.p, VC_NCTR));
    GMX_CHECK(tm.end(tm.KERNEL));
    const double t_finish = gmx_tick::now();
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(select_host, select.p, (size_t) E, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));
    *covered = (int32_t) h[VC_COVERED];
    if (stats) {
        stats->iterations = round + tail_rounds;
        stats->edges_examined = (int64_t) (h[VC_SKIPS] + h[VC_EVALS] + h[VC_WALKS]);
        stats->vertices_reached = (int64_t) h[VC_COVERED];
        stats->edges_reached = kept;
    }
    if (getenv("GMX_VC_LOG"))   // one line per call (tools/vc_prof.py and the tests parse it)
        fprintf(stderr, "gmx v_cover: plan %s build_ms %.3f V %lld E %lld L %lld; tail %lld wave %lld; rounds %d grid + %d tail; picks %lld kept %lld "
                        "covered %llu; skips %llu evals %llu walks %llu; ms %.3f grid + %.3f tail + %.3f finish\n",
                built ? "built" : "reused", built ? p->build_ms : 0.0, (long long) V, (long long) E, (long long) p->L, (long long) tail_from,
                (long long) wave_min, round, tail_rounds, (long long) picks, (long long) kept, h[VC_COVERED], h[VC_SKIPS], h[VC_EVALS], h[VC_WALKS],
                (t_rounds - t_start) * 1e3 - tail_ms, tail_ms, (t_finish - t_rounds) * 1e3);
    return GMX_OK;
}

void gmx_touch_vcover() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) vc_tail_kernel);
}
