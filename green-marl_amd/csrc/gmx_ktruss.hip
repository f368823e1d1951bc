// gmx_ktruss.hip -- per-edge triangle support and k-truss decomposition on gfx950: gmx_ktruss.  The reference has no such
// program; the definition, the schedule that fixes truss[] and the statistics are the contract at gmx_ktruss in gmx.h.
//
// The stored slots are read as gmx_clustering reads them, N(v) = { u != v : v -> u or u -> v is stored }, on the plan of
// gmx_tcd.hip (cached on the graph, shared with gmx_triangle_counting_directed and gmx_clustering): perm and UP', every
// undirected edge once in sorted rows.  The position of an edge in up_idx is its EDGE ID.  On the first call the plan gets
// (tcd_plan_adjacency in gmx_tcd.hip, which gmx_squares calls as well)
//   adjacency  nb_begin / nb_idx / nb_eid: row v = DOWN'(v) then UP'(v), which is sorted as it stands (all of DOWN' < v < all
//              of UP'), with the edge id of every slot.  The id of an upper slot is its own position; the lower slots come
//              from ONE stable sort of (w, position) over up_idx: the run of w lists the edges (x, w) by ascending x.
//   up_src     the lower end of every edge id (its row in UP').
//   support    one work item per edge id {a, b}: the shorter of the two rows is walked (ties: a, the lower plan id), the
//              longer one binary-searched.  A row of up to KT_LANE slots is walked by the edge's lane, a longer one by the
//              wave, 64 slots a step.  No atomics: sup[e] is written once.
//   peeling    gmx_kcore.hip's discipline on edges.  One word sup[e] that only falls, by atomic decrements of 1, so every
//              value is returned to exactly one decrement; rem[e] = KT_LIVE, or the round that removes e.
//     level    s = the smallest sup of a live edge (kt_min_kernel over the live list); kt_scan_kernel drops the entries
//              that are no longer live, stamps and queues sup <= s, keeps the rest.
//     round    the queue segment [qs, qe) holds the edges stamped `round`.  A queue entry is the end with the shorter row;
//              the rows go through the merge-path tile (gmx_frontier.h), one item per slot x of the row: e1 = {end, x} from
//              the slot, e2 = {other end, x} by binary search.  The triangle still exists when neither was stamped with an
//              earlier round.  Both stamped `round`: nothing.  Only e1: e2 is decremented iff id(e) < id(e1) (the mirror
//              image for e2).  Neither: both.  So every vanishing triangle decrements each surviving edge exactly once, and
//              the decrement that returns s + 1 stamps the edge round + 1 and appends it.  An edge is queued once in the
//              whole run: q_e[] / q_v[] hold every round's segment behind the other.
// The schedule does not depend on the order of the decrements: the number of decrements an edge takes in a round is fixed
// by the stamps at the round's start (a stamp written during the round is round + 1 and reads like KT_LIVE: "not earlier,
// not this round"), so whether it reaches s in the round is too; truss, the stamps and the segment bounds follow from that.
//     tail     while the queue's rows hold at most GMX_KTRUSS_TAIL slots (and, at a level's start, the list at most as many
//              entries) one workgroup runs rounds and level scans with a barrier between them, a wave per queue entry, and
//              hands back otherwise.
// Rounds are separated by a kernel boundary or, in the tail, by a barrier.
#include "gmx_tcd_plan.h"
#include "gmx_rowgroup.h"
#include "gmx_frontier.h"

#define KT_THREADS BFS_THREADS
#define KT_LANE 16           // support: a lane walks a shorter row of up to this many slots by itself.  NOT MEASURED
#define KT_TAIL_THREADS 1024
#define KT_TAIL 1024         // GMX_KTRUSS_TAIL: the tail launch takes over while the queue to expand holds at most this many row slots.
                             // Taken over from gmx_kcore.hip's KC_TAIL; swept on RMAT-20 and the 1024 x 1024 grid:
                             // 0 .. 4096 flat on RMAT-20 (30 of 2254 rounds), 0 .. 1024 within 6 % on the grid, 16384: 3 x there
#define KT_LIVE 0x7f7f7f7f   // rem[e]: not queued -- above every round (at most |UP'| < 2^30 of them), and one memset
#define KT_NONE 0xFFFFFFFFu  // the minimum over no edge

typedef unsigned long long kt_word;

struct kt_ctl {
    kt_word qtail;       // tail of q_e[] / q_v[]: edges removed so far
    kt_word slots;       // slots of the shorter rows of q[0, qtail)
    kt_word nkeep;       // tail of the list the scan writes
    kt_word sum_sup;     // the sum of the supports: 3 x triangles
    unsigned int maxdec, pad0;
    // what the tail hands back
    long long t_qs, t_qe, t_nlist, t_levels, t_rounds, t_scanned, t_level_q0, t_m;
    int32_t t_s, t_state, t_swapped, t_pad;
    kt_word pad1[1];
    struct {
        unsigned int minsup;
        unsigned int pad[31];
    } shard[BFS_SHARDS];
};

enum { KT_DONE = 0, KT_BOUNDARY = 1, KT_MIDLEVEL = 2 };

struct kt_state {
    const int32_t* nb_begin;
    const int32_t* nb_idx;
    const int32_t* nb_eid;
    const int32_t* up_src;
    const int32_t* up_idx;
    int32_t* sup;
    int32_t* rem;
    int32_t* truss;
    int32_t* q_e;
    int32_t* q_v;
    kt_ctl* ctl;
    int64_t U;   // |UP'|: the queue's capacity
};

__device__ __forceinline__ int32_t kt_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int kt_shard() { return (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (BFS_SHARDS - 1); }

// ------------------------------------------------------------------ support
// the shorter row of edge {a, b}, a < b (ties: a), as [*sb, *se), and the longer one as [*lb, *le)
__device__ __forceinline__ void kt_rows(const int32_t* __restrict__ nb_begin, int32_t a, int32_t b, int32_t* sb, int32_t* se, int32_t* lb, int32_t* le) {
    const int32_t ab = nb_begin[a], ae = nb_begin[a + 1], bb = nb_begin[b], be = nb_begin[b + 1];
    const bool a_short = ae - ab <= be - bb;
    *sb = a_short ? ab : bb;
    *se = a_short ? ae : be;
    *lb = a_short ? bb : ab;
    *le = a_short ? be : ae;
}

// a wave takes 64 edge ids at a time, a lane each
__global__ void __launch_bounds__(KT_THREADS) kt_support_kernel(const int32_t* __restrict__ nb_begin, const int32_t* __restrict__ nb_idx,
                                                                const int32_t* __restrict__ up_src, const int32_t* __restrict__ up_idx, int64_t U, int lane_max,
                                                                int32_t* __restrict__ sup) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t) blockIdx.x * (KT_THREADS / 64) + (threadIdx.x >> 6), nwaves = (int64_t) gridDim.x * (KT_THREADS / 64);
    for (int64_t base = wave * 64; base < U; base += nwaves * 64) {   // (wave-uniform)
        const int64_t e = base + lane;
        const bool have = e < U;
        int32_t sb = 0, se = 0, lb = 0, le = 0;
        if (have) kt_rows(nb_begin, up_src[e], up_idx[e], &sb, &se, &lb, &le);
        const bool by_wave = se - sb > lane_max;
        int32_t cnt = 0;
        if (!by_wave)
            for (int32_t p = sb; p < se; p++) cnt += rg_contains<false>(nb_idx, lb, le, nb_idx[p]) ? 1 : 0;
        unsigned long long m = __ballot(by_wave);
        while (m) {   // the long rows, one after the other by the whole wave: the same trip counts in every lane
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t wsb = __shfl(sb, src, 64), wse = __shfl(se, src, 64), wlb = __shfl(lb, src, 64), wle = __shfl(le, src, 64);
            int32_t c = 0;
            for (int32_t p0 = wsb; p0 < wse; p0 += 64) {
                const int32_t p = p0 + lane;
                const bool hit = p < wse && rg_contains<false>(nb_idx, wlb, wle, nb_idx[p]);
                c += (int32_t) __popcll(__ballot(hit));
            }
            if (lane == src) cnt = c;
        }
        if (have) sup[e] = cnt;
    }
}

__global__ void __launch_bounds__(KT_THREADS) kt_sum_kernel(const int32_t* __restrict__ sup, int64_t U, kt_ctl* __restrict__ ctl) {
    kt_word n = 0;
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < U; e += (int64_t) gridDim.x * blockDim.x) n += (kt_word) sup[e];
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ctl->sum_sup, n);
}

// ------------------------------------------------------------------ peeling
// the smallest sup among the live edges of list[0, n) (list == NULL: the edges 0 .. n-1) into the sharded words
__global__ void __launch_bounds__(KT_THREADS) kt_min_kernel(kt_state S, const int32_t* __restrict__ list, int64_t n) {
    unsigned int mn = KT_NONE;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const int32_t e = list ? list[i] : (int32_t) i;
        if (S.rem[e] == KT_LIVE) mn = min(mn, (unsigned int) S.sup[e]);
    }
    mn = wave_min(mn);
    if ((threadIdx.x & 63) == 0 && mn != KT_NONE) atomicMin(&S.ctl->shard[kt_shard()].minsup, mn);
}

// the workgroup's LDS list of edge ids goes to the queue: thread 0 claims the tail once, everybody writes the edge and the
// end with the shorter row (ties: the lower plan id, as the support kernel walks), and the rows' slots are added up.
// Called by the whole workgroup after the barrier that completes s_list.
__device__ __forceinline__ void kt_flush(const kt_state& S, const int32_t* s_list, unsigned int cnt, kt_word* s_base) {
    if (threadIdx.x == 0 && cnt) *s_base = atomicAdd(&S.ctl->qtail, (kt_word) cnt);
    __syncthreads();
    kt_word len = 0;
    for (unsigned int i = threadIdx.x; i < cnt; i += KT_THREADS) {
        if ((int64_t) (*s_base + i) >= S.U) break;   // (an edge is queued once: never taken; the host then sees qtail != U)
        const int32_t t = s_list[i], a = S.up_src[t], b = S.up_idx[t];
        const int32_t la = S.nb_begin[a + 1] - S.nb_begin[a], lb = S.nb_begin[b + 1] - S.nb_begin[b];
        S.q_e[*s_base + i] = t;
        S.q_v[*s_base + i] = la <= lb ? a : b;
        len += (kt_word) (la <= lb ? la : lb);
    }
    len = wave_sum(len);
    if ((threadIdx.x & 63) == 0 && len) atomicAdd(&S.ctl->slots, len);
}

// list[0, n) -> dropped (stamped by a round of the level before), queued (sup <= s: truss s + 2, stamp `round`) or kept
__global__ void __launch_bounds__(KT_THREADS) kt_scan_kernel(kt_state S, const int32_t* __restrict__ list, int64_t n, int32_t s, int32_t round,
                                                             int32_t* __restrict__ out) {
    __shared__ int32_t s_keep[BFS_ITEMS], s_q[BFS_ITEMS];
    __shared__ unsigned int s_nkeep, s_nq;
    __shared__ kt_word s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t t0 = (int64_t) blockIdx.x * BFS_ITEMS; t0 < n; t0 += (int64_t) gridDim.x * BFS_ITEMS) {
        if (tid == 0) s_nkeep = s_nq = 0;
        __syncthreads();
        for (int j = 0; j < BFS_ITEMS / KT_THREADS; j++) {
            const int64_t i = t0 + j * KT_THREADS + tid;
            const int32_t e = i < n ? (list ? list[i] : (int32_t) i) : 0;
            const bool live = i < n && S.rem[e] == KT_LIVE;
            const int32_t d = live ? S.sup[e] : 0;
            wave_append(live && d <= s, e, s_q, &s_nq, lane, [&] {
                S.rem[e] = round;
                S.truss[e] = s + 2;
            });
            wave_append(live && d > s, e, s_keep, &s_nkeep, lane);
        }
        __syncthreads();
        frontier_flush(s_keep, s_nkeep, &S.ctl->nkeep, out, &s_base);
        __syncthreads();
        kt_flush(S, s_q, s_nq, &s_base);
        __syncthreads();
    }
}

// the slot (w, e1 = {end, w}) of the walked row of queued edge e, whose other end is o: *t1, *t2 = the edges to decrement
// (or -1).  e2 = {o, w} by binary search; the triangle was still there when the round began if neither carries an earlier
// stamp (a stamp written during the round is round + 1)
__device__ __forceinline__ void kt_triangle(const kt_state& S, int32_t e, int32_t o, int32_t w, int32_t e1, int32_t round, int32_t* t1, int32_t* t2) {
    if (w == o) return;
    const int32_t ob = S.nb_begin[o], oe = S.nb_begin[o + 1];
    const int32_t f = rg_lower_bound<false>(S.nb_idx, ob, oe, w);
    if (f >= oe || S.nb_idx[f] != w) return;
    const int32_t e2 = S.nb_eid[f];
    const int32_t r1 = kt_load(&S.rem[e1]), r2 = kt_load(&S.rem[e2]);
    if (r1 < round || r2 < round) return;
    const bool in1 = r1 == round, in2 = r2 == round;
    if (!in1 && !in2) {
        *t1 = e1;
        *t2 = e2;
    } else if (in1 && !in2) {
        if (e < e1) *t2 = e2;
    } else if (in2 && !in1) {
        if (e < e2) *t1 = e1;
    }
}

// a round: one merge-path tile of the shorter rows of the queue segment qv[0, n) / qe[0, n), stamped `round`, at level s.
// LDS: the tile's rows (8 + 4 + 4 + 4 bytes each) and the list of what it queues, two edges per item at most: 56 KiB, two
// workgroups per CU.  NOT MEASURED against a list in memory.
__global__ void __launch_bounds__(KT_THREADS) kt_round_kernel(kt_state S, const int32_t* __restrict__ qv, const int32_t* __restrict__ qe, int64_t n,
                                                              const int64_t* __restrict__ off, int64_t m, int32_t s, int32_t round) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_e[BFS_ITEMS + 2];   // the row's edge ...
    __shared__ int32_t s_o[BFS_ITEMS + 2];   // ... and its other end
    __shared__ int32_t s_list[2 * BFS_ITEMS];
    __shared__ int64_t s_split[2][2];
    __shared__ unsigned int s_n;
    __shared__ kt_word s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_n = 0;
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.nb_begin, qv, n, off, m, s_off, s_row, [&](int i, int32_t v, bool in_range) {
        const int32_t e = in_range ? qe[t.v0 + i] : 0;
        const int32_t a = in_range ? S.up_src[e] : 0;
        s_e[i] = e;
        s_o[i] = in_range ? (a == v ? S.up_idx[e] : a) : 0;
    });
    if (t.e1 <= t.e0) return;   // (workgroup-uniform)
    for (int j = 0; j < BFS_ITEMS / KT_THREADS; j++) {
        const int64_t x = t.e0 + tid + (int64_t) j * KT_THREADS;
        int32_t t1 = -1, t2 = -1;   // the edges this item decrements
        if (x < t.e1) {
            const int lo = frontier_slot(s_off, nv, x);
            const int64_t p = (int64_t) s_row[lo] + (x - s_off[lo]);
            const int32_t w = S.nb_idx[p], e1 = S.nb_eid[p], e = s_e[lo], o = s_o[lo];
            kt_triangle(S, e, o, w, e1, round, &t1, &t2);
        }
        const bool last1 = t1 >= 0 && atomicSub(&S.sup[t1], 1) == s + 1;
        const bool last2 = t2 >= 0 && atomicSub(&S.sup[t2], 1) == s + 1;
        wave_append(last1, t1, s_list, &s_n, lane, [&] {
            S.rem[t1] = round + 1;
            S.truss[t1] = s + 2;
        });
        wave_append(last2, t2, s_list, &s_n, lane, [&] {
            S.rem[t2] = round + 1;
            S.truss[t2] = s + 2;
        });
    }
    __syncthreads();
    kt_flush(S, s_list, s_n, &s_base);
}

// ---- the tail: one workgroup goes on from the host's state -- the list la[0, nlist) (identity: the edge ids themselves), the
// level s, the queue segment [qs, qe) of round `round` whose shorter rows hold m slots -- until no edge is live (KT_DONE), a
// level would start on a list of more than tail_from entries (KT_BOUNDARY) or a queue's rows hold more than tail_from slots
// (KT_MIDLEVEL).  sup[] and rem[] are read with agent-scope loads: sup's values come from atomics, and the level scan must
// see them as they are.  The queue, the lists and truss are plain stores of this workgroup, read behind its barrier.
// Every lane of the wave must be in kt_tail_append; the appending lanes stamp and place their edge.
__device__ __forceinline__ void kt_tail_append(const kt_state& S, bool on, int32_t t, int32_t stamp, int32_t truss, unsigned int* s_tail, kt_word* s_m,
                                               int lane) {
    const unsigned long long mk = __ballot(on);
    if (!mk) return;
    const int leader = __ffsll((long long) mk) - 1;
    unsigned int at = 0;
    if (lane == leader) at = atomicAdd(s_tail, (unsigned int) __popcll(mk));
    at = __shfl(at, leader, 64);
    if (on) {
        const unsigned int i = at + (unsigned int) __popcll(mk & ((1ULL << lane) - 1));
        const int32_t a = S.up_src[t], b = S.up_idx[t];
        const int32_t la = S.nb_begin[a + 1] - S.nb_begin[a], lb = S.nb_begin[b + 1] - S.nb_begin[b];
        S.rem[t] = stamp;
        S.truss[t] = truss;
        if ((int64_t) i < S.U) {   // (an edge is queued once: always)
            S.q_e[i] = t;
            S.q_v[i] = la <= lb ? a : b;
        }
        atomicAdd(s_m, (kt_word) (la <= lb ? la : lb));
    }
}

__global__ void __launch_bounds__(KT_TAIL_THREADS) kt_tail_kernel(kt_state S, int32_t* la, int32_t* lb, int identity, int64_t nlist, int32_t s, int32_t round,
                                                                  int64_t qs, int64_t qe, int64_t level_q0, int64_t m, int64_t tail_from) {
    __shared__ unsigned int s_tail, s_keep, s_min;
    __shared__ kt_word s_m;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = KT_TAIL_THREADS >> 6;
    if (tid == 0) {
        s_tail = (unsigned int) qe;
        s_keep = 0;
        s_min = KT_NONE;
        s_m = 0;
    }
    __syncthreads();
    kt_word tot = 0;   // slots of the shorter rows of what this launch queued
    long long levels = 0, rounds = 0, scanned = 0;
    int swapped = 0, state = KT_DONE;
    for (;;) {   // a level removes at least one edge and a round has a queue that is not empty: the loop ends
        if (qs == qe) {   // a level starts (everything here is workgroup-uniform)
            if (nlist == 0) break;
            if (nlist > tail_from) {
                state = KT_BOUNDARY;
                break;
            }
            unsigned int mn = KT_NONE;
            for (int64_t i = tid; i < nlist; i += KT_TAIL_THREADS) {
                const int32_t e = identity ? (int32_t) i : la[i];
                if (kt_load(&S.rem[e]) == KT_LIVE) mn = min(mn, (unsigned int) kt_load(&S.sup[e]));
            }
            mn = wave_min(mn);
            if (lane == 0 && mn != KT_NONE) atomicMin(&s_min, mn);
            __syncthreads();
            const unsigned int snew = s_min;
            if (snew == KT_NONE) {   // every entry was removed by the last rounds
                nlist = 0;
                break;
            }
            for (int64_t base = tid - lane; base < nlist; base += KT_TAIL_THREADS) {   // (wave-uniform trip count)
                const int64_t i = base + lane;
                const int32_t e = i < nlist ? (identity ? (int32_t) i : la[i]) : 0;
                const bool live = i < nlist && kt_load(&S.rem[e]) == KT_LIVE;
                const int32_t d = live ? kt_load(&S.sup[e]) : 0;
                kt_tail_append(S, live && d <= (int32_t) snew, e, round, (int32_t) snew + 2, &s_tail, &s_m, lane);
                wave_append(live && d > (int32_t) snew, e, lb, &s_keep, lane);
            }
            __syncthreads();
            levels++;
            scanned += nlist;
            nlist = (int64_t) s_keep;
            s = (int32_t) snew;
            level_q0 = qs;
            int32_t* x = la; la = lb; lb = x;
            swapped ^= 1;
            identity = 0;
        } else {   // a round: a wave per queue entry, 64 slots of its shorter row a step
            if (m > tail_from) {
                state = KT_MIDLEVEL;
                break;
            }
            for (int64_t i = qs + wave; i < qe; i += nwaves) {
                const int32_t e = S.q_e[i], v = S.q_v[i];
                const int32_t a = S.up_src[e], o = a == v ? S.up_idx[e] : a;
                const int32_t rb = S.nb_begin[v], re = S.nb_begin[v + 1];
                for (int32_t p0 = rb; p0 < re; p0 += 64) {
                    const int32_t p = p0 + lane;
                    int32_t t1 = -1, t2 = -1;
                    if (p < re) kt_triangle(S, e, o, S.nb_idx[p], S.nb_eid[p], round, &t1, &t2);
                    const bool last1 = t1 >= 0 && atomicSub(&S.sup[t1], 1) == s + 1;
                    const bool last2 = t2 >= 0 && atomicSub(&S.sup[t2], 1) == s + 1;
                    kt_tail_append(S, last1, t1, round + 1, s + 2, &s_tail, &s_m, lane);
                    kt_tail_append(S, last2, t2, round + 1, s + 2, &s_tail, &s_m, lane);
                }
            }
            __syncthreads();
            rounds++;
            round++;
            qs = qe;
        }
        // behind either step's barrier: the queue's new end and the slots of its rows
        qe = (int64_t) s_tail;
        m = (int64_t) s_m;
        tot += (kt_word) m;
        __syncthreads();
        if (tid == 0) {
            s_keep = 0;
            s_min = KT_NONE;
            s_m = 0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        kt_ctl* c = S.ctl;
        c->qtail = (kt_word) s_tail;
        c->slots += tot;
        c->t_qs = qs;
        c->t_qe = qe;
        c->t_nlist = nlist;
        c->t_levels = levels;
        c->t_rounds = rounds;
        c->t_scanned = scanned;
        c->t_level_q0 = level_q0;
        c->t_m = m;
        c->t_s = s;
        c->t_state = state;
        c->t_swapped = swapped;
    }
}

// the largest number of decrements one edge received (GMX_KTRUSS_PHASES)
__global__ void __launch_bounds__(KT_THREADS) kt_maxdec_kernel(const int32_t* __restrict__ sup0, const int32_t* __restrict__ sup, int64_t U,
                                                               kt_ctl* __restrict__ ctl) {
    int32_t mx = 0;
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < U; e += (int64_t) gridDim.x * blockDim.x) mx = max(mx, sup0[e] - sup[e]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctl->maxdec, (unsigned int) mx);
}

// ------------------------------------------------------------------ finish
// one thread per device slot u -> w: the edge id of {perm[u], perm[w]} is its position in UP', and the values go to the
// UPLOADED slot (order[i], or i); a self-loop slot gets 0.  Only the arrays asked for are written.
__global__ void __launch_bounds__(KT_THREADS) kt_finish_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx,
                                                               const int32_t* __restrict__ order, int64_t V, int64_t E,
                                                               const int32_t* __restrict__ perm /* NULL: identity */, const int32_t* __restrict__ up_begin,
                                                               const int32_t* __restrict__ up_idx, const int32_t* __restrict__ sup0,
                                                               const int32_t* __restrict__ truss, int32_t* __restrict__ sup_out, int32_t* __restrict__ truss_out) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (int64_t) gridDim.x * blockDim.x) {
        const int32_t u = csr_row_of(begin, V, (uint32_t) i), w = idx[i];
        const int64_t dst = order ? order[i] : i;
        int32_t sv = 0, tv = 0;
        if (u != w) {
            const int32_t pu = perm ? perm[u] : u, pw = perm ? perm[w] : w;
            const int32_t a = pu < pw ? pu : pw, b = pu < pw ? pw : pu;
            const int32_t e = rg_lower_bound<false>(up_idx, up_begin[a], up_begin[a + 1], b);   // (there: {a, b} is an edge)
            sv = sup0[e];
            if (truss_out) tv = truss[e];
        }
        if (sup_out) sup_out[dst] = sv;
        if (truss_out) truss_out[dst] = tv;
    }
}

// ------------------------------------------------------------------ host
// sup[e] = the triangles on edge id e, for every entry on a plan that has its adjacency (gmx_tcd_plan.h); enqueued on stream 0
int kt_support_into(tcd_plan* p, int32_t* sup) {
    hipLaunchKernelGGL(kt_support_kernel, dim3(grid_for(p->E_up)), dim3(KT_THREADS), 0, 0, (const int32_t*) p->nb_begin.p, (const int32_t*) p->nb_idx.p,
                       (const int32_t*) p->up_src.p, (const int32_t*) p->up_idx.p, p->E_up, KT_LANE, sup);
    GMX_HIP(hipGetLastError());
    return GMX_OK;
}

extern "C" int gmx_ktruss(gmx_graph_t* g, int32_t* truss_host, int32_t* support_host, int32_t* max_truss, int64_t* num_edges, gmx_stats_t* stats_out) {
    GMX_REQUIRE(max_truss, "NULL max_truss");
    GMX_REQUIRE(g, "NULL graph");
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    *max_truss = 0;
    if (num_edges) *num_edges = 0;
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    // knobs, read at every call; no result byte depends on them
    const bool ordered = !getenv("GMX_KTRUSS_NO_ORDER");
    const bool phase_log = getenv("GMX_KTRUSS_PHASES") != nullptr;
    const bool peel = truss_host != nullptr;
    const int64_t tail_from = gmx_env_int("GMX_KTRUSS_TAIL", KT_TAIL, 0, INT64_MAX);
    // E = 0 or self loops only: zero arrays, answered without a plan
    int64_t real = 0;
    GMX_CHECK(tcd_real_slots(g, &real));
    if (real == 0) {
        if (truss_host) memset(truss_host, 0, (size_t) E * sizeof(int32_t));
        if (support_host) memset(support_host, 0, (size_t) E * sizeof(int32_t));
        return GMX_OK;
    }
    // graph preprocessing (cached on the graph, shared with gmx_triangle_counting_directed and gmx_clustering; outside the timed region)
    bool built = false;
    tcd_plan* p = nullptr;
    GMX_CHECK(tcd_plan_get(g, ordered, &p, &built));
    const int64_t U = p->E_up;
    if (num_edges) *num_edges = U;
    float ph_ms[6] = {0, 0, 0, 0, 0, 0};   // plan additions, support, level scans, grid rounds, finish, tail launches (GMX_KTRUSS_PHASES)
    gmx_phase_clock phase;
    GMX_CHECK(phase.enable(phase_log));
    const bool adj_built = !p->kt_ready;
    phase.begin();
    GMX_CHECK(tcd_plan_adjacency(p));
    phase.end(&ph_ms[0]);
    if (!truss_host && !support_host) return GMX_OK;   // only *num_edges was asked for

    // the call's scratch: per edge id, and the arrays asked for by slot
    dbuf<int32_t> sup0, sup, rem, truss, q_e, q_v, l0, l1, sup_out, truss_out;
    dbuf<kt_ctl> ctl;
    const size_t scratch = (size_t) U * 4 * (peel ? 8 : 1) + (size_t) E * 4 * ((truss_host ? 1 : 0) + (support_host ? 1 : 0)) + sizeof(kt_ctl);
    bool failed = sup0.alloc((size_t) U) || ctl.alloc(1) || (support_host && sup_out.alloc((size_t) E)) || (truss_host && truss_out.alloc((size_t) E));
    if (!failed && peel)
        failed = sup.alloc((size_t) U) || rem.alloc((size_t) U) || truss.alloc((size_t) U) || q_e.alloc((size_t) U) || q_v.alloc((size_t) U) ||
                 l0.alloc((size_t) U) || l1.alloc((size_t) U);
    if (failed) {
        const std::string why = gmx_last_error();
        gmx_set_error("ktruss: the per-edge scratch needs %zu bytes: %s", scratch, why.c_str());
        return GMX_ERR_NOMEM;
    }
    frontier_scan fs;
    if (peel) GMX_CHECK(gmx_frontier_scan_alloc(&fs, (size_t) U, 0));
    gmx_pinned<kt_ctl> h_ctl;
    GMX_CHECK(h_ctl.alloc());
    const kt_ctl* h = h_ctl.p;

    kt_state S;
    S.nb_begin = p->nb_begin.p;
    S.nb_idx = p->nb_idx.p;
    S.nb_eid = p->nb_eid.p;
    S.up_src = p->up_src.p;
    S.up_idx = p->up_idx.p;
    S.sup = sup.p;
    S.rem = rem.p;
    S.truss = truss.p;
    S.q_e = q_e.p;
    S.q_v = q_v.p;
    S.ctl = ctl.p;
    S.U = U;
    const int gu = grid_for(U);

    // ---- support
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.KERNEL));
    phase.begin();
    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(kt_ctl), 0));
    GMX_CHECK(kt_support_into(p, sup0.p));
    hipLaunchKernelGGL(kt_sum_kernel, dim3(gu), dim3(KT_THREADS), 0, 0, (const int32_t*) sup0.p, U, ctl.p);
    GMX_HIP(hipGetLastError());
    phase.end(&ph_ms[1]);

    // ---- levels and rounds
    int64_t levels = 0, scanned = 0, grid_rounds = 0, tail_rounds = 0, level_q0 = 0;
    int32_t s = -2, round = 0;
    if (peel) {
        GMX_HIP(hipMemcpyAsync(sup.p, sup0.p, (size_t) U * sizeof(int32_t), hipMemcpyDeviceToDevice, 0));
        GMX_HIP(hipMemsetAsync(rem.p, 0x7f, (size_t) U * sizeof(int32_t), 0));   // KT_LIVE
        int32_t* la = l0.p;   // the live list (identity: the edges 0 .. U-1, nothing stored yet)
        int32_t* lb = l1.p;
        bool identity = true;
        int64_t nlist = U, qs = 0, qe = 0, at_qs = 0, at_qe = 0;   // at_*: slots of the shorter rows of q[0, qs) and q[0, qe)
        for (;;) {   // every level removes at least one edge, every round of a level at least one more: the loop ends
            const bool boundary = qs == qe;
            if (boundary && nlist == 0) break;
            if (tail_from > 0 && (boundary ? nlist : at_qe - at_qs) <= tail_from) {
                phase.begin();
                hipLaunchKernelGGL(kt_tail_kernel, dim3(1), dim3(KT_TAIL_THREADS), 0, 0, S, la, lb, identity ? 1 : 0, nlist, s, round, qs, qe, level_q0,
                                   at_qe - at_qs, tail_from);
                GMX_HIP(hipGetLastError());
                GMX_CHECK(gmx_read_back(h_ctl, (const kt_ctl*) ctl.p));
                phase.end(&ph_ms[5]);
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
                s = h->t_s;
                at_qe = (int64_t) h->slots;
                at_qs = at_qe - h->t_m;
                if (h->t_state == KT_DONE) break;
                continue;   // KT_BOUNDARY / KT_MIDLEVEL: the step it stopped at is too large for one workgroup and runs on the grid
            }
            if (boundary) {   // a level starts: its s, then the scan
                phase.begin();
                GMX_HIP(hipMemsetAsync(&ctl.p->shard[0], 0xff, sizeof(ctl.p->shard), 0));
                GMX_HIP(hipMemsetAsync(&ctl.p->nkeep, 0, sizeof(kt_word), 0));
                hipLaunchKernelGGL(kt_min_kernel, dim3(grid_for(nlist)), dim3(KT_THREADS), 0, 0, S, identity ? (const int32_t*) nullptr : (const int32_t*) la,
                                   nlist);
                GMX_HIP(hipGetLastError());
                GMX_CHECK(gmx_read_back(h_ctl, (const kt_ctl*) ctl.p));
                unsigned int mn = KT_NONE;
                for (int i = 0; i < BFS_SHARDS; i++) mn = std::min(mn, h->shard[i].minsup);
                if (mn == KT_NONE) {   // every entry was removed by the last rounds
                    nlist = 0;
                    phase.end(&ph_ms[2]);
                    break;
                }
                hipLaunchKernelGGL(kt_scan_kernel, dim3(grid_for(nlist, BFS_ITEMS)), dim3(KT_THREADS), 0, 0, S,
                                   identity ? (const int32_t*) nullptr : (const int32_t*) la, nlist, (int32_t) mn, round, lb);
                GMX_HIP(hipGetLastError());
                GMX_CHECK(gmx_read_back(h_ctl, (const kt_ctl*) ctl.p));
                phase.end(&ph_ms[2]);
                levels++;
                scanned += nlist;
                s = (int32_t) mn;
                nlist = (int64_t) h->nkeep;
                std::swap(la, lb);
                identity = false;
                level_q0 = qs;
                qe = (int64_t) h->qtail;
                at_qe = (int64_t) h->slots;
                if (qe == qs) {
                    gmx_set_error("ktruss: level %d queued no edge", (int) s);
                    return GMX_ERR_HIP;
                }
            } else {   // a round
                phase.begin();
                const int64_t n = qe - qs, m = at_qe - at_qs;
                if (m > 0) {
                    GMX_CHECK(gmx_frontier_offsets(S.nb_begin, q_v.p + qs, n, &fs, nullptr, false));
                    hipLaunchKernelGGL(kt_round_kernel, dim3((unsigned) frontier_tiles(n, m)), dim3(KT_THREADS), 0, 0, S, (const int32_t*) (q_v.p + qs),
                                       (const int32_t*) (q_e.p + qs), n, (const int64_t*) fs.off.p, m, s, round);
                    GMX_HIP(hipGetLastError());
                }
                GMX_CHECK(gmx_read_back(h_ctl, (const kt_ctl*) ctl.p));
                phase.end(&ph_ms[3]);
                grid_rounds++;
                round++;
                qs = qe;
                qe = (int64_t) h->qtail;
                at_qs = at_qe;
                at_qe = (int64_t) h->slots;
            }
        }
        if (phase_log) {
            hipLaunchKernelGGL(kt_maxdec_kernel, dim3(gu), dim3(KT_THREADS), 0, 0, (const int32_t*) sup0.p, (const int32_t*) sup.p, U, ctl.p);
            GMX_HIP(hipGetLastError());
        }
    }
    // ---- the values by uploaded slot
    phase.begin();
    if (support_host || truss_host) {
        hipLaunchKernelGGL(kt_finish_kernel, dim3(grid_for(E)), dim3(KT_THREADS), 0, 0, (const int32_t*) g->begin.p, (const int32_t*) g->node_idx.p,
                           (const int32_t*) g->e_idx2idx.p, V, E, (const int32_t*) p->perm.p, (const int32_t*) p->up_begin.p, (const int32_t*) p->up_idx.p,
                           (const int32_t*) sup0.p, (const int32_t*) truss.p, sup_out.p, truss_out.p);
        GMX_HIP(hipGetLastError());
    }
    phase.end(&ph_ms[4]);
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(gmx_read_back(h_ctl, (const kt_ctl*) ctl.p));
    GMX_CHECK(tm.begin(tm.D2H));
    if (truss_host) GMX_HIP(hipMemcpy(truss_host, truss_out.p, (size_t) E * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (support_host) GMX_HIP(hipMemcpy(support_host, sup_out.p, (size_t) E * sizeof(int32_t), hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    if (peel && (int64_t) h->qtail != U) {
        gmx_set_error("ktruss: %lld of %lld edges were removed", (long long) h->qtail, (long long) U);
        return GMX_ERR_HIP;
    }
    const int64_t top = peel ? U - level_q0 : 0;   // the last level's removals: the edges of the largest truss number
    const int64_t walked = peel ? (int64_t) h->slots : 0;
    if (peel) *max_truss = s + 2;
    stats->iterations = round;
    stats->vertices_reached = top;
    stats->edges_examined = walked;
    if (phase_log)
        fprintf(stderr, "gmx ktruss phases: plan %.3f ms, support %.3f ms, scans %.3f ms, grid %.3f ms, tail %.3f ms, finish %.3f ms, max_decrements %u\n",
                ph_ms[0], ph_ms[1], ph_ms[2], ph_ms[3], ph_ms[5], ph_ms[4], h->maxdec);
    if (getenv("GMX_KTRUSS_LOG"))   // one line per call (tools/ktruss_prof.py and the tests parse it)
        fprintf(stderr,
                "gmx ktruss: plan V %lld E %lld up %lld order %s built %d adj_built %d; support plain triangles %llu; levels %lld rounds %d scanned %lld "
                "grid_rounds %lld tail_rounds %lld slots %lld max_truss %d top %lld\n",
                (long long) p->V, (long long) p->E, (long long) U, p->ordered ? "degree" : "identity", built ? 1 : 0, adj_built ? 1 : 0, h->sum_sup / 3,
                (long long) levels, (int) round, (long long) scanned, (long long) grid_rounds, (long long) tail_rounds, (long long) walked, peel ? (int) (s + 2) : 0, (long long) top);
    return GMX_OK;
}

void gmx_touch_ktruss() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) kt_round_kernel);
}
