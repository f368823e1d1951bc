// gmx_graphlets.hip -- the census of the connected subgraphs on 2, 3 and 4 vertices, in total and per vertex by orbit (the
// 15-entry graphlet degree vector of ORCA), for gfx950: gmx_graphlets.  The reference has no such program; the definition,
// the orbit numbering, the two conventions and the statistics are the contract at gmx_graphlets in gmx.h.
//
// The stored slots are read as gmx_clustering reads them, N(v) = { u != v : v -> u or u -> v is stored }, on the plan of
// gmx_tcd.hip (cached on the graph, shared with the counting family) and its symmetric adjacency, in plan ids.  With d the
// degree, t(e) the triangles on edge e, T(v) those through v and S(u) = sum over w in N(u) of (d_w - 1), every sum below
// over u in N(v), the subgraph (non-induced) counts are
//     n0  = d_v                  n1 = sum (d_u - 1)                n2 = C(d_v, 2)         n3 = T(v)
//     n4  = sum S(u) - d_v (d_v - 1) - 2 T(v)                      n5 = (d_v - 1) n1 - sum t(vu)
//     n6  = sum C(d_u - 1, 2)    n7 = C(d_v, 3)                    n8 = gmx_squares' count
//     n9  = sum T(u) - sum t(vu) n10 = sum t(vu) (d_u - 2)         n11 = T(v) (d_v - 2)
//     n12 = sum over the triangles {v, a, b} of (t(ab) - 1)
//     n13 = sum C(t(vu), 2)      n14 = gmx_kclique's count at k = 4
// and the induced ones follow from them, solved from the bottom up (gl_induced).  All of it in unsigned 64-bit words: the
// transform is integer-linear, so wrap-around in an n_k is harmless and a result is exact whenever it fits an int64 itself.
// C(x, 2) and C(d, 3) divide BEFORE they multiply -- the even factor by two, the factor that is a multiple of three by three
// -- so that the product does not wrap where the binomial itself fits (a star of 3.4 million leaves: d (d - 1) (d - 2) > 2^64).
//
// What already exists stays on the device: t(e) by edge id from gmx_ktruss.hip's support kernel (kt_support_into), the
// per-vertex words of gmx_squares.hip and gmx_kclique.hip (sq_count_into, kc_count_into: gmx_classcount.h).  T(v) is half the
// sum of t(e) over v's row, which pass A takes anyway, so gmx_lcc.hip's walk is not run a second time; d is the row length.
//   pass A   per vertex over its nb row: sum (d_u - 1), sum C(d_u - 1, 2), sum t(e), sum t(e) (d_u - 2), sum C(t(e), 2)
//   pass B   the same loop once S and T are known: sum S(u), sum T(u)
//            A wave takes 64 consecutive vertices, a lane each: a row of up to GL_ALONE slots is walked by its lane, a longer
//            one by the wave, 64 slots a step and one reduction; those rows are owned by one wave and stored without an
//            atomic.  A row of more than GL_LONG slots is listed by pass A and cut into 64-slot groups dealt to the waves of
//            a second launch, which add one atomic per (row, wave) and term.  No per-slot atomics.
//   walk     n12, the hot path: gmx_lcc.hip's walk on UP' (work items (v, group of 64 slots) from gmx_rowgroup.h, UP'(v) from
//            the group's first slot on staged in the wave's LDS slice, lane i owns the slot u = A[i], the shorter of the tail
//            and UP'(u) is streamed and the other searched; by the lane alone up to GL_WALK_ALONE entries, else by the wave).
//            The three edge ids of a match (v, u, w) are positions in up_idx: the slot's, the tail position's and the search
//            hit's in UP'(u).  u takes t(vw) - 1 in a register of the slot's lane, v takes t(uw) - 1 through one wave
//            reduction per item, w takes t(vu) - 1 in a 32-bit LDS counter per list position, flushed once per item (a
//            position takes at most 64 credits of less than V each per item: 32 bits hold them while V <= 2^26, beyond that
//            the plain credits are used).  A list longer than the slice (GMX_GRAPHLETS_CAP entries) is searched in memory and
//            credits w by a global atomic.  LDS: cap x (4 + 4) bytes a wave, 16 KiB a workgroup at the default 512 -- the
//            occupancy gmx_lcc.hip keeps (its 1024 entries with byte counters are 20 KiB); 1024 entries here would be 32 KiB
//            and 20 waves a CU.  The hub bit matrix of gmx_lcc.hip is left out.
//            GMX_GRAPHLETS_PLAIN=1: one work item per edge as kt_support_kernel, every common neighbour w of the edge's ends
//            takes t(e) - 1 by one 64-bit global atomic.
//   finish   per caller's id: the fifteen n_k, the transform if asked for, the row of gdv, the column sums.
// Totals only (gdv_host == NULL): no walk, no pass, no per-vertex credits: one pass over the edges and the vertices
// (sum (d_a - 1)(d_b - 1), sum t(e) (d_a + d_b - 4) = 2 sum T(v) (d_v - 2), sum C(t(e), 2), sum t(e), sum C(d, 2), sum C(d, 3))
// and the totals of gmx_squares' and gmx_kclique's total-only modes.
// Integers only: every result is unique and the same bytes under every knob, order and upload form.
#include "gmx_classcount.h"

#define GL_THREADS 256
#define GL_WAVES 4
#define GL_CLAIM 8           // work items per dequeue (gmx_lcc.hip's)
#define GL_CAP 512           // GMX_GRAPHLETS_CAP: list entries and counters staged per wave (2 KiB + 2 KiB)
#define GL_CAP_MIN 64
#define GL_CAP_MAX 1024
#define GL_WALK_ALONE 4      // a lane walks a side of up to this many entries by itself (gmx_lcc.hip's LCC_ALONE).  NOT MEASURED here
#define GL_ALONE 16          // passes A and B: a lane walks a row of up to this many slots by itself (gmx_ktruss.hip's KT_LANE).  NOT MEASURED
#define GL_LONG 2048         // GMX_GRAPHLETS_LONG: a row of more slots is cut into groups for the second launch
#define GL_LONG_GRID_X 64    // workgroups along a long row ...
#define GL_LONG_GRID_Y 32    // ... and over the list of long rows
#define GL_ORBITS 15
#define GL_GRAPHLETS 9

enum {   // the per-vertex words, [V] each, in plan ids
    GL_A1, GL_A6, GL_ST, GL_A10, GL_A13,   // pass A: sum (d_u - 1), sum C(d_u - 1, 2), sum t(e), sum t(e) (d_u - 2), sum C(t(e), 2)
    GL_BS, GL_BT,                          // pass B: sum S(u), sum T(u)
    GL_W12, GL_SQM, GL_SQE, GL_KC, GL_NACC
};
enum {
    GL_NEXT, GL_STAGED, GL_MEMORY, GL_HITS, GL_NLONG, GL_SQ0, GL_SQ1, GL_KC4, GL_NONZERO, GL_COL0,
    GL_E_P4 = GL_COL0 + GL_ORBITS, GL_E_PAW, GL_E_DIA, GL_E_T, GL_V_C2, GL_V_C3, GL_NCTR
};

__host__ __device__ __forceinline__ cc_word gl_c2(cc_word x) { return (x & 1) ? x * ((x - 1) >> 1) : (x >> 1) * (x - 1); }   // (0 for x = 0: 0 * anything)
__host__ __device__ __forceinline__ cc_word gl_c3(cc_word d) {
    if (d < 3) return 0;
    cc_word a = d, b = d - 1, c = d - 2;
    if (a & 1) b >>= 1; else a >>= 1;             // (halving leaves a multiple of three one)
    const int r = (int) (d % 3);                  // d - r is the multiple of three among d, d - 1, d - 2
    if (r == 0) a /= 3; else if (r == 1) b /= 3; else c /= 3;
    return a * b * c;
}

// ------------------------------------------------------------------ passes A and B
struct gl_rows {
    const int32_t* nb_begin;
    const int32_t* nb_idx;
    const int32_t* nb_eid;
    const int32_t* sup;
    cc_word* acc;
    int64_t V;
    int32_t long_min;
    int32_t* long_list;   // the rows of more than long_min slots, listed by pass A
    cc_word* ctr;
};

template <int PASS> struct gl_pass { static constexpr int K = PASS == 0 ? 5 : 2, FIRST = PASS == 0 ? GL_A1 : GL_BS; };

template <int PASS>
__device__ __forceinline__ void gl_slot(const gl_rows& G, int32_t p, cc_word* x) {
    const int32_t u = G.nb_idx[p];
    if (PASS == 0) {
        const cc_word du = (cc_word) (G.nb_begin[u + 1] - G.nb_begin[u]), t = (cc_word) G.sup[G.nb_eid[p]];   // (du >= 1: v is there)
        x[0] += du - 1;
        x[1] += gl_c2(du - 1);
        x[2] += t;
        x[3] += t * (du - 2);   // (du = 1: t = 0)
        x[4] += gl_c2(t);
    } else {
        x[0] += G.acc[(int64_t) GL_A1 * G.V + u];
        x[1] += G.acc[(int64_t) GL_ST * G.V + u] >> 1;
    }
}

// a wave takes 64 consecutive vertices, a lane each
template <int PASS>
__global__ void __launch_bounds__(GL_THREADS) gl_rows_kernel(gl_rows G) {
    constexpr int K = gl_pass<PASS>::K;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t) blockIdx.x * (GL_THREADS / 64) + (threadIdx.x >> 6), nwaves = (int64_t) gridDim.x * (GL_THREADS / 64);
    for (int64_t base = wave * 64; base < G.V; base += nwaves * 64) {   // (wave-uniform)
        const int64_t v = base + lane;
        int32_t rb = 0, re = 0;
        if (v < G.V) {
            rb = G.nb_begin[v];
            re = G.nb_begin[v + 1];
        }
        const int32_t d = re - rb;
        const bool is_long = d > G.long_min, by_wave = !is_long && d > GL_ALONE;
        cc_word x[K];
#pragma unroll
        for (int k = 0; k < K; k++) x[k] = 0;
        if (!is_long && !by_wave)
            for (int32_t p = rb; p < re; p++) gl_slot<PASS>(G, p, x);
        unsigned long long m = __ballot(by_wave);
        while (m) {   // the longer rows, one after the other by the whole wave: the same trip counts in every lane
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t wb = __builtin_amdgcn_readlane(rb, src), we = __builtin_amdgcn_readlane(re, src);
            cc_word y[K];
#pragma unroll
            for (int k = 0; k < K; k++) y[k] = 0;
            for (int32_t p = wb + lane; p < we; p += 64) gl_slot<PASS>(G, p, y);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const cc_word s = cc_wave_total(y[k]);
                if (lane == src) x[k] = s;
            }
        }
        if (v < G.V && !is_long) {
#pragma unroll
            for (int k = 0; k < K; k++) G.acc[(int64_t) (gl_pass<PASS>::FIRST + k) * G.V + v] = x[k];
        }
        if (PASS == 0 && is_long) G.long_list[atomicAdd(&G.ctr[GL_NLONG], 1ull)] = (int32_t) v;   // (at most 2 |UP'| / long_min of them: the list holds them)
    }
}

// the listed rows: workgroup (x, y) takes the rows y, y + gridDim.y, ... and of each the 64-slot groups its waves are dealt
// round robin; one atomic per (row, wave) and term into words that are zero before the launch
template <int PASS>
__global__ void __launch_bounds__(GL_THREADS) gl_long_rows_kernel(gl_rows G) {
    constexpr int K = gl_pass<PASS>::K;
    const int lane = threadIdx.x & 63;
    const int64_t nlong = (int64_t) G.ctr[GL_NLONG];
    const int64_t wv = (int64_t) blockIdx.x * (GL_THREADS / 64) + (threadIdx.x >> 6), nw = (int64_t) gridDim.x * (GL_THREADS / 64);
    for (int64_t i = blockIdx.y; i < nlong; i += gridDim.y) {   // (workgroup-uniform)
        const int32_t v = G.long_list[i];
        const int32_t rb = G.nb_begin[v], re = G.nb_begin[v + 1];
        cc_word x[K];
#pragma unroll
        for (int k = 0; k < K; k++) x[k] = 0;
        for (int64_t p0 = (int64_t) rb + wv * 64; p0 < re; p0 += nw * 64) {   // (wave-uniform)
            const int64_t p = p0 + lane;
            if (p < re) gl_slot<PASS>(G, (int32_t) p, x);
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const cc_word s = wave_sum(x[k]);
            if (lane == 0 && s) atomicAdd(&G.acc[(int64_t) (gl_pass<PASS>::FIRST + k) * G.V + v], s);
        }
    }
}

// ------------------------------------------------------------------ the weighted triangle walk
struct gl_walk {
    const int32_t* up_begin;
    const int32_t* up_idx;
    const int32_t* sup;     // [|UP'|]: t(e) by edge id
    cc_word* w12;           // [V], zero
};

// the credit of w, found at position f of R, from the slot whose edge carries c = t(vu) - 1
template <bool COUNTERS>
__device__ __forceinline__ void gl_credit_w(uint32_t* cnt, cc_word* __restrict__ w12, int32_t f, int32_t w, int32_t c, bool& touched) {
    if (!c) return;
    if (COUNTERS) {
        atomicAdd(&cnt[f], (uint32_t) c);
        touched = true;
    } else {
        atomicAdd(&w12[w], (cc_word) c);
    }
}

// One work item: R[0, da) is UP'(v) from the group's first slot on, whose edge ids are ab, ab + 1, ... (LDS: the wave's slice;
// otherwise the row in memory); the group's slots are R[0 .. 63], one per lane.  COUNTERS (only with LDS): the w credits go to
// cnt[], which is all zero on entry and on return.  Returns this lane's matches.
template <bool LDS, bool COUNTERS>
__device__ __forceinline__ unsigned int gl_item(const int32_t* R, uint32_t* cnt, int32_t da, int32_t ab, int32_t v, const gl_walk& G, int lane) {
    const int32_t* __restrict__ up_begin = G.up_begin;
    const int32_t* __restrict__ up_idx = G.up_idx;
    const int32_t* __restrict__ sup = G.sup;
    const bool act = lane + 1 < da;
    int32_t bb = 0, be = 0, u = 0, cw = 0;
    if (act) {
        u = R[lane];
        bb = up_begin[u];
        be = up_begin[u + 1];
        cw = sup[ab + lane] - 1;   // what every w of this slot takes (-1 on an edge without a triangle, which has no match)
    }
    const int32_t db = be - bb, ta = act ? da - (lane + 1) : 0;
    const bool tail_side = ta < db;
    const int32_t shorter = db == 0 || ta == 0 ? 0 : (tail_side ? ta : db);
    cc_word cu = 0, cv = 0;   // u's credit (the slot's) and this lane's share of v's
    unsigned int hits = 0;
    bool touched = false;
    if (act && shorter > 0 && shorter <= GL_WALK_ALONE) {
        if (!tail_side) {
            for (int32_t q = bb; q < be; q++) {
                const int32_t w = up_idx[q];
                const int32_t f = rg_lower_bound<LDS>(R, lane + 1, da, w);
                if (f < da && R[f] == w) {
                    hits++;
                    cu += (cc_word) (sup[ab + f] - 1);
                    cv += (cc_word) (sup[q] - 1);
                    gl_credit_w<COUNTERS>(cnt, G.w12, f, w, cw, touched);
                }
            }
        } else {
            for (int32_t f = lane + 1; f < da; f++) {
                const int32_t w = R[f];
                const int32_t q = rg_lower_bound<false>(up_idx, bb, be, w);
                if (q < be && up_idx[q] == w) {
                    hits++;
                    cu += (cc_word) (sup[ab + f] - 1);
                    cv += (cc_word) (sup[q] - 1);
                    gl_credit_w<COUNTERS>(cnt, G.w12, f, w, cw, touched);
                }
            }
        }
    }
    // the other slots, one after the other by the whole wave: every loop below has the same trip count in all lanes
    unsigned long long m = __ballot(act && shorter > GL_WALK_ALONE);
    while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        const int32_t sbb = __builtin_amdgcn_readlane(bb, src), sbe = __builtin_amdgcn_readlane(be, src), scw = __builtin_amdgcn_readlane(cw, src);
        const int32_t sdb = sbe - sbb, sta = da - (src + 1);
        cc_word pu = 0;
        if (sdb <= sta) {   // stream UP'(u), search the tail
            for (int32_t q0 = sbb; q0 < sbe; q0 += 64) {
                const int32_t q = q0 + lane;
                if (q < sbe) {
                    const int32_t w = up_idx[q];
                    const int32_t f = rg_lower_bound<LDS>(R, src + 1, da, w);
                    if (f < da && R[f] == w) {
                        hits++;
                        pu += (cc_word) (sup[ab + f] - 1);
                        cv += (cc_word) (sup[q] - 1);
                        gl_credit_w<COUNTERS>(cnt, G.w12, f, w, scw, touched);
                    }
                }
            }
        } else {            // stream the tail, search UP'(u) in memory
            for (int32_t f0 = src + 1; f0 < da; f0 += 64) {
                const int32_t f = f0 + lane;
                if (f < da) {
                    const int32_t w = R[f];
                    const int32_t q = rg_lower_bound<false>(up_idx, sbb, sbe, w);
                    if (q < sbe && up_idx[q] == w) {
                        hits++;
                        pu += (cc_word) (sup[ab + f] - 1);
                        cv += (cc_word) (sup[q] - 1);
                        gl_credit_w<COUNTERS>(cnt, G.w12, f, w, scw, touched);
                    }
                }
            }
        }
        pu = cc_wave_total(pu);
        if (lane == src) cu = pu;
    }
    const cc_word tot = wave_sum(cv);
    if (lane == 0 && tot) atomicAdd(&G.w12[v], tot);
    if (COUNTERS) {
        // flush the positions' counters and leave them zero.  Lane i's first position is i, its own slot: u's credit rides on
        // that position's atomic
        rg_lds_landed();
        if (__ballot(touched || cu != 0)) {
            for (int32_t k = lane; k < da; k += 64) {
                const uint32_t c = cnt[k];
                if (c) cnt[k] = 0;
                const cc_word sum = (cc_word) c + (k == lane ? cu : 0);   // (cu != 0: lane + 1 < da, so k = lane is visited)
                if (sum) atomicAdd(&G.w12[R[k]], sum);
            }
        }
    } else if (cu) {
        atomicAdd(&G.w12[u], cu);
    }
    return hits;
}

// COUNTERS: the LDS counters for the w credits of staged items; false: a global atomic per credit (V > 2^26)
template <bool COUNTERS>
__global__ void __launch_bounds__(GL_WAVES * 64) gl_walk_kernel(gl_walk G, const int64_t* __restrict__ grp_off, int64_t V, int cap /* <= GL_CAP_MAX */,
                                                                cc_word* __restrict__ ctr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gl_lds[];   // [GL_WAVES][cap] list entries, then as many counters
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int32_t* A = (int32_t*) gl_lds + (size_t) wv * cap;
    uint32_t* cnt = (uint32_t*) gl_lds + (size_t) (GL_WAVES + wv) * cap;
    for (int k = lane; k < cap; k += 64) cnt[k] = 0;
    rg_lds_landed();
    unsigned int staged = 0, in_memory = 0;
    cc_word hits = 0;
    rg_items<GL_CLAIM>(grp_off, V, 0, 1, &ctr[GL_NEXT], lane, [&](int32_t v, int32_t group) {
        const int32_t ab = G.up_begin[v] + group * 64, ae = G.up_begin[v + 1];
        const int32_t da = ae - ab;   // UP'(v) from the group's first slot on (>= 2)
        if (da <= cap) {
            rg_stage(A, G.up_idx + ab, da, lane);
            staged++;
            hits += gl_item<true, COUNTERS>(A, cnt, da, ab, v, G, lane);
            rg_slice_done();
        } else {
            in_memory++;
            hits += gl_item<false, false>(G.up_idx + ab, cnt, da, ab, v, G, lane);
        }
    });
    hits = wave_sum(hits);
    if (lane == 0) {
        if (staged) atomicAdd(&ctr[GL_STAGED], (cc_word) staged);
        if (in_memory) atomicAdd(&ctr[GL_MEMORY], (cc_word) in_memory);
        if (hits) atomicAdd(&ctr[GL_HITS], hits);
    }
}

// GMX_GRAPHLETS_PLAIN=1: a wave takes 64 edge ids at a time, a lane each; the shorter row of the edge's ends is walked (by the
// lane up to GL_ALONE slots, else by the wave) and the longer one searched, as kt_support_kernel does it; every common
// neighbour takes t(e) - 1.  Every triangle is met three times, once from each edge
__global__ void __launch_bounds__(GL_THREADS) gl_plain_walk_kernel(const int32_t* __restrict__ nb_begin, const int32_t* __restrict__ nb_idx,
                                                                   const int32_t* __restrict__ up_src, const int32_t* __restrict__ up_idx,
                                                                   const int32_t* __restrict__ sup, int64_t U, cc_word* __restrict__ w12,
                                                                   cc_word* __restrict__ ctr) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t) blockIdx.x * (GL_THREADS / 64) + (threadIdx.x >> 6), nwaves = (int64_t) gridDim.x * (GL_THREADS / 64);
    cc_word hits = 0;
    for (int64_t base = wave * 64; base < U; base += nwaves * 64) {   // (wave-uniform)
        const int64_t e = base + lane;
        int32_t sb = 0, se = 0, lb = 0, le = 0, c = 0;
        if (e < U) {
            const int32_t a = up_src[e], b = up_idx[e];
            const int32_t ab = nb_begin[a], ae = nb_begin[a + 1], bb = nb_begin[b], be = nb_begin[b + 1];
            const bool a_short = ae - ab <= be - bb;
            sb = a_short ? ab : bb;
            se = a_short ? ae : be;
            lb = a_short ? bb : ab;
            le = a_short ? be : ae;
            c = sup[e] - 1;
            if (c < 0) se = sb;   // no triangle on e: nothing to find
        }
        const bool by_wave = se - sb > GL_ALONE;
        if (!by_wave)
            for (int32_t p = sb; p < se; p++) {
                const int32_t w = nb_idx[p];
                if (rg_contains<false>(nb_idx, lb, le, w)) {
                    hits++;
                    if (c) atomicAdd(&w12[w], (cc_word) c);
                }
            }
        unsigned long long m = __ballot(by_wave);
        while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t wsb = __builtin_amdgcn_readlane(sb, src), wse = __builtin_amdgcn_readlane(se, src), wlb = __builtin_amdgcn_readlane(lb, src),
                          wle = __builtin_amdgcn_readlane(le, src), wc = __builtin_amdgcn_readlane(c, src);
            for (int32_t p = wsb + lane; p < wse; p += 64) {
                const int32_t w = nb_idx[p];
                if (rg_contains<false>(nb_idx, wlb, wle, w)) {
                    hits++;
                    if (wc) atomicAdd(&w12[w], (cc_word) wc);
                }
            }
        }
    }
    hits = wave_sum(hits);
    if (lane == 0 && hits) atomicAdd(&ctr[GL_HITS], hits);
}

// ------------------------------------------------------------------ the transform and the finishing kernel
// n[0 .. 14] -> o[0 .. 14] in place, from the bottom up
__host__ __device__ __forceinline__ void gl_induced(cc_word* n) {
    const cc_word o14 = n[14], o13 = n[13] - 3 * o14, o12 = n[12] - 3 * o14;
    const cc_word o11 = n[11] - 2 * o13 - 3 * o14, o10 = n[10] - 2 * o12 - 2 * o13 - 6 * o14;
    const cc_word o9 = n[9] - 2 * o12 - 3 * o14, o8 = n[8] - o12 - o13 - 3 * o14, o7 = n[7] - o11 - o13 - o14;
    const cc_word o6 = n[6] - o9 - o10 - 2 * o12 - o13 - 3 * o14;
    const cc_word o5 = n[5] - 2 * o8 - o10 - 2 * o11 - 2 * o12 - 4 * o13 - 6 * o14;
    const cc_word o4 = n[4] - 2 * o8 - 2 * o9 - o10 - 4 * o12 - 2 * o13 - 6 * o14;
    const cc_word o3 = n[3];
    n[2] -= o3;
    n[1] -= 2 * o3;
    n[4] = o4; n[5] = o5; n[6] = o6; n[7] = o7; n[8] = o8; n[9] = o9; n[10] = o10; n[11] = o11; n[12] = o12; n[13] = o13;
}

// one thread per caller's id x: the row of gdv; the column sums and the vertices with a 4-node orbit
__global__ void __launch_bounds__(GL_THREADS) gl_finish_kernel(const cc_word* __restrict__ acc, const int32_t* __restrict__ nb_begin,
                                                               const int32_t* __restrict__ perm /* NULL: identity */, int64_t V, int induced,
                                                               int64_t* __restrict__ gdv, cc_word* __restrict__ ctr) {
    cc_word col[GL_ORBITS], nz = 0;
#pragma unroll
    for (int k = 0; k < GL_ORBITS; k++) col[k] = 0;
    for (int64_t x = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; x < V; x += (int64_t) gridDim.x * blockDim.x) {
        const int64_t p = perm ? perm[x] : x;
        auto at = [&](int a) { return acc[(int64_t) a * V + p]; };
        const cc_word d = (cc_word) (nb_begin[p + 1] - nb_begin[p]), st = at(GL_ST), T = st >> 1;
        cc_word n[GL_ORBITS];
        n[0] = d;
        n[1] = at(GL_A1);
        n[2] = gl_c2(d);
        n[3] = T;
        n[4] = at(GL_BS) - d * (d - 1) - 2 * T;
        n[5] = (d - 1) * at(GL_A1) - st;
        n[6] = at(GL_A6);
        n[7] = gl_c3(d);
        n[8] = at(GL_SQM) + (at(GL_SQE) >> 1);
        n[9] = at(GL_BT) - st;
        n[10] = at(GL_A10);
        n[11] = T * (d - 2);
        n[12] = at(GL_W12);
        n[13] = at(GL_A13);
        n[14] = at(GL_KC);
        if (induced) gl_induced(n);
        cc_word any = 0;
#pragma unroll
        for (int k = 0; k < GL_ORBITS; k++) {
            gdv[x * GL_ORBITS + k] = (int64_t) n[k];
            col[k] += n[k];
            if (k >= 4) any |= n[k];
        }
        nz += any ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < GL_ORBITS; k++) {
        const cc_word s = wave_sum(col[k]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&ctr[GL_COL0 + k], s);
    }
    nz = wave_sum(nz);
    if ((threadIdx.x & 63) == 0 && nz) atomicAdd(&ctr[GL_NONZERO], nz);
}

// totals only: the sums over the edge ids and over the vertices
__global__ void __launch_bounds__(GL_THREADS) gl_totals_kernel(const int32_t* __restrict__ nb_begin, const int32_t* __restrict__ up_src,
                                                               const int32_t* __restrict__ up_idx, const int32_t* __restrict__ sup, int64_t V, int64_t U,
                                                               cc_word* __restrict__ ctr) {
    cc_word s[6] = {0, 0, 0, 0, 0, 0};
    const int64_t first = (int64_t) blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t e = first; e < U; e += stride) {
        const int32_t a = up_src[e], b = up_idx[e];
        const cc_word da = (cc_word) (nb_begin[a + 1] - nb_begin[a]), db = (cc_word) (nb_begin[b + 1] - nb_begin[b]), t = (cc_word) sup[e];
        s[0] += (da - 1) * (db - 1);
        s[1] += t * (da + db - 4);   // (t = 0 unless both ends have two neighbours)
        s[2] += gl_c2(t);
        s[3] += t;
    }
    for (int64_t v = first; v < V; v += stride) {
        const cc_word d = (cc_word) (nb_begin[v + 1] - nb_begin[v]);
        s[4] += gl_c2(d);
        s[5] += gl_c3(d);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const cc_word t = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&ctr[GL_E_P4 + k], t);
    }
}

// ------------------------------------------------------------------ host
// a sum identity of the orbits' column sums
static int gl_identity(const char* what, cc_word a, cc_word b) {
    if (a == b) return GMX_OK;
    gmx_set_error("graphlets: %s: %llu against %llu", what, a, b);
    return GMX_ERR_HIP;
}

extern "C" int gmx_graphlets(gmx_graph_t* g, int induced, int64_t* gdv_host, int64_t* totals, gmx_stats_t* stats) {
    GMX_REQUIRE(totals, "NULL totals");
    GMX_REQUIRE(induced == 0 || induced == 1, "graphlets: induced = %d is neither 0 nor 1", induced);
    GMX_REQUIRE(g, "NULL graph");
    if (stats) memset(stats, 0, sizeof(*stats));
    memset(totals, 0, GL_GRAPHLETS * sizeof(int64_t));
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    // knobs, read at every call; no result byte depends on them
    const bool ordered = !getenv("GMX_GRAPHLETS_NO_ORDER");
    const bool plain = getenv("GMX_GRAPHLETS_PLAIN") != nullptr;
    const bool phase_log = getenv("GMX_GRAPHLETS_PHASES") != nullptr;
    const int cap = (int) gmx_env_int("GMX_GRAPHLETS_CAP", GL_CAP, GL_CAP_MIN, GL_CAP_MAX);
    const int32_t long_min = (int32_t) gmx_env_int("GMX_GRAPHLETS_LONG", GL_LONG, 1, INT32_MAX);
    const bool counts = gdv_host != nullptr;
    const int mode = !counts ? CC_NONE : plain ? CC_PLAIN : CC_LOCAL;   // the walk's credits (the log line's `counts`)
    const int family_mode = counts ? CC_LOCAL : CC_NONE;                // gmx_squares' and gmx_kclique's: never their plain forms (4-cliques: 400 x on RMAT-20)
    bool empty = false;
    GMX_CHECK(cc_answer_empty(g, nullptr, stats, &empty));
    if (empty) {
        if (gdv_host) memset(gdv_host, 0, (size_t) V * GL_ORBITS * sizeof(int64_t));
        return GMX_OK;
    }
    // graph preprocessing (cached on the graph, shared with the other entries on the plan; outside the timed region)
    bool built = false;
    tcd_plan* p = nullptr;
    GMX_CHECK(tcd_plan_get(g, ordered, &p, &built));
    const int64_t U = p->E_up;
    float ph_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // plan additions, support, pass A, pass B, walk, squares, kclique, finish (GMX_GRAPHLETS_PHASES)
    gmx_phase_clock phase;
    GMX_CHECK(phase.enable(phase_log));
    const bool adj_built = !p->kt_ready, groups_built = counts && !plain && !p->lcc_ready;
    bool sq_built = false, kc_built = false;
    phase.begin();
    GMX_CHECK(tcd_plan_adjacency(p));
    if (counts && !plain) GMX_CHECK(lcc_plan_groups(p));
    phase.end(&ph_ms[0]);

    // the call's scratch: t(e) by edge id, the per-vertex words in the plan's numbering, the list of long rows, the rows asked for, the sums
    dbuf<int32_t> sup, long_list;
    dbuf<cc_word> acc, ctr;
    dbuf<int64_t> gdv;
    const size_t n_long_max = (size_t) (2 * U / long_min) + 1;
    const size_t scratch = (size_t) U * 4 + GL_NCTR * sizeof(cc_word) + (counts ? (size_t) V * (GL_NACC + GL_ORBITS) * 8 + n_long_max * 4 : 0);
    if (sup.alloc((size_t) U) || ctr.alloc(GL_NCTR) || (counts && (acc.alloc((size_t) GL_NACC * (size_t) V) || long_list.alloc(n_long_max) || gdv.alloc((size_t) V * GL_ORBITS)))) {
        const std::string why = gmx_last_error();
        gmx_set_error("graphlets: the per-edge and per-vertex scratch needs %zu bytes: %s", scratch, why.c_str());
        return GMX_ERR_NOMEM;
    }
    GMX_HIP(hipMemset(ctr.p, 0, GL_NCTR * sizeof(cc_word)));
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.KERNEL));
    phase.begin();
    GMX_CHECK(kt_support_into(p, sup.p));
    phase.end(&ph_ms[1]);
    if (counts) {
        GMX_HIP(hipMemsetAsync(acc.p, 0, (size_t) GL_NACC * (size_t) V * sizeof(cc_word), 0));
        const gl_rows R = {p->nb_begin.p, p->nb_idx.p, p->nb_eid.p, sup.p, acc.p, V, long_min, long_list.p, ctr.p};
        const dim3 rows_grid(grid_for(V, GL_THREADS / 64 * 64, 256 * 16)), long_grid(GL_LONG_GRID_X, GL_LONG_GRID_Y);
        phase.begin();
        hipLaunchKernelGGL(gl_rows_kernel<0>, rows_grid, dim3(GL_THREADS), 0, 0, R);
        hipLaunchKernelGGL(gl_long_rows_kernel<0>, long_grid, dim3(GL_THREADS), 0, 0, R);
        GMX_HIP(hipGetLastError());
        phase.end(&ph_ms[2]);
        phase.begin();
        hipLaunchKernelGGL(gl_rows_kernel<1>, rows_grid, dim3(GL_THREADS), 0, 0, R);
        hipLaunchKernelGGL(gl_long_rows_kernel<1>, long_grid, dim3(GL_THREADS), 0, 0, R);
        GMX_HIP(hipGetLastError());
        phase.end(&ph_ms[3]);
        phase.begin();
        cc_word* const w12 = acc.p + (size_t) GL_W12 * V;
        if (plain) {
            hipLaunchKernelGGL(gl_plain_walk_kernel, dim3(grid_for(U)), dim3(GL_THREADS), 0, 0, (const int32_t*) p->nb_begin.p, (const int32_t*) p->nb_idx.p,
                               (const int32_t*) p->up_src.p, (const int32_t*) p->up_idx.p, (const int32_t*) sup.p, U, w12, ctr.p);
        } else {
            const gl_walk W = {p->up_begin.p, p->up_idx.p, sup.p, w12};
            const size_t lds = (size_t) GL_WAVES * cap * 2 * sizeof(int32_t);
            if (V <= (1LL << 26))
                hipLaunchKernelGGL(gl_walk_kernel<true>, dim3(256 * 8), dim3(GL_WAVES * 64), lds, 0, W, (const int64_t*) p->up_grp_off.p, V, cap, ctr.p);
            else
                hipLaunchKernelGGL(gl_walk_kernel<false>, dim3(256 * 8), dim3(GL_WAVES * 64), lds, 0, W, (const int64_t*) p->up_grp_off.p, V, cap, ctr.p);
        }
        GMX_HIP(hipGetLastError());
        phase.end(&ph_ms[4]);
    } else {
        phase.begin();
        hipLaunchKernelGGL(gl_totals_kernel, dim3(grid_for(U > V ? U : V)), dim3(GL_THREADS), 0, 0, (const int32_t*) p->nb_begin.p, (const int32_t*) p->up_src.p,
                           (const int32_t*) p->up_idx.p, (const int32_t*) sup.p, V, U, ctr.p);
        GMX_HIP(hipGetLastError());
        phase.end(&ph_ms[2]);
    }
    phase.begin();
    GMX_CHECK(sq_count_into(p, family_mode, counts ? acc.p + (size_t) GL_SQM * V : nullptr, counts ? acc.p + (size_t) GL_SQE * V : nullptr, ctr.p + GL_SQ0, &sq_built));
    phase.end(&ph_ms[5]);
    phase.begin();
    GMX_CHECK(kc_count_into(p, 4, family_mode, counts ? acc.p + (size_t) GL_KC * V : nullptr, ctr.p + GL_KC4, &kc_built));
    phase.end(&ph_ms[6]);
    phase.begin();
    if (counts) {
        hipLaunchKernelGGL(gl_finish_kernel, dim3(grid_for(V, GL_THREADS, 256 * 16)), dim3(GL_THREADS), 0, 0, (const cc_word*) acc.p, (const int32_t*) p->nb_begin.p,
                           (const int32_t*) p->perm.p, V, induced, gdv.p, ctr.p);
        GMX_HIP(hipGetLastError());
    }
    phase.end(&ph_ms[7]);
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    cc_word h[GL_NCTR];
    GMX_HIP(hipMemcpy(h, ctr.p, sizeof(h), hipMemcpyDeviceToHost));
    if (counts) GMX_HIP(hipMemcpy(gdv_host, gdv.p, (size_t) V * GL_ORBITS * sizeof(int64_t), hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    cc_word G[GL_GRAPHLETS];
    const cc_word squares = h[GL_SQ0] + h[GL_SQ1] / 2, cliques = h[GL_KC4];
    cc_word walked = 0;
    if (counts) {
        const cc_word* c = h + GL_COL0;
        GMX_CHECK(gl_identity("the ends and the inner vertices of the 4-paths", c[4], c[5]));
        GMX_CHECK(gl_identity("the leaves of the claws and three times their centres", c[6], 3 * c[7]));
        GMX_CHECK(gl_identity("the tails' ends and the carrying corners of the paws", c[9], c[11]));
        GMX_CHECK(gl_identity("the far corners of the paws and twice the carrying ones", c[10], 2 * c[11]));
        GMX_CHECK(gl_identity("the two kinds of corners of the diamonds", c[12], c[13]));
        walked = plain ? h[GL_HITS] / 3 : h[GL_HITS];
        GMX_CHECK(gl_identity("the triangles walked and a third of the triangle orbit's sum", 3 * walked, c[3]));
        GMX_CHECK(gl_identity("the degrees and twice the edges", c[0], 2 * (cc_word) U));
        G[0] = c[0] / 2; G[1] = c[2]; G[2] = c[3] / 3; G[3] = c[4] / 2; G[4] = c[7]; G[5] = c[8] / 4; G[6] = c[11]; G[7] = c[13] / 2; G[8] = c[14] / 4;
        // the squares and the 4-cliques as their own entries total them (under either convention n8 and n14 are reachable from the sums)
        const cc_word n14 = c[14], n8 = induced ? c[8] + c[12] + c[13] + 3 * c[14] : c[8];
        GMX_CHECK(gl_identity("the square orbit's sum and four times the squares", n8, 4 * squares));
        GMX_CHECK(gl_identity("the clique orbit's sum and four times the 4-cliques", n14, 4 * cliques));
    } else {
        const cc_word tri = h[GL_E_T] / 3;
        G[0] = (cc_word) U; G[1] = h[GL_V_C2]; G[2] = tri; G[3] = h[GL_E_P4] - 3 * tri; G[4] = h[GL_V_C3]; G[5] = squares; G[6] = h[GL_E_PAW] / 2; G[7] = h[GL_E_DIA];
        G[8] = cliques;
        if (induced) {
            G[7] -= 6 * G[8];
            G[6] -= 4 * G[7] + 12 * G[8];
            G[5] -= G[7] + 3 * G[8];
            G[4] -= G[6] + 2 * G[7] + 4 * G[8];
            G[3] -= 4 * G[5] + 2 * G[6] + 6 * G[7] + 12 * G[8];
            G[1] -= 3 * G[2];
        }
    }
    for (int k = 0; k < GL_GRAPHLETS; k++) totals[k] = (int64_t) G[k];
    if (stats) {
        stats->iterations = 1;
        stats->edges_examined = (int64_t) walked;
        stats->vertices_reached = counts ? (int64_t) h[GL_NONZERO] : 0;
    }
    if (phase_log)
        fprintf(stderr, "gmx graphlets phases: plan %.3f ms, support %.3f ms, pass_a %.3f ms, pass_b %.3f ms, walk %.3f ms, squares %.3f ms, kclique %.3f ms, finish %.3f ms\n",
                ph_ms[0], ph_ms[1], ph_ms[2], ph_ms[3], ph_ms[4], ph_ms[5], ph_ms[6], ph_ms[7]);
    if (getenv("GMX_GRAPHLETS_LOG"))   // one line per call (tools/graphlets_prof.py and the tests parse it)
        fprintf(stderr, "gmx graphlets: plan V %lld E %lld up %lld order %s built %d adj_built %d groups_built %d squares_built %d kclique_built %d; cap %d long %d "
                        "counts %s induced %d; items %llu staged + %llu memory; long_rows %llu; triangles %llu; totals %llu %llu %llu %llu %llu %llu %llu %llu %llu\n",
                (long long) p->V, (long long) p->E, (long long) U, p->ordered ? "degree" : "identity", built ? 1 : 0, adj_built ? 1 : 0, groups_built ? 1 : 0, sq_built ? 1 : 0,
                kc_built ? 1 : 0, cap, (int) long_min, cc_mode_word(mode), induced, h[GL_STAGED], h[GL_MEMORY], h[GL_NLONG], walked, G[0], G[1], G[2], G[3], G[4], G[5],
                G[6], G[7], G[8]);
    return GMX_OK;
}

void gmx_touch_graphlets() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) gl_rows_kernel<0>);
    (void) cc_finish_kernel;   // (gmx_classcount.h's: the rows here are finished by gl_finish_kernel)
}
