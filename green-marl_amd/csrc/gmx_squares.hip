// gmx_squares.hip -- 4-cycle (square) counts, in total and through every vertex, for gfx950: gmx_squares.  The reference has
// no such program; the definition, the method, the routing rule of the classes and the statistics are the contract at
// gmx_squares in gmx.h.
//
// The stored slots are read as gmx_clustering reads them, N(v) = { u != v : v -> u or u -> v is stored }, on the plan of
// gmx_tcd.hip (cached on the graph, shared with gmx_triangle_counting_directed, gmx_clustering, gmx_ktruss and gmx_kclique)
// and the symmetric adjacency that tcd_plan_adjacency adds to it: row v of nb_idx = DOWN'(v) then UP'(v), sorted.  A square is
// found exactly once, at its highest plan id u, by the wedges u - v - w with v in DOWN'(u), w in N'(v), w < u: with c(w) the
// wedges of u that end in w, the squares with top u and opposite vertex w number C(c(w), 2).  The frame of the entry, the mode
// dispatch, the batches and the finishing kernel are gmx_classcount.h's, shared with gmx_kclique.hip.
//   additions  per DOWN' slot (u, v) the prefix length |{ w in N'(v) : w < u }| (one binary search), kept as the exclusive
//              sums inside u's row, so that a row can be cut by wedges; W(u) = the wedges of u; the vertices by ascending W
//              (one device sort; the vertices with fewer than two lower neighbours in front).
//   pass 1     every wedge adds 1 to the table entry of its w.  Without count_host the add returns the old value, and the sum
//              of the old values over the c adds to one entry is 0 + 1 + ... + (c - 1) = C(c, 2) in whatever order they
//              arrive: that is the total, and there is no pass 2.
//   pass 2     the same wedges again, x = c(w) - 1: v takes x (summed over the slot's wedges in a register, one atomic per
//              slot), w and u take x into the doubled accumulator end2 (u's share by a wave reduction), and the sum of x over
//              u's wedges is twice its squares.  count = mid + end2 / 2, permuted back by the finishing kernel.
// Size classes, one launch each over a range of the list:
//   wave     W <= GMX_SQUARES_WAVE_MAX: a wave per vertex, an open-addressing table (key w, count) of at least 2 W slots in
//            the wave's LDS slice, LDS atomics.
//   block    W <= GMX_SQUARES_LDS_SLOTS / 2: a workgroup per vertex, the table in dynamic LDS.
//   global   the rest: u int32 counters per vertex in workspace memory (all zero between calls of a batch), dealt in batches
//            of at most GMX_SQUARES_BATCH_BYTES; per batch a counting, a crediting and a zeroing launch (the last one walks
//            the wedges again and stores 0, it does not clear V words).  The vertices with W > GMX_SQUARES_SPLIT, a suffix
//            of the batch, go to a launch of their own in which a vertex is cut into ranges of DOWN' slots of about SPLIT
//            wedges, a workgroup each.
//   skipped  fewer than two lower neighbours: never launched.
// A slot's wedges are walked by its lane when they are at most SQ_ALONE, else by the wave, 64 a step.
// Every loop ends by construction (a row or a prefix is walked once; a probe sequence visits at most every slot of a table
// that is at most half full); no kernel waits for another workgroup.  Integers only: every result is unique and the same
// bytes under every knob.
#include "gmx_classcount.h"

#define SQ_THREADS 256
#define SQ_WAVES 4                    // waves of a wave-class workgroup
#define SQ_WAVE_SLOTS 256             // table slots of a wave's LDS slice (2 KiB)
#define SQ_WAVE_MAX (SQ_WAVE_SLOTS / 2)   // GMX_SQUARES_WAVE_MAX: the wave class holds W <= this (at most half the slice).  Swept on RMAT-20
                                      // (DESIGN.md 4.2v): 0 .. 128 within 0.2 %, the class is 0.1 ms of 527
#define SQ_BLOCK_THREADS 256
#define SQ_LDS_SLOTS 4096             // GMX_SQUARES_LDS_SLOTS: table slots of a block-class workgroup, 8 bytes each: 32 KiB, five workgroups a CU.
                                      // Swept on RMAT-20: 1024 +2 %, 2048 .. 8192 flat, 18432 -1 % (one workgroup a CU: the class itself 1.5 -> 9.1 ms)
#define SQ_LDS_SLOTS_MIN 64
#define SQ_LDS_SLOTS_MAX 18432        // 144 KiB of the CU's 160
#define SQ_SPLIT 4096                 // GMX_SQUARES_SPLIT: a global-class vertex with more wedges is cut into workgroups of about this many.
                                      // Swept on RMAT-20: 4096 -10 %, 16384 -6 % against 65536; 262144 +11 %, never +57 %; at this default 1024 +1 %
#define SQ_MAX_PARTS 1024             // ... at most this many
#define SQ_BATCH_BYTES (1LL << 30)    // GMX_SQUARES_BATCH_BYTES: counters of one global-class batch.  Swept on RMAT-20 (4 MiB of counters a vertex):
                                      // 64 MiB +60 %, 1 GiB -10 % against 256 MiB -- a batch of few vertices does not fill the machine; 4 GiB +13 % against 1 GiB
#define SQ_ALONE 16                   // a lane walks a prefix of up to this many entries by itself.  Taken over from gmx_kclique.hip's KC_ALONE.  NOT MEASURED
#define SQ_EMPTY (-1)                 // a free table slot (no plan id)

enum { SQ_TOTAL, SQ_TOTAL2, SQ_NONZERO, SQ_SUM, SQ_NCTR };   // squares = TOTAL + TOTAL2 / 2
enum { SQ_STEP_COUNT, SQ_STEP_CREDIT, SQ_STEP_ZERO };       // the launches of a global-class batch

struct sq_graph {   // what every kernel reads of the plan
    const int32_t* nb_begin;
    const int32_t* nb_idx;
    const int32_t* up_begin;
    const int32_t* excl;   // [|UP'|]: per DOWN' slot (u's row begins at nb_begin[u] - up_begin[u]) the wedges of the slots in front of it
    const uint32_t* W;     // [V]
};

// open addressing in LDS, linear probing: key[S] (SQ_EMPTY: free) and cnt[S]; at most S / 2 distinct keys are inserted
struct sq_hash {
    int32_t* key;
    int32_t* cnt;
    uint32_t S;
    __device__ __forceinline__ uint32_t home(int32_t w) const { return (uint32_t) (((uint64_t) ((uint32_t) w * 0x9E3779B1u) * S) >> 32); }
    __device__ __forceinline__ int32_t add(int32_t w) const {   // + 1; the count before
        uint32_t s = home(w);
        for (uint32_t t = 0; t < S; t++) {
            const int32_t old = atomicCAS(&key[s], SQ_EMPTY, w);
            if (old == SQ_EMPTY || old == w) return atomicAdd(&cnt[s], 1);
            s = s + 1 == S ? 0 : s + 1;
        }
        return 0;   // (never: a free slot exists)
    }
    __device__ __forceinline__ int32_t get(int32_t w) const {   // of a key that is there
        uint32_t s = home(w);
        for (uint32_t t = 0; t < S; t++) {
            if (key[s] == w) return cnt[s];
            s = s + 1 == S ? 0 : s + 1;
        }
        return 1;   // (never)
    }
};
// u counters in workspace memory, indexed by w < u
struct sq_dense {
    int32_t* ctr;
    __device__ __forceinline__ int32_t add(int32_t w) const { return atomicAdd(&ctr[w], 1); }
    __device__ __forceinline__ int32_t get(int32_t w) const { return ctr[w]; }
};

struct sq_vertex {   // u as the kernels see it
    int32_t u, rb, pb, D;
    uint32_t W;
};
__device__ __forceinline__ sq_vertex sq_vertex_of(const sq_graph& G, int32_t u) {
    const int32_t rb = G.nb_begin[u], ub = G.up_begin[u];
    return {u, rb, rb - ub, G.nb_begin[u + 1] - rb - (G.up_begin[u + 1] - ub), G.W[u]};
}

// The wedges u - v - w of u's DOWN' slots [j0, j1), 64 slots a chunk, the chunks dealt round robin to the nwaves waves that
// call this together (this one is wave wv): f(v, w) per wedge returns what the wedge adds to its slot's sum, g(v, sum) is
// called once per slot with a sum that is not zero, by one lane.  Returns this lane's share of the sum over all the wedges.
template <class F, class G>
__device__ __forceinline__ cc_word sq_walk(const sq_graph& P, const sq_vertex& X, int32_t j0, int32_t j1, int wv, int nwaves, int lane, F f, G g) {
    cc_word mine = 0;
    for (int32_t jc = j0 + wv * 64; jc < j1; jc += nwaves * 64) {   // (wave-uniform)
        const int32_t j = jc + lane;
        const bool act = j < j1;
        int32_t v = 0, vb = 0, len = 0;
        if (act) {
            v = P.nb_idx[X.rb + j];
            vb = P.nb_begin[v];
            len = (int32_t) ((j + 1 < X.D ? (uint32_t) P.excl[X.pb + j + 1] : X.W) - (uint32_t) P.excl[X.pb + j]);
        }
        const bool by_wave = len > SQ_ALONE;
        if (!by_wave) {   // (len == 0 where the lane has no slot)
            cc_word s = 0;
            for (int32_t i = 0; i < len; i++) s += f(v, P.nb_idx[vb + i]);
            if (s) g(v, s);
            mine += s;
        }
        unsigned long long m = __ballot(by_wave);
        while (m) {   // (the same trip counts in every lane)
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t sv = __builtin_amdgcn_readlane(v, src), svb = __builtin_amdgcn_readlane(vb, src), slen = __builtin_amdgcn_readlane(len, src);
            cc_word s = 0;
            for (int32_t i = lane; i < slen; i += 64) s += f(sv, P.nb_idx[svb + i]);
            mine += s;
            s = wave_sum(s);
            if (lane == 0 && s) g(sv, s);
        }
    }
    return mine;
}

// pass 2's wedge: x = c(w) - 1 to w (PLAIN: to v and u as well, one atomic each)
template <int MODE, class Table>
__device__ __forceinline__ cc_word sq_credit_wedge(const Table& T, int32_t u, int32_t v, int32_t w, cc_word* __restrict__ mid, cc_word* __restrict__ end2) {
    const cc_word x = (cc_word) (T.get(w) - 1);
    if (x) {
        atomicAdd(&end2[w], x);
        if (MODE == CC_PLAIN) {
            atomicAdd(&mid[v], x);
            atomicAdd(&end2[u], x);
        }
    }
    return x;
}

// both passes over the slots [j0, j1) of one vertex by nwaves waves; `between` separates the passes (the table's adds have
// landed for every wave that reads it).  Returns this lane's share of the total (NONE) or of the doubled total, and gives
// u its share.
template <int MODE, class Table, class Sync>
__device__ __forceinline__ cc_word sq_vertex_passes(const sq_graph& P, const sq_vertex& X, const Table& T, int32_t j0, int32_t j1, int wv, int nwaves, int lane,
                                                    cc_word* __restrict__ mid, cc_word* __restrict__ end2, Sync between) {
    auto nothing = [](int32_t, cc_word) {};
    if (MODE == CC_NONE) return sq_walk(P, X, j0, j1, wv, nwaves, lane, [&](int32_t, int32_t w) { return (cc_word) T.add(w); }, nothing);
    sq_walk(P, X, j0, j1, wv, nwaves, lane, [&](int32_t, int32_t w) { (void) T.add(w); return (cc_word) 0; }, nothing);
    between();
    const int32_t u = X.u;
    const cc_word mine = sq_walk(P, X, j0, j1, wv, nwaves, lane, [&](int32_t v, int32_t w) { return sq_credit_wedge<MODE>(T, u, v, w, mid, end2); },
                                 [&](int32_t v, cc_word s) { if (MODE == CC_LOCAL) atomicAdd(&mid[v], s); });
    if (MODE == CC_LOCAL) {
        const cc_word own = cc_wave_total(mine);
        if (lane == 0 && own) atomicAdd(&end2[u], own);
    }
    return mine;
}

__device__ __forceinline__ void sq_tally(cc_word mine, int mode, int lane, cc_word* __restrict__ out) {
    mine = wave_sum(mine);
    if (lane == 0 && mine) atomicAdd(&out[mode == CC_NONE ? SQ_TOTAL : SQ_TOTAL2], mine);
}

// ------------------------------------------------------------------ the plan's additions
// a wave per vertex u: the prefix length of every DOWN' slot, scanned inside the row; W[u]; the sort key: 0 for a vertex
// with fewer than two lower neighbours, else W + 1; the wedges of the others summed
__global__ void __launch_bounds__(SQ_THREADS) sq_prefix_kernel(const int32_t* __restrict__ nb_begin, const int32_t* __restrict__ nb_idx,
                                                               const int32_t* __restrict__ up_begin, int64_t V, int32_t* __restrict__ excl,
                                                               uint32_t* __restrict__ W, uint32_t* __restrict__ key, cc_word* __restrict__ wedges) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t) gridDim.x * (SQ_THREADS / 64);
    cc_word live = 0;
    for (int64_t u = (int64_t) blockIdx.x * (SQ_THREADS / 64) + (threadIdx.x >> 6); u < V; u += nwaves) {   // (wave-uniform)
        const int32_t rb = nb_begin[u], ub = up_begin[u];
        const int32_t D = nb_begin[u + 1] - rb - (up_begin[u + 1] - ub), pb = rb - ub;
        uint32_t carry = 0;
        for (int32_t jc = 0; jc < D; jc += 64) {
            const int32_t j = jc + lane;
            uint32_t len = 0;
            if (j < D) {
                const int32_t v = nb_idx[rb + j], vb = nb_begin[v];
                len = (uint32_t) (rg_lower_bound<false>(nb_idx, vb, nb_begin[v + 1], (int32_t) u) - vb);
            }
            uint32_t incl = len;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            if (j < D) excl[pb + j] = (int32_t) (carry + incl - len);
            carry += (uint32_t) __builtin_amdgcn_readlane((int) incl, 63);
        }
        if (lane == 0) {
            W[u] = carry;
            key[u] = D >= 2 ? carry + 1 : 0;
            if (D >= 2) live += carry;
        }
    }
    if (lane == 0 && live) atomicAdd(wedges, live);
}

// ------------------------------------------------------------------ wave class
template <int MODE>
__global__ void __launch_bounds__(SQ_WAVES * 64) sq_wave_kernel(sq_graph P, const int32_t* __restrict__ list, int64_t n, cc_word* __restrict__ mid,
                                                                cc_word* __restrict__ end2, cc_word* __restrict__ out) {
    __shared__ int32_t s_key[SQ_WAVES][SQ_WAVE_SLOTS];
    __shared__ int32_t s_cnt[SQ_WAVES][SQ_WAVE_SLOTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cc_word total = 0;
    const int64_t nwaves = (int64_t) gridDim.x * SQ_WAVES;
    for (int64_t it = (int64_t) blockIdx.x * SQ_WAVES + wv; it < n; it += nwaves) {   // (wave-uniform)
        const sq_vertex X = sq_vertex_of(P, list[it]);
        const uint32_t S = X.W > 32 ? 2 * X.W : 64;   // (W <= SQ_WAVE_SLOTS / 2)
        for (uint32_t s = lane; s < S; s += 64) {
            s_key[wv][s] = SQ_EMPTY;
            s_cnt[wv][s] = 0;
        }
        rg_lds_landed();
        const sq_hash T = {s_key[wv], s_cnt[wv], S};
        total += sq_vertex_passes<MODE>(P, X, T, 0, X.D, 0, 1, lane, mid, end2, [] { rg_lds_landed(); });
        rg_lds_landed();   // all lanes are done with the table before it is cleared
    }
    sq_tally(total, MODE, lane, out);
}

// ------------------------------------------------------------------ block class
template <int MODE>
__global__ void __launch_bounds__(SQ_BLOCK_THREADS) sq_block_kernel(sq_graph P, const int32_t* __restrict__ list, int64_t n, uint32_t slots,
                                                                    cc_word* __restrict__ mid, cc_word* __restrict__ end2, cc_word* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sq_lds[];
    int32_t* key = (int32_t*) sq_lds;
    int32_t* cnt = key + slots;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    cc_word total = 0;
    for (int64_t it = blockIdx.x; it < n; it += gridDim.x) {   // (workgroup-uniform)
        const sq_vertex X = sq_vertex_of(P, list[it]);
        const uint32_t S = X.W > 32 ? 2 * X.W : 64;   // (W <= slots / 2, slots >= 64)
        for (uint32_t s = tid; s < S; s += SQ_BLOCK_THREADS) {
            key[s] = SQ_EMPTY;
            cnt[s] = 0;
        }
        __syncthreads();
        const sq_hash T = {key, cnt, S};
        total += sq_vertex_passes<MODE>(P, X, T, 0, X.D, wv, SQ_BLOCK_THREADS / 64, lane, mid, end2, [] { __syncthreads(); });
        __syncthreads();   // everybody is done with the table before it is cleared
    }
    sq_tally(total, MODE, lane, out);
}

// ------------------------------------------------------------------ global class
// the workgroups a vertex of W wedges and D lower neighbours is cut into
__host__ __device__ __forceinline__ int32_t sq_parts(int64_t W, int64_t D, int64_t split) {
    if (W <= split) return 1;
    int64_t p = (W + split - 1) / split;
    p = p < D ? p : D;
    return (int32_t) (p < SQ_MAX_PARTS ? p : SQ_MAX_PARTS);
}

// workgroup (b, part): vertex list[b], whose counters are ws[b * stride ...), all zero before the batch and after it
template <int MODE, int STEP>
__global__ void __launch_bounds__(SQ_BLOCK_THREADS) sq_global_kernel(sq_graph P, const int32_t* __restrict__ list, int64_t split, int32_t* __restrict__ ws,
                                                                     int64_t ws_off, int64_t stride, cc_word* __restrict__ mid, cc_word* __restrict__ end2,
                                                                     cc_word* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = SQ_BLOCK_THREADS / 64;
    const sq_vertex X = sq_vertex_of(P, list[blockIdx.x]);
    const int32_t parts = sq_parts(X.W, X.D, split), part = (int32_t) blockIdx.y;
    if (part >= parts) return;   // (workgroup-uniform)
    // the slots whose first wedge lies in this part's share of the W wedges
    const int32_t* ex = P.excl + X.pb;
    const int32_t j0 = part == 0 ? 0 : rg_lower_bound<false>(ex, 0, X.D, (int32_t) ((uint64_t) part * X.W / (uint32_t) parts));
    const int32_t j1 = part + 1 == parts ? X.D : rg_lower_bound<false>(ex, 0, X.D, (int32_t) ((uint64_t) (part + 1) * X.W / (uint32_t) parts));
    const sq_dense T = {ws + (ws_off + (int64_t) blockIdx.x) * stride};
    auto nothing = [](int32_t, cc_word) {};
    const int32_t u = X.u;
    cc_word mine = 0;
    if (STEP == SQ_STEP_COUNT) {
        if (MODE == CC_NONE)
            mine = sq_walk(P, X, j0, j1, wv, nw, lane, [&](int32_t, int32_t w) { return (cc_word) T.add(w); }, nothing);
        else
            sq_walk(P, X, j0, j1, wv, nw, lane, [&](int32_t, int32_t w) { (void) T.add(w); return (cc_word) 0; }, nothing);
    } else if (STEP == SQ_STEP_CREDIT) {
        mine = sq_walk(P, X, j0, j1, wv, nw, lane, [&](int32_t v, int32_t w) { return sq_credit_wedge<MODE>(T, u, v, w, mid, end2); },
                       [&](int32_t v, cc_word s) { if (MODE == CC_LOCAL) atomicAdd(&mid[v], s); });
        if (MODE == CC_LOCAL) {
            const cc_word own = cc_wave_total(mine);
            if (lane == 0 && own) atomicAdd(&end2[u], own);
        }
    } else {
        sq_walk(P, X, j0, j1, wv, nw, lane, [&](int32_t, int32_t w) { T.ctr[w] = 0; return (cc_word) 0; }, nothing);
    }
    if (STEP != SQ_STEP_ZERO) sq_tally(mine, MODE, lane, out);
}

// ------------------------------------------------------------------ host
// the plan's additions, once per plan (the symmetric adjacency is there)
static int sq_prepare(tcd_plan* p) {
    if (p->sq_ready) return GMX_OK;
    const int64_t V = p->V, U = p->E_up;
    const size_t bytes = ((size_t) U + 2 * (size_t) V) * sizeof(int32_t);
    if (p->sq_excl.alloc((size_t) U) || p->sq_W.alloc((size_t) V) || p->sq_vtx.alloc((size_t) V)) {
        const std::string why = gmx_last_error();
        p->sq_excl.release();
        p->sq_W.release();
        p->sq_vtx.release();
        gmx_set_error("squares: the wedge prefixes of %lld edges and the class list of %lld vertices need %zu bytes: %s", (long long) U, (long long) V, bytes, why.c_str());
        return GMX_ERR_NOMEM;
    }
    hipStream_t s = 0;
    gmx_ws_scope scope;
    wbuf<uint32_t> key, key2;
    wbuf<cc_word> wedges;
    size_t tb = 0;   // the sort's temporary storage, once the sort knows it
    int rc = key.alloc((size_t) V) || key2.alloc((size_t) V) || wedges.alloc(1) ? GMX_ERR_NOMEM : GMX_OK;
    if (rc == GMX_OK) {
        GMX_HIP(hipMemsetAsync(wedges.p, 0, sizeof(cc_word), s));
        hipLaunchKernelGGL(sq_prefix_kernel, dim3(grid_for(V, SQ_THREADS / 64, 256 * 16)), dim3(SQ_THREADS), 0, s, (const int32_t*) p->nb_begin.p,
                           (const int32_t*) p->nb_idx.p, (const int32_t*) p->up_begin.p, V, p->sq_excl.p, p->sq_W.p, key.p, wedges.p);
        rc = tcd_sort_by_key(key.p, key2.p, p->sq_vtx.p, V, 32u, s, &tb);
    }
    GMX_CHECK(cc_sort_nomem(rc, "squares", "their wedges", V, 3 * (size_t) V * sizeof(int32_t) + sizeof(cc_word), tb));
    p->sq_key.assign((size_t) V, 0);
    cc_word h = 0;
    GMX_HIP(hipMemcpy(p->sq_key.data(), key2.p, (size_t) V * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GMX_HIP(hipMemcpy(&h, wedges.p, sizeof(h), hipMemcpyDeviceToHost));
    p->sq_wedges = (int64_t) h;
    p->sq_ready = true;
    return GMX_OK;
}

struct sq_launch {   // what every class's launch shares
    sq_graph P;
    const int32_t* list;
    int mode;
    cc_word* mid;
    cc_word* end2;
    cc_word* out;
};

static int sq_launch_wave(const sq_launch& L, int64_t lo, int64_t hi) {
    const int64_t n = hi - lo;
    return cc_with_mode(L.mode, [&](auto mode) -> int {
        hipLaunchKernelGGL(sq_wave_kernel<decltype(mode)::value>, dim3(grid_for(n, SQ_WAVES, 256 * 8)), dim3(SQ_WAVES * 64), 0, 0, L.P, L.list + lo, n, L.mid, L.end2, L.out);
        GMX_HIP(hipGetLastError());
        return GMX_OK;
    });
}

static int sq_launch_block(const sq_launch& L, int64_t lo, int64_t hi, int slots) {
    const int64_t n = hi - lo;
    const size_t lds = (size_t) slots * 2 * sizeof(int32_t);
    return cc_with_mode(L.mode, [&](auto mode) -> int {
        constexpr int MODE = decltype(mode)::value;
        if (lds > 64 * 1024)   // (above 64 KiB a kernel has to be told)
            GMX_HIP(hipFuncSetAttribute((const void*) sq_block_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        hipLaunchKernelGGL(sq_block_kernel<MODE>, dim3(grid_for(n, 1, 256 * 8)), dim3(SQ_BLOCK_THREADS), lds, 0, L.P, L.list + lo, n, (uint32_t) slots, L.mid, L.end2, L.out);
        GMX_HIP(hipGetLastError());
        return GMX_OK;
    });
}

// one step of a batch over the list's [lo, hi), the batch's slots [off, off + hi - lo), `parts` workgroups a vertex at most
static int sq_launch_global(const sq_launch& L, int step, int64_t lo, int64_t hi, int64_t off, int parts, int64_t split, int32_t* ws, int64_t stride) {
    if (hi <= lo) return GMX_OK;
    return cc_with_mode(L.mode, [&](auto mode) -> int {
        return cc_with_mode(step, [&](auto step_c) -> int {   // (three steps: the same ladder)
            hipLaunchKernelGGL((sq_global_kernel<decltype(mode)::value, decltype(step_c)::value>), dim3((unsigned) (hi - lo), (unsigned) parts), dim3(SQ_BLOCK_THREADS), 0, 0,
                               L.P, L.list + lo, split, ws, off, stride, L.mid, L.end2, L.out);
            GMX_HIP(hipGetLastError());
            return GMX_OK;
        });
    });
}

// the thresholds of a call (gmx_squares: its knobs; sq_count_into: the defaults)
struct sq_knobs {
    int64_t wave_max = SQ_WAVE_MAX;
    int lds_slots = SQ_LDS_SLOTS;
    int64_t batch_bytes = SQ_BATCH_BYTES, split = SQ_SPLIT;
};
// the global class's batches: [lo, hi) of the list, every vertex with as many counters as the batch's highest id needs
// (whole 256-byte lines); [mid, hi) are the vertices that are cut into up to `parts` workgroups
struct sq_batch { int64_t lo, mid, hi, stride; int parts; };
struct sq_classes {   // the classes of a call, as ranges of the list: [p0, p1) wave, [p1, p2) block, [p2, V) global
    int64_t p0 = 0, p1 = 0, p2 = 0, n_split = 0;
    std::vector<sq_batch> batches;
    size_t ws_words = 0;   // int32 counters of the largest batch
};

// the classes under the thresholds K: key 0 = skipped, else W + 1
static int sq_classify(tcd_plan* p, const sq_knobs& K, sq_classes* C) {
    const int64_t V = p->V;
    const std::vector<uint32_t>& key = p->sq_key;
    auto below = [&](int64_t k) -> int64_t { return std::lower_bound(key.begin(), key.end(), (uint32_t) std::min<int64_t>(k, UINT32_MAX)) - key.begin(); };
    const int64_t p0 = below(1), p1 = K.wave_max > 0 ? below(K.wave_max + 2) : p0, p2 = std::max(p1, below((int64_t) K.lds_slots / 2 + 2));
    const int64_t n_global = V - p2;
    C->p0 = p0;
    C->p1 = p1;
    C->p2 = p2;
    if (n_global > 0) {
        std::vector<int32_t> ug((size_t) n_global);
        GMX_HIP(hipMemcpy(ug.data(), p->sq_vtx.p + p2, (size_t) n_global * sizeof(int32_t), hipMemcpyDeviceToHost));
        std::vector<cc_batch> cut;
        C->ws_words = (size_t) cc_plan_batches(p2, V, [&](int64_t i) { return (std::max<int64_t>(ug[i - p2], 1) + 63) & ~(int64_t) 63; },
                                               K.batch_bytes / (int64_t) sizeof(int32_t), &cut);
        for (const cc_batch& b : cut) {
            int64_t m = b.hi;   // W ascends along the list: the vertices to cut are a suffix
            while (m > b.lo && (int64_t) key[m - 1] - 1 > K.split) m--;
            C->n_split += b.hi - m;
            C->batches.push_back({b.lo, m, b.hi, b.stride, sq_parts((int64_t) key[b.hi - 1] - 1, INT32_MAX, K.split)});
        }
    }
    return GMX_OK;
}

// every class's launches; ws: the global class's counters, all zero.  ph_ms[1 .. 3]: wave, block, global (GMX_SQUARES_PHASES)
static int sq_run(const sq_launch& L, const sq_classes& C, const sq_knobs& K, int32_t* ws, gmx_phase_clock* phase, float* ph_ms) {
    phase->begin();
    if (C.p1 > C.p0) GMX_CHECK(sq_launch_wave(L, C.p0, C.p1));
    phase->end(&ph_ms[1]);
    phase->begin();
    if (C.p2 > C.p1) GMX_CHECK(sq_launch_block(L, C.p1, C.p2, K.lds_slots));
    phase->end(&ph_ms[2]);
    phase->begin();
    for (const sq_batch& b : C.batches)
        for (int step = SQ_STEP_COUNT; step <= SQ_STEP_ZERO; step++) {
            if (step == SQ_STEP_CREDIT && L.mode == CC_NONE) continue;
            GMX_CHECK(sq_launch_global(L, step, b.lo, b.mid, 0, 1, K.split, ws, b.stride));
            GMX_CHECK(sq_launch_global(L, step, b.mid, b.hi, b.mid - b.lo, b.parts, K.split, ws, b.stride));
        }
    phase->end(&ph_ms[3]);
    return GMX_OK;
}

// gmx_squares' walk for another entry on the plan (gmx_classcount.h): the adjacency is there
int sq_count_into(tcd_plan* p, int mode, cc_word* mid, cc_word* end2, cc_word* total2, bool* classes_built) {
    *classes_built = !p->sq_ready;
    GMX_CHECK(sq_prepare(p));
    const sq_knobs K;
    sq_classes Cl;
    GMX_CHECK(sq_classify(p, K, &Cl));
    gmx_ws_scope scope;
    wbuf<int32_t> ws;
    if (Cl.ws_words && ws.alloc(Cl.ws_words)) {
        const std::string why = gmx_last_error();
        gmx_set_error("squares: the global class's counters need %zu bytes: %s", Cl.ws_words * sizeof(int32_t), why.c_str());
        return GMX_ERR_NOMEM;
    }
    if (Cl.ws_words) GMX_HIP(hipMemsetAsync(ws.p, 0, Cl.ws_words * sizeof(int32_t), 0));
    static_assert(SQ_TOTAL == 0 && SQ_TOTAL2 == 1, "total2[] is the front of the sums");
    const sq_launch L = {{p->nb_begin.p, p->nb_idx.p, p->up_begin.p, p->sq_excl.p, p->sq_W.p}, p->sq_vtx.p, mode, mid, end2, total2};
    gmx_phase_clock off;
    float ph_ms[4] = {0, 0, 0, 0};
    return sq_run(L, Cl, K, ws.p, &off, ph_ms);
}

extern "C" int gmx_squares(gmx_graph_t* g, int64_t* count_host, int64_t* squares, gmx_stats_t* stats) {
    GMX_REQUIRE(squares, "NULL squares");
    GMX_REQUIRE(g, "NULL graph");
    if (stats) memset(stats, 0, sizeof(*stats));
    *squares = 0;
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    // knobs, read at every call; no result byte depends on them
    const bool ordered = !getenv("GMX_SQUARES_NO_ORDER");
    sq_knobs K;
    K.wave_max = gmx_env_int("GMX_SQUARES_WAVE_MAX", SQ_WAVE_MAX, 0, SQ_WAVE_SLOTS / 2);
    K.lds_slots = (int) gmx_env_int("GMX_SQUARES_LDS_SLOTS", SQ_LDS_SLOTS, SQ_LDS_SLOTS_MIN, SQ_LDS_SLOTS_MAX);
    K.batch_bytes = gmx_env_int("GMX_SQUARES_BATCH_BYTES", SQ_BATCH_BYTES, 1, INT64_MAX);
    K.split = gmx_env_int("GMX_SQUARES_SPLIT", SQ_SPLIT, 1, INT64_MAX);
    const bool plain = getenv("GMX_SQUARES_PLAIN") != nullptr;
    const bool phase_log = getenv("GMX_SQUARES_PHASES") != nullptr;
    const int mode = !count_host ? CC_NONE : plain ? CC_PLAIN : CC_LOCAL;
    bool empty = false;
    GMX_CHECK(cc_answer_empty(g, count_host, stats, &empty));
    if (empty) return GMX_OK;
    // graph preprocessing (cached on the graph, shared with the other entries on the plan; outside the timed region)
    bool built = false;
    tcd_plan* p = nullptr;
    GMX_CHECK(tcd_plan_get(g, ordered, &p, &built));
    float ph_ms[5] = {0, 0, 0, 0, 0};   // plan additions, wave, block, global, finish (GMX_SQUARES_PHASES)
    gmx_phase_clock phase;
    GMX_CHECK(phase.enable(phase_log));
    const bool adj_built = !p->kt_ready, classes_built = !p->sq_ready;
    phase.begin();
    GMX_CHECK(tcd_plan_adjacency(p));
    GMX_CHECK(sq_prepare(p));
    phase.end(&ph_ms[0]);

    sq_classes Cl;
    GMX_CHECK(sq_classify(p, K, &Cl));
    const int64_t p0 = Cl.p0, n_wave = Cl.p1 - Cl.p0, n_block = Cl.p2 - Cl.p1, n_global = V - Cl.p2, n_split = Cl.n_split;
    const std::vector<sq_batch>& batches = Cl.batches;
    const size_t ws_words = Cl.ws_words;
    // the call's scratch: the two accumulators in the plan's numbering, the array asked for, the sums, the global class's counters
    cc_scratch S;
    GMX_CHECK(S.alloc(SQ_NCTR, count_host != nullptr, 2, V, ws_words * sizeof(int32_t), "squares: the per-vertex scratch and the global class's counters need %zu bytes: %s"));
    cc_word* const mid = S.acc.p;
    cc_word* const end2 = S.acc.p ? S.acc.p + V : nullptr;
    int32_t* const ws = (int32_t*) S.ws.p;
    const sq_launch L = {{p->nb_begin.p, p->nb_idx.p, p->up_begin.p, p->sq_excl.p, p->sq_W.p}, p->sq_vtx.p, mode, mid, end2, S.out.p};
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.KERNEL));
    if (count_host) GMX_HIP(hipMemsetAsync(mid, 0, 2 * (size_t) V * sizeof(cc_word), 0));
    if (ws_words) GMX_HIP(hipMemsetAsync(ws, 0, ws_words * sizeof(int32_t), 0));   // (once: every batch leaves its counters zero)
    GMX_CHECK(sq_run(L, Cl, K, ws, &phase, ph_ms));
    phase.begin();
    if (count_host) {
        hipLaunchKernelGGL(cc_finish_kernel, dim3(grid_for(V)), dim3(CC_THREADS), 0, 0, (const cc_word*) mid, (const cc_word*) end2, (const int32_t*) p->perm.p, V,
                           S.cnt_out.p, S.out.p + SQ_NONZERO, S.out.p + SQ_SUM);
        GMX_HIP(hipGetLastError());
    }
    phase.end(&ph_ms[4]);
    cc_word h[SQ_NCTR];
    GMX_CHECK(cc_read_back(tm, S, h, SQ_NCTR, V, count_host, stats));
    const cc_word total = h[SQ_TOTAL] + h[SQ_TOTAL2] / 2;
    GMX_CHECK(cc_check("squares", count_host != nullptr, h[SQ_SUM], 4, total, h[SQ_NONZERO], p->sq_wedges, stats));
    *squares = (int64_t) total;
    if (phase_log)
        fprintf(stderr, "gmx squares phases: plan %.3f ms, wave %.3f ms, block %.3f ms, global %.3f ms, finish %.3f ms\n", ph_ms[0], ph_ms[1], ph_ms[2], ph_ms[3],
                ph_ms[4]);
    if (getenv("GMX_SQUARES_LOG"))   // one line per call (tools/squares_prof.py and the tests parse it)
        fprintf(stderr, "gmx squares: plan V %lld E %lld up %lld order %s built %d adj_built %d classes_built %d; wave_max %lld lds_slots %d split %lld "
                        "batch_bytes %lld counts %s; items %lld wave + %lld block + %lld global (%lld split) + %lld skipped; wedges %lld batches %zu squares %llu\n",
                (long long) p->V, (long long) p->E, (long long) p->E_up, p->ordered ? "degree" : "identity", built ? 1 : 0, adj_built ? 1 : 0, classes_built ? 1 : 0,
                (long long) K.wave_max, K.lds_slots, (long long) K.split, (long long) K.batch_bytes, cc_mode_word(mode),
                (long long) n_wave, (long long) n_block, (long long) n_global, (long long) n_split, (long long) p0, (long long) p->sq_wedges, batches.size(), total);
    return GMX_OK;
}

void gmx_touch_squares() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) sq_wave_kernel<CC_LOCAL>);
}
