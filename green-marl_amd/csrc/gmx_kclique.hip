// gmx_kclique.hip -- k-clique counts, in total and through every vertex, for gfx950: gmx_kclique (3 <= k <= 8).  The
// reference has no such program; the definition, the method and the statistics are the contract at gmx_kclique in gmx.h.
//
// The stored slots are read as gmx_clustering reads them, N(v) = { u != v : v -> u or u -> v is stored }, on the plan of
// gmx_tcd.hip (cached on the graph, shared with gmx_triangle_counting_directed, gmx_clustering and gmx_ktruss): perm and UP',
// per vertex the distinct neighbours above it in the plan's numbering, sorted.  A k-clique is found exactly once, at its
// lowest plan id v, as a (k-1)-clique among S = UP'(v):
//   matrix   local index i = position in S; row i is the bit set A[i] = { j > i : S_j in UP'(S_i) }, W = ceil(d / 64) words of
//            64 bits, d = |S|.  UP'(S_i) is streamed and every entry (up to the last of S) searched in S.
//   count    P_1 = all; choose i_1, P_2 = A[i_1]; choose i_2 in P_2, P_3 = P_2 & A[i_2]; ... after k - 2 choices the last set is
//            only popcounted.  Rows only hold bits above their own index, so the walk below a choice j starts at word j / 64.
//            Rows of several words (small, large, global): nothing but the chosen indices is kept, a word of P_t is the AND
//            of the chosen rows' words (at most six), recomputed where it is read.  Rows of one word (wave): P_t itself goes
//            down the walk in a register.
//   credits  a chosen index gets its subtree's total when the walk returns, the members of the last set +1 each, v the
//            vertex total.  The first two go to 64-bit counters per local index (LDS; the global class: workspace memory) that
//            are flushed once per vertex to cnt[], which is held in plan ids and permuted back by the finishing kernel.
//            count_host == NULL: no counters and no enumeration of the last set at all.
// Size classes, one launch each (the global class: one per batch), over the plan's list of the vertices by ascending d:
//   wave     d <= 64: W = 1; a wave per vertex, list, rows and counters in the wave's LDS slice (1280 bytes); LANE i owns
//            i_1 = i and walks its subtree by itself.
//   small    d <= min(256, cap) and large  d <= cap: a workgroup per vertex (256 and 1024 threads), matrix, counters and list
//            in dynamic LDS (11 KiB and 140 KiB); a WAVE owns i_1, its lanes take the i_2 of A[i_1] and each walks the rest by
//            itself (k = 3 has no i_2: a thread per i_1).  A class of few vertices gives each of them to several workgroups,
//            which all build the matrix and share the i_1, so that the machine is filled.
//   global   d > cap: the large class's kernel with matrix and counters in workspace memory, one workgroup per vertex, dealt in
//            batches of at most GMX_KCLIQUE_BATCH_BYTES (zeroed by a memset in front of the batch's launch).
//   skipped  d < k - 1: never launched.
// Every loop ends by construction (a list, a row or a word range is walked once); no kernel waits for another workgroup.
// Integers only: every result is unique and the same bytes under every knob.
// The credit modes, the mode dispatch, the batches, the finishing kernel and the frame of the entry are gmx_classcount.h's,
// shared with gmx_squares.hip.
#include "gmx_classcount.h"

#define KC_THREADS 256
#define KC_WAVES 4               // waves of a wave-class workgroup
#define KC_WAVE_D 64             // wave class: d <= 64
#define KC_SMALL_D 256           // small class: d <= 256
#define KC_CAP 1024              // GMX_KCLIQUE_CAP: large class: d <= cap
#define KC_CAP_MIN 64
#define KC_SMALL_THREADS 256
#define KC_LARGE_THREADS 1024
#define KC_SMALL_GRID (256 * 16) // small class: workgroups of a launch at most.  4 waves a workgroup and 110 - 123 VGPRs (4 waves a SIMD) put 4 of them
                                 // on a CU, 1024 on the MI355X's 256 CUs: four rounds of that.  NOT MEASURED
#define KC_SMALL_SPLIT 32        // ... and at most this many workgroups share a vertex when the class has few.  NOT MEASURED
#define KC_LARGE_GRID 256        // large class: 140 KiB of LDS, a workgroup per CU; the MI355X's 256 CUs as a constant (as gmx_lcc.hip's grid), not
                                 // asked of the device: on another CU count the grid-stride loop is still right, only the fill differs
#define KC_LARGE_SPLIT 16        // NOT MEASURED
#define KC_ALONE 16              // wave class, matrix: a lane walks an UP'(S_i) of up to this many entries by itself.  NOT MEASURED
#define KC_BATCH_BYTES (256LL << 20)   // GMX_KCLIQUE_BATCH_BYTES: matrices and counters of one global-class launch.  NOT MEASURED
#define KC_MAX_K 8
#define KC_ROWS (KC_MAX_K - 2)   // chosen indices at most

enum { KC_TOTAL, KC_NONZERO, KC_SUM, KC_NCTR };
enum { KC_SMALL, KC_LARGE, KC_GLOBAL };   // KIND of a workgroup kernel

// n credits for local index j (MODE: gmx_classcount.h's; CC_LOCAL: the counters ctr[])
template <int MODE>
__device__ __forceinline__ void kc_credit(cc_word* ctr, cc_word* __restrict__ cnt, const int32_t* S, int32_t j, cc_word n) {
    if (MODE == CC_LOCAL) atomicAdd(&ctr[j], n);
    if (MODE == CC_PLAIN) atomicAdd(&cnt[S[j]], n);
}

// The walk below N chosen rows ro[0 .. N) (offsets into A), LEFT more indices to choose before the popcount; `from` = the
// word of the last chosen index.  Returns the cliques found; the chosen indices and the last set's members are credited.
template <int LEFT, int N, int MODE>
__device__ __forceinline__ cc_word kc_walk(const cc_word* A, int32_t W, int32_t (&ro)[KC_ROWS], int32_t from, cc_word* ctr, cc_word* __restrict__ cnt,
                                           const int32_t* S) {
    cc_word total = 0;
    for (int32_t w = from; w < W; w++) {
        cc_word x = A[ro[0] + w];
#pragma unroll
        for (int s = 1; s < N; s++) x &= A[ro[s] + w];
        if constexpr (LEFT == 0) {
            total += (cc_word) __popcll(x);
            if (MODE != CC_NONE)
                while (x) {
                    const int32_t j = w * 64 + __builtin_ctzll(x);
                    x &= x - 1;
                    kc_credit<MODE>(ctr, cnt, S, j, 1);
                }
        } else {
            while (x) {
                const int32_t j = w * 64 + __builtin_ctzll(x);
                x &= x - 1;
                ro[N] = j * W;
                const cc_word sub = kc_walk<LEFT - 1, N + 1, MODE>(A, W, ro, w, ctr, cnt, S);
                total += sub;
                if (MODE != CC_NONE && sub) kc_credit<MODE>(ctr, cnt, S, j, sub);
            }
        }
    }
    return total;
}

// the same with LEFT = left known at run time (N + left <= KC_ROWS: the caller's k <= 8)
template <int N, int MODE>
__device__ __forceinline__ cc_word kc_walk_from(int left, const cc_word* A, int32_t W, int32_t (&ro)[KC_ROWS], int32_t from, cc_word* ctr,
                                                cc_word* __restrict__ cnt, const int32_t* S) {
    switch (left) {
    case 0: return kc_walk<0, N, MODE>(A, W, ro, from, ctr, cnt, S);
    case 1: return kc_walk<1, N, MODE>(A, W, ro, from, ctr, cnt, S);
    case 2: return kc_walk<2, N, MODE>(A, W, ro, from, ctr, cnt, S);
    case 3: return kc_walk<3, N, MODE>(A, W, ro, from, ctr, cnt, S);
    case 4: return kc_walk<4, N, MODE>(A, W, ro, from, ctr, cnt, S);
    default:
        if constexpr (N + 5 <= KC_ROWS) return kc_walk<5, N, MODE>(A, W, ro, from, ctr, cnt, S);
        return 0;
    }
}

// The same walk for rows of ONE word (the wave class): the candidate set itself, x = the AND of the chosen rows, goes down in
// a register instead of the chosen rows, so a level costs one row read.  LEFT more indices to choose before x is popcounted.
template <int LEFT, int MODE>
__device__ __forceinline__ cc_word kc_walk_word(const cc_word* A, cc_word x, cc_word* ctr, cc_word* __restrict__ cnt, const int32_t* S) {
    if constexpr (LEFT == 0) {
        const cc_word total = (cc_word) __popcll(x);
        if (MODE != CC_NONE)
            while (x) {
                const int32_t j = __builtin_ctzll(x);
                x &= x - 1;
                kc_credit<MODE>(ctr, cnt, S, j, 1);
            }
        return total;
    } else {
        cc_word total = 0;
        while (x) {
            const int32_t j = __builtin_ctzll(x);
            x &= x - 1;
            const cc_word sub = kc_walk_word<LEFT - 1, MODE>(A, x & A[j], ctr, cnt, S);   // (row j holds bits above j only)
            total += sub;
            if (MODE != CC_NONE && sub) kc_credit<MODE>(ctr, cnt, S, j, sub);
        }
        return total;
    }
}
template <int MODE>
__device__ __forceinline__ cc_word kc_walk_word_from(int left, const cc_word* A, cc_word x, cc_word* ctr, cc_word* __restrict__ cnt, const int32_t* S) {
    switch (left) {
    case 0: return kc_walk_word<0, MODE>(A, x, ctr, cnt, S);
    case 1: return kc_walk_word<1, MODE>(A, x, ctr, cnt, S);
    case 2: return kc_walk_word<2, MODE>(A, x, ctr, cnt, S);
    case 3: return kc_walk_word<3, MODE>(A, x, ctr, cnt, S);
    case 4: return kc_walk_word<4, MODE>(A, x, ctr, cnt, S);
    default: return kc_walk_word<5, MODE>(A, x, ctr, cnt, S);
    }
}

// ------------------------------------------------------------------ the plan's additions
__global__ void __launch_bounds__(KC_THREADS) kc_len_kernel(const int32_t* __restrict__ up_begin, int64_t V, uint32_t* __restrict__ d) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) d[v] = (uint32_t) (up_begin[v + 1] - up_begin[v]);
}
// below[t] = the entries of the ascending d[0, V) that are < t, t < n
__global__ void __launch_bounds__(KC_THREADS) kc_below_kernel(const int32_t* __restrict__ d, int64_t V, int n, int64_t* __restrict__ below) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int64_t lo = 0, hi = V;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (d[mid] < t) lo = mid + 1; else hi = mid;
    }
    below[t] = lo;
}

// ------------------------------------------------------------------ wave class
// list[0, n): vertices with k - 1 <= d <= 64.  A wave per vertex; lane i holds S_i, builds or shares in building row i and
// walks the subtree of i_1 = i.
template <int MODE>
__global__ void __launch_bounds__(KC_WAVES * 64) kc_wave_kernel(const int32_t* __restrict__ up_begin, const int32_t* __restrict__ up_idx,
                                                                const int32_t* __restrict__ list, int64_t n, int k, int alone_max, int only_build,
                                                                cc_word* __restrict__ cnt /* [V] by plan id, or NULL */, cc_word* __restrict__ out) {
    __shared__ cc_word s_A[KC_WAVES][64];
    __shared__ cc_word s_c[KC_WAVES][64];
    __shared__ int32_t s_S[KC_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    cc_word* A = s_A[wv];
    cc_word* c = s_c[wv];
    int32_t* S = s_S[wv];
    c[lane] = 0;
    cc_word total = 0;
    const int64_t nwaves = (int64_t) gridDim.x * KC_WAVES;
    for (int64_t it = (int64_t) blockIdx.x * KC_WAVES + wv; it < n; it += nwaves) {   // (wave-uniform)
        const int32_t v = list[it];
        const int32_t ab = up_begin[v], d = up_begin[v + 1] - ab;   // 2 <= d <= 64
        const bool act = lane < d;
        int32_t u = 0, bb = 0, be = 0;
        if (act) {
            u = up_idx[ab + lane];
            bb = up_begin[u];
            be = up_begin[u + 1];
        }
        S[lane] = act ? u : INT32_MAX;
        rg_lds_landed();     // the wave's own LDS writes are visible to all its lanes
        const int32_t last = S[d - 1];
        // the matrix: a short UP'(S_i) by lane i alone, the others one after the other by the whole wave
        const bool by_wave = act && be - bb > alone_max;
        cc_word row = 0;
        if (act && !by_wave)
            for (int32_t p = bb; p < be; p++) {
                const int32_t w = up_idx[p];
                if (w > last) break;
                const int32_t f = rg_lower_bound<true>(S, lane + 1, d, w);
                if (f < d && S[f] == w) row |= 1ull << f;
            }
        A[lane] = row;
        rg_lds_landed();
        unsigned long long m = __ballot(by_wave);
        while (m) {   // (the same trip counts in every lane)
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t sbb = __builtin_amdgcn_readlane(bb, src), sbe = __builtin_amdgcn_readlane(be, src);
            for (int32_t p0 = sbb; p0 < sbe; p0 += 64) {
                const int32_t p = p0 + lane;
                const int32_t w = p < sbe ? up_idx[p] : INT32_MAX;
                if (w <= last) {
                    const int32_t f = rg_lower_bound<true>(S, src + 1, d, w);
                    if (f < d && S[f] == w) atomicOr(&A[src], 1ull << f);
                }
                if (__builtin_amdgcn_readfirstlane(w) > last) break;   // (lane 0 has p < sbe) sorted: nothing further is in S
            }
        }
        rg_lds_landed();     // the wave's own LDS atomics have landed
        if (!only_build) {
            cc_word mine = 0;
            if (act) {
                mine = kc_walk_word_from<MODE>(k - 3, A, A[lane], c, cnt, S);
                if (MODE != CC_NONE && mine) kc_credit<MODE>(c, cnt, S, lane, mine);
            }
            const cc_word tot = cc_wave_total(mine);
            total += tot;
            if (MODE != CC_NONE) {
                if (lane == 0 && tot) atomicAdd(&cnt[v], tot);
                if (MODE == CC_LOCAL) {   // flush the counters and leave them zero
                    rg_lds_landed();
                    const cc_word cv = c[lane];
                    if (cv) {   // (only a lane < d can hold credits)
                        c[lane] = 0;
                        atomicAdd(&cnt[u], cv);
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();        // all lanes are done with S and A before they are overwritten
    }
    if (lane == 0 && total) atomicAdd(&out[KC_TOTAL], total);
}

// ------------------------------------------------------------------ small, large and global classes
// dynamic LDS of a workgroup whose vertices have d <= dmax (a multiple of 64): matrix, counters, list
static size_t kc_lds_bytes(int dmax) { return (size_t) dmax * (dmax >> 6) * sizeof(cc_word) + (size_t) dmax * sizeof(cc_word) + (size_t) dmax * sizeof(int32_t); }
// global class: 64-bit words of the matrix and the counters of a vertex of d upper neighbours, in whole 256-byte lines
static int64_t kc_ws_words(int64_t d) { return (d * ((d + 63) >> 6) + d + 31) & ~(int64_t) 31; }

// list[0, n): a vertex goes to `split` workgroups (work item it = vertex it / split, share it % split), each of which builds the
// matrix for itself and takes every split-th of the i_1 its waves (k == 3: threads) would own: few vertices still fill the
// machine.  GLOBAL: split == 1, n == gridDim.x, vertex b's matrix and counters at ws + b * ws_stride, all zero.
// A wave owns i_1, its lanes the i_2 of A[i_1]; k == 3: a thread per i_1.
template <int MODE, int KIND>
__global__ void __launch_bounds__(KIND == KC_SMALL ? KC_SMALL_THREADS : KC_LARGE_THREADS) kc_block_kernel(const int32_t* __restrict__ up_begin, const int32_t* __restrict__ up_idx,
                                                                    const int32_t* __restrict__ list, int64_t n, int split, int k, int dmax, int only_build,
                                                                    cc_word* __restrict__ ws, int64_t ws_stride, cc_word* __restrict__ cnt,
                                                                    cc_word* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kc_lds[];
    constexpr bool GLOBAL = KIND == KC_GLOBAL;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, T = blockDim.x, nwaves = T >> 6;
    cc_word* A = GLOBAL ? nullptr : (cc_word*) kc_lds;
    cc_word* c = GLOBAL ? nullptr : A + (size_t) dmax * (dmax >> 6);
    int32_t* S_lds = GLOBAL ? nullptr : (int32_t*) (c + dmax);
    if (!GLOBAL) {
        for (int j = tid; j < dmax; j += T) c[j] = 0;
        __syncthreads();
    }
    cc_word total = 0;
    for (int64_t it = blockIdx.x; it < n * split; it += gridDim.x) {   // (workgroup-uniform)
        const int32_t v = list[it / split], share = (int32_t) (it % split);
        const int32_t ab = up_begin[v], d = up_begin[v + 1] - ab, W = (d + 63) >> 6;
        const int32_t* S = GLOBAL ? up_idx + ab : S_lds;
        if (GLOBAL) {
            A = ws + it * ws_stride;
            c = A + (int64_t) d * W;
        } else {
            for (int32_t j = tid; j < d; j += T) S_lds[j] = up_idx[ab + j];
            for (int32_t x = tid; x < d * W; x += T) A[x] = 0;
            __syncthreads();
        }
        const int32_t last = S[d - 1];
        // the matrix: a wave streams UP'(S_i)
        for (int32_t i = wv; i < d; i += nwaves) {   // (wave-uniform)
            const int32_t u = S[i], bb = up_begin[u], be = up_begin[u + 1];
            for (int32_t p0 = bb; p0 < be; p0 += 64) {
                const int32_t p = p0 + lane;
                const int32_t w = p < be ? up_idx[p] : INT32_MAX;
                if (w <= last) {
                    const int32_t f = rg_lower_bound<true>(S, i + 1, d, w);
                    if (f < d && S[f] == w) atomicOr(&A[i * W + (f >> 6)], 1ull << (f & 63));
                }
                if (__builtin_amdgcn_readfirstlane(w) > last) break;   // (lane 0 has p < be) sorted: nothing further is in S
            }
        }
        if (GLOBAL) __threadfence();
        __syncthreads();
        if (!only_build) {
            cc_word vsum = 0;   // the wave's share of the vertex total (the same in every lane)
            if (k == 3) {
                cc_word mine = 0;
                for (int32_t i = share * T + tid; i < d; i += split * T) {
                    int32_t ro[KC_ROWS] = {i * W, 0, 0, 0, 0, 0};
                    const cc_word t = kc_walk<0, 1, MODE>(A, W, ro, i >> 6, c, cnt, S);   // (one row: nothing to hand down)
                    if (MODE != CC_NONE && t) kc_credit<MODE>(c, cnt, S, i, t);
                    mine += t;
                }
                vsum = cc_wave_total(mine);
            } else {
                for (int32_t i = share * nwaves + wv; i < d; i += split * nwaves) {   // (wave-uniform)
                    cc_word mine = 0;
                    for (int32_t j = i + 1 + lane; j < d; j += 64) {
                        if (!((A[i * W + (j >> 6)] >> (j & 63)) & 1ull)) continue;
                        int32_t ro[KC_ROWS] = {i * W, j * W, 0, 0, 0, 0};
                        const cc_word sub = kc_walk_from<2, MODE>(k - 4, A, W, ro, j >> 6, c, cnt, S);
                        if (MODE != CC_NONE && sub) kc_credit<MODE>(c, cnt, S, j, sub);
                        mine += sub;
                    }
                    const cc_word tot = cc_wave_total(mine);
                    if (MODE != CC_NONE && lane == 0 && tot) kc_credit<MODE>(c, cnt, S, i, tot);
                    vsum += tot;
                }
            }
            total += vsum;
            if (MODE != CC_NONE && lane == 0 && vsum) atomicAdd(&cnt[v], vsum);
            if (MODE == CC_LOCAL) {   // flush the counters (LDS: and leave them zero)
                if (GLOBAL) __threadfence();
                __syncthreads();
                for (int32_t j = tid; j < d; j += T) {
                    const cc_word cv = GLOBAL ? __hip_atomic_load(&c[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : c[j];
                    if (cv) {
                        if (!GLOBAL) c[j] = 0;
                        atomicAdd(&cnt[S[j]], cv);
                    }
                }
            }
        }
        __syncthreads();   // everybody is done with the list and the matrix before they are overwritten
    }
    if (lane == 0 && total) atomicAdd(&out[KC_TOTAL], total);
}

// ------------------------------------------------------------------ host
// the plan's additions, once per plan: the vertices by ascending d and where every d begins in that list
static int kc_prepare(tcd_plan* p) {
    if (p->kc_ready) return GMX_OK;
    const int64_t V = p->V;
    const size_t bytes = 2 * (size_t) V * sizeof(int32_t);
    if (p->kc_vtx.alloc((size_t) V) || p->kc_d.alloc((size_t) V)) {
        const std::string why = gmx_last_error();
        p->kc_vtx.release();
        p->kc_d.release();
        gmx_set_error("kclique: the size-class list of %lld vertices needs %zu bytes: %s", (long long) V, bytes, why.c_str());
        return GMX_ERR_NOMEM;
    }
    hipStream_t s = 0;
    gmx_ws_scope scope;
    wbuf<uint32_t> key;
    wbuf<int64_t> below;
    const int nb = KC_CAP + 2;
    size_t tb = 0;   // the sort's temporary storage, once the sort knows it
    int rc = key.alloc((size_t) V) || below.alloc((size_t) nb) ? GMX_ERR_NOMEM : GMX_OK;
    if (rc == GMX_OK) {
        hipLaunchKernelGGL(kc_len_kernel, dim3(grid_for(V)), dim3(KC_THREADS), 0, s, (const int32_t*) p->up_begin.p, V, key.p);
        rc = tcd_sort_by_key(key.p, (uint32_t*) p->kc_d.p, p->kc_vtx.p, V, (unsigned) gmx_bits_for(V + 1) /* d <= V - 1 */, s, &tb);
    }
    GMX_CHECK(cc_sort_nomem(rc, "kclique", "list length", V, 2 * (size_t) V * sizeof(int32_t) + (size_t) nb * sizeof(int64_t), tb));
    hipLaunchKernelGGL(kc_below_kernel, dim3((nb + KC_THREADS - 1) / KC_THREADS), dim3(KC_THREADS), 0, s, (const int32_t*) p->kc_d.p, V, nb, below.p);
    GMX_HIP(hipGetLastError());
    p->kc_below.assign((size_t) nb, 0);
    GMX_HIP(hipMemcpy(p->kc_below.data(), below.p, (size_t) nb * sizeof(int64_t), hipMemcpyDeviceToHost));
    p->kc_ready = true;
    return GMX_OK;
}

struct kc_launch {   // what every class's launch shares
    const int32_t* up_begin;
    const int32_t* up_idx;
    const int32_t* list;
    int k, mode;
    cc_word* cnt;
    cc_word* out;
};

static int kc_launch_wave(const kc_launch& L, int64_t lo, int64_t hi, int only_build) {
    const int64_t n = hi - lo;
    const dim3 grid(grid_for(n, KC_WAVES, 256 * 8)), block(KC_WAVES * 64);
    return cc_with_mode(L.mode, [&](auto mode) -> int {
        hipLaunchKernelGGL(kc_wave_kernel<decltype(mode)::value>, grid, block, 0, 0, L.up_begin, L.up_idx, L.list + lo, n, L.k, KC_ALONE, only_build, L.cnt, L.out);
        GMX_HIP(hipGetLastError());
        return GMX_OK;
    });
}

template <int KIND>
static int kc_launch_block(const kc_launch& L, int64_t lo, int64_t hi, int threads, int max_grid, int max_split, int dmax, int only_build, cc_word* ws,
                           int64_t ws_stride) {
    const int64_t n = hi - lo;
    // the shares of a vertex: as many as fill max_grid workgroups, at most max_split
    const int split = (int) std::max<int64_t>(1, std::min<int64_t>(max_split, max_grid / n));
    const int64_t items = n * split;
    const size_t lds = KIND == KC_GLOBAL ? 0 : kc_lds_bytes(dmax);
    return cc_with_mode(L.mode, [&](auto mode) -> int {
        constexpr int MODE = decltype(mode)::value;
        if (KIND == KC_LARGE)   // (above 64 KiB a kernel has to be told)
            GMX_HIP(hipFuncSetAttribute((const void*) kc_block_kernel<MODE, KIND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        hipLaunchKernelGGL((kc_block_kernel<MODE, KIND>), dim3((unsigned) (items < max_grid ? items : max_grid)), dim3(threads), lds, 0, L.up_begin, L.up_idx,
                           L.list + lo, n, split, L.k, dmax, only_build, ws, ws_stride, L.cnt, L.out);
        GMX_HIP(hipGetLastError());
        return GMX_OK;
    });
}

struct kc_classes {   // the classes of a call, as ranges of the list: [p0, p1) wave, [p1, p2) small, [p2, p3) large, [p3, V) global
    int64_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    std::vector<cc_batch> batches;   // the global class's: every vertex in a slot as large as the batch's last one needs (d ascends along the list)
    size_t ws_bytes = 0;
};

static int kc_classify(tcd_plan* p, int k, int cap, bool use_wave, int64_t batch_bytes, kc_classes* C) {
    const int64_t V = p->V;
    const std::vector<int64_t>& below = p->kc_below;
    const int small_hi = cap < KC_SMALL_D ? cap : KC_SMALL_D;
    const int64_t p0 = below[k - 1], p1 = use_wave ? below[KC_WAVE_D + 1] : p0, p2 = below[small_hi + 1], p3 = below[cap + 1];
    const int64_t n_global = V - p3;
    C->p0 = p0;
    C->p1 = p1;
    C->p2 = p2;
    C->p3 = p3;
    if (n_global > 0) {
        std::vector<int32_t> dg((size_t) n_global);
        GMX_HIP(hipMemcpy(dg.data(), p->kc_d.p + p3, (size_t) n_global * sizeof(int32_t), hipMemcpyDeviceToHost));
        // (only without the degree order, which bounds d by sqrt(2 |UP'|) < 2^16: the kernels keep row offsets in 32 bits)
        GMX_REQUIRE(kc_ws_words(dg.back()) <= INT32_MAX, "kclique: an upper list of %d entries: its bit matrix needs 32-bit row offsets", (int) dg.back());
        C->ws_bytes = sizeof(cc_word) * (size_t) cc_plan_batches(p3, V, [&](int64_t i) { return kc_ws_words(dg[i - p3]); }, batch_bytes / (int64_t) sizeof(cc_word), &C->batches);
    }
    return GMX_OK;
}

// every class's launches; ws: the global class's workspace.  ph_ms[1 .. 5]: matrices, wave, small, large, global (GMX_KCLIQUE_PHASES)
static int kc_run(const kc_launch& L, const kc_classes& C, cc_word* ws, bool phase_log, gmx_phase_clock* phase, float* ph_ms) {
    // a class's launch; under GMX_KCLIQUE_PHASES once more in front of it, stopping behind the matrix, to time that share
    auto timed = [&](int slot, auto&& launch) -> int {
        float tb = 0;
        if (phase_log) {
            phase->begin();
            GMX_CHECK(launch(1));
            tb = phase->end(&ph_ms[1]);
        }
        phase->begin();
        GMX_CHECK(launch(0));
        const float t = phase->end();
        ph_ms[slot] += t > tb ? t - tb : 0.f;
        return GMX_OK;
    };
    if (C.p1 > C.p0) GMX_CHECK(timed(2, [&](int only_build) -> int { return kc_launch_wave(L, C.p0, C.p1, only_build); }));
    if (C.p2 > C.p1)
        GMX_CHECK(timed(3, [&](int only_build) -> int { return kc_launch_block<KC_SMALL>(L, C.p1, C.p2, KC_SMALL_THREADS, KC_SMALL_GRID, KC_SMALL_SPLIT, KC_SMALL_D, only_build, nullptr, 0); }));
    if (C.p3 > C.p2)
        GMX_CHECK(timed(4, [&](int only_build) -> int { return kc_launch_block<KC_LARGE>(L, C.p2, C.p3, KC_LARGE_THREADS, KC_LARGE_GRID, KC_LARGE_SPLIT, KC_CAP, only_build, nullptr, 0); }));
    for (const cc_batch& b : C.batches)
        GMX_CHECK(timed(5, [&](int only_build) -> int {
            GMX_HIP(hipMemsetAsync(ws, 0, (size_t) ((b.hi - b.lo) * b.stride) * sizeof(cc_word), 0));
            return kc_launch_block<KC_GLOBAL>(L, b.lo, b.hi, KC_LARGE_THREADS, INT32_MAX, 1, 0, only_build, ws, b.stride);
        }));
    return GMX_OK;
}

// gmx_kclique's count for another entry on the plan (gmx_classcount.h), at the default thresholds
int kc_count_into(tcd_plan* p, int k, int mode, cc_word* cnt, cc_word* total, bool* classes_built) {
    *classes_built = !p->kc_ready;
    GMX_CHECK(kc_prepare(p));
    kc_classes Cl;
    GMX_CHECK(kc_classify(p, k, KC_CAP, true, KC_BATCH_BYTES, &Cl));
    gmx_ws_scope scope;
    wbuf<char> ws;
    if (Cl.ws_bytes && ws.alloc(Cl.ws_bytes)) {
        const std::string why = gmx_last_error();
        gmx_set_error("kclique: the global class's matrices need %zu bytes: %s", Cl.ws_bytes, why.c_str());
        return GMX_ERR_NOMEM;
    }
    static_assert(KC_TOTAL == 0, "total[] is the front of the sums");
    const kc_launch L = {p->up_begin.p, p->up_idx.p, p->kc_vtx.p, k, mode, cnt, total};
    gmx_phase_clock off;
    float ph_ms[6] = {0, 0, 0, 0, 0, 0};
    return kc_run(L, Cl, (cc_word*) ws.p, false, &off, ph_ms);
}

extern "C" int gmx_kclique(gmx_graph_t* g, int32_t k, int64_t* count_host, int64_t* cliques, gmx_stats_t* stats) {
    GMX_REQUIRE(cliques, "NULL cliques");
    GMX_REQUIRE(k >= 3 && k <= KC_MAX_K, "kclique: k = %d is outside 3 .. %d", (int) k, KC_MAX_K);
    GMX_REQUIRE(g, "NULL graph");
    if (stats) memset(stats, 0, sizeof(*stats));
    *cliques = 0;
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    // knobs, read at every call; no result byte depends on them
    const bool ordered = !getenv("GMX_KCLIQUE_NO_ORDER");
    const int cap = (int) gmx_env_int("GMX_KCLIQUE_CAP", KC_CAP, KC_CAP_MIN, KC_CAP);
    const bool use_wave = gmx_env_int("GMX_KCLIQUE_WAVE", 1, 0, 1) != 0;
    const int64_t batch_bytes = gmx_env_int("GMX_KCLIQUE_BATCH_BYTES", KC_BATCH_BYTES, 1, INT64_MAX);
    const bool plain = getenv("GMX_KCLIQUE_PLAIN") != nullptr;
    const bool phase_log = getenv("GMX_KCLIQUE_PHASES") != nullptr;
    const int mode = !count_host ? CC_NONE : plain ? CC_PLAIN : CC_LOCAL;
    bool empty = false;
    GMX_CHECK(cc_answer_empty(g, count_host, stats, &empty));
    if (empty) return GMX_OK;
    // graph preprocessing (cached on the graph, shared with gmx_triangle_counting_directed, gmx_clustering and gmx_ktruss; outside the timed region)
    bool built = false;
    tcd_plan* p = nullptr;
    GMX_CHECK(tcd_plan_get(g, ordered, &p, &built));
    float ph_ms[7] = {0, 0, 0, 0, 0, 0, 0};   // plan additions, matrices, wave, small, large, global, finish (GMX_KCLIQUE_PHASES)
    gmx_phase_clock phase;
    GMX_CHECK(phase.enable(phase_log));
    const bool classes_built = !p->kc_ready;
    phase.begin();
    GMX_CHECK(kc_prepare(p));
    phase.end(&ph_ms[0]);

    kc_classes Cl;
    GMX_CHECK(kc_classify(p, (int) k, cap, use_wave, batch_bytes, &Cl));
    const int64_t p0 = Cl.p0, n_wave = Cl.p1 - Cl.p0, n_small = Cl.p2 - Cl.p1, n_large = Cl.p3 - Cl.p2, n_global = V - Cl.p3;
    const std::vector<cc_batch>& batches = Cl.batches;
    const size_t ws_bytes = Cl.ws_bytes;
    // the call's scratch: cnt in the plan's numbering, the array asked for, the sums, the global class's workspace
    cc_scratch S;
    GMX_CHECK(S.alloc(KC_NCTR, count_host != nullptr, 1, V, ws_bytes, "kclique: the per-vertex scratch and the global class's matrices need %zu bytes: %s"));
    cc_word* const cnt = S.acc.p;
    cc_word* const ws = (cc_word*) S.ws.p;
    const kc_launch L = {p->up_begin.p, p->up_idx.p, p->kc_vtx.p, (int) k, mode, cnt, S.out.p};
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.KERNEL));
    if (count_host) GMX_HIP(hipMemsetAsync(cnt, 0, (size_t) V * sizeof(cc_word), 0));
    GMX_CHECK(kc_run(L, Cl, ws, phase_log, &phase, ph_ms));
    phase.begin();
    if (count_host) {
        hipLaunchKernelGGL(cc_finish_kernel, dim3(grid_for(V)), dim3(CC_THREADS), 0, 0, (const cc_word*) cnt, (const cc_word*) nullptr, (const int32_t*) p->perm.p, V,
                           S.cnt_out.p, S.out.p + KC_NONZERO, S.out.p + KC_SUM);
        GMX_HIP(hipGetLastError());
    }
    phase.end(&ph_ms[6]);
    cc_word h[KC_NCTR];
    GMX_CHECK(cc_read_back(tm, S, h, KC_NCTR, V, count_host, stats));
    GMX_CHECK(cc_check("kclique", count_host != nullptr, h[KC_SUM], (int) k, h[KC_TOTAL], h[KC_NONZERO], p->E_up, stats));
    *cliques = (int64_t) h[KC_TOTAL];
    if (phase_log)
        fprintf(stderr, "gmx kclique phases: plan %.3f ms, matrices %.3f ms, wave %.3f ms, small %.3f ms, large %.3f ms, global %.3f ms, finish %.3f ms\n",
                ph_ms[0], ph_ms[1], ph_ms[2], ph_ms[3], ph_ms[4], ph_ms[5], ph_ms[6]);
    if (getenv("GMX_KCLIQUE_LOG"))   // one line per call (tools/kclique_prof.py and the tests parse it)
        fprintf(stderr, "gmx kclique: plan V %lld E %lld up %lld order %s built %d classes_built %d; k %d cap %d counts %s; items %lld wave + %lld small + "
                        "%lld large + %lld global + %lld skipped; batches %zu cliques %llu\n",
                (long long) p->V, (long long) p->E, (long long) p->E_up, p->ordered ? "degree" : "identity", built ? 1 : 0, classes_built ? 1 : 0, (int) k, cap,
                cc_mode_word(mode), (long long) n_wave, (long long) n_small, (long long) n_large, (long long) n_global,
                (long long) p0, batches.size(), h[KC_TOTAL]);
    return GMX_OK;
}

void gmx_touch_kclique() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) kc_wave_kernel<CC_LOCAL>);
}
