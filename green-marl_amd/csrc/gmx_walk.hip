// gmx_walk.hip -- the sampling programs: parallel_random_walk_jump_sampling (gmx_random_walk_sampling) and
// random_node_sampling / random_degree_node_sampling (gmx_node_sampling), on one 48-bit stream (gmx.h: the stream).
//
// The device returns the bytes of the program run by one thread.  That is possible because the draws a token consumes
// depend only on the degree of the vertex it stands on (1 when the row is empty, else 2): an exclusive sum of
// Token[v] * dpt(v) over the live vertices in ascending order gives every vertex its offset into the round's part of the
// stream, token k of n starts at base[n] + k * dpt(n), and a jump by any offset is an affine map composed from the
// table of jumps by 2^k.  TokenNxt is integer adds and count a sum, so nothing else depends on an order.
//
// A round on the grid:   rw_scan_kernel   the live list (ascending): Selected, count, tokens and draws per row, Token = 0
//                        two scans        token offsets (the merge-path offsets) and draw offsets
//                        rw_move_kernel   a merge-path tile over (live rows, tokens): every token jumps to its offset, draws
//                                         and adds to TokenNxt[m]; the add that returns 0 puts m on the touched list
//                        ordering         the touched list sorted (short) or a dense pass over TokenNxt (long)
// and, while at most GMX_RW_TAIL tokens walk, whole rounds by one workgroup in one launch (rw_tail_kernel).  Tokens are
// conserved -- every token moves to exactly one vertex -- so which of the two runs is decided by num_tokens.
#include "gmx_frontier.h"

#include <rocprim/rocprim.hpp>

#define RW_THREADS BFS_THREADS
#define RW_TAIL 2048             // GMX_RW_TAIL default: tokens one workgroup still walks
#define RW_TAIL_THREADS 1024
#define RW_TAIL_ROUNDS 1024      // rounds per tail launch: a launch stays short whatever max_rounds is
#define RW_SORT_LDS 4096         // the tail sorts a list of at most this many entries in LDS
#define RW_BATCH_MAX (1 << 22)   // draws per batch of the initial set
#define RW_SORT_SHARE 8          // auto: the touched list is sorted while it has at most V / RW_SORT_SHARE entries

typedef unsigned long long rw_word;
#define RW_MASK ((1ULL << 48) - 1)
#define RW_A 0x5DEECE66DULL
#define RW_C 0xBULL

struct rw_map { uint64_t a, c; };   // x -> (a x + c) mod 2^48
static inline rw_map rw_then(rw_map f, rw_map g) {   // x -> g(f(x))
    rw_map r;
    r.a = (g.a * f.a) & RW_MASK;
    r.c = (g.a * f.c + g.c) & RW_MASK;
    return r;
}
static rw_map rw_steps(uint64_t n) {   // n single draws
    rw_map r = {1, 0}, p = {RW_A, RW_C};
    for (; n; n >>= 1) {
        if (n & 1) r = rw_then(r, p);
        p = rw_then(p, p);
    }
    return r;
}
__host__ __device__ __forceinline__ uint64_t rw_apply(rw_map m, uint64_t x) { return (m.a * x + m.c) & RW_MASK; }
__device__ __forceinline__ uint64_t rw_jump(const rw_map* __restrict__ tab, uint64_t x, uint64_t n) {   // tab[k]: 2^k draws
    for (int k = 0; n; n >>= 1, k++)
        if (n & 1) x = rw_apply(tab[k], x);
    return x;
}
__device__ __forceinline__ double rw_next(uint64_t& x) {
    x = (RW_A * x + RW_C) & RW_MASK;
    return (double) x * (1.0 / 281474976710656.0);
}

struct rw_ctl {
    rw_word x;        // tail: the stream state
    rw_word count;    // vertices selected so far
    rw_word draws;    // grid: draws of the current round
    rw_word nnext;    // grid: entries of the touched list
    rw_word nlive;    // tail: entries of the live list it leaves
    rw_word rounds;   // tail: rounds run by the last launch
    rw_word cut;      // initial set: draws the batch consumed when it completed the set (0: it did not)
    rw_word newc;     // initial set: vertices the batch added
    rw_word tdraws;   // tail: draws of the last launch
};

struct rw_state {
    const int32_t* begin;
    const int32_t* node_idx;
    const rw_map* tab;
    uint8_t* selected;
    rw_ctl* ctl;
    int64_t V;
    double p_jump;
};

// ------------------------------------------------------------------ the initial set
// draw j of the batch (state x before it) picks pick[j]; first[p] = the smallest j that picked p, among the vertices no
// earlier batch took
__global__ void __launch_bounds__(RW_THREADS) rw_init_draw_kernel(rw_state S, uint64_t x, int64_t B, const int32_t* __restrict__ token,
                                                                  int32_t* __restrict__ pick, uint32_t* __restrict__ first) {
    const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    uint64_t y = rw_jump(S.tab, x, (uint64_t) j);
    const int32_t p = (int32_t) (rw_next(y) * (double) S.V);
    pick[j] = p;
    if (token[p] == 0) atomicMin(&first[p], (uint32_t) j);
}
__global__ void __launch_bounds__(RW_THREADS) rw_init_flag_kernel(int64_t B, const int32_t* __restrict__ token, const int32_t* __restrict__ pick,
                                                                  const uint32_t* __restrict__ first, int32_t* __restrict__ flag) {
    const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    const int32_t p = pick[j];
    flag[j] = token[p] == 0 && first[p] == (uint32_t) j ? 1 : 0;
}
// incl: the inclusive sums of flag.  The first `need` new vertices get their token and their place in the list
__global__ void __launch_bounds__(RW_THREADS) rw_init_take_kernel(rw_state S, int64_t B, int32_t need, int64_t have, const int32_t* __restrict__ pick,
                                                                  const int32_t* __restrict__ flag, const int32_t* __restrict__ incl,
                                                                  int32_t* __restrict__ token, int32_t* __restrict__ list) {
    const int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= B) return;
    const int32_t c = incl[j];
    if (flag[j] && c <= need) {
        const int32_t p = pick[j];
        token[p] = 1;
        list[have + c - 1] = p;
        if (c == need) S.ctl->cut = (rw_word) (j + 1);
    }
    if (j == B - 1) S.ctl->newc = (rw_word) (c < need ? c : need);
}

// ------------------------------------------------------------------ a round on the grid
// one token of a row of deg slots that starts at slot b, stream state y at its offset: the vertex it moves to
__device__ __forceinline__ int32_t rw_token_move(const rw_state& S, int32_t b, int32_t deg, uint64_t y) {
    if (deg == 0) return (int32_t) (rw_next(y) * (double) S.V);
    const bool jump = rw_next(y) < S.p_jump;
    const double u = rw_next(y);
    if (jump) return (int32_t) (u * (double) S.V);
    return S.node_idx[(int64_t) b + (int32_t) (u * (double) deg)];
}

__global__ void __launch_bounds__(RW_THREADS) rw_scan_kernel(rw_state S, const int32_t* __restrict__ live, int64_t n, int32_t* __restrict__ token,
                                                             int32_t* __restrict__ tokc, int64_t* __restrict__ drawc) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    rw_word fresh = 0, draws = 0;
    for (int64_t base = (int64_t) blockIdx.x * blockDim.x; base < n; base += stride) {   // (wave-uniform trip count)
        const int64_t i = base + threadIdx.x;
        if (i < n) {
            const int32_t v = live[i];
            const int32_t t = token[v];
            token[v] = 0;   // this array is the next round's TokenNxt
            const int64_t d = S.begin[v + 1] == S.begin[v] ? (int64_t) t : 2 * (int64_t) t;
            tokc[i] = t;
            drawc[i] = d;
            draws += (rw_word) d;
            if (!S.selected[v]) {
                S.selected[v] = 1;
                fresh++;
            }
        }
    }
    fresh = wave_sum(fresh);
    draws = wave_sum(draws);
    if (lane == 0) {
        if (fresh) atomicAdd(&S.ctl->count, fresh);
        if (draws) atomicAdd(&S.ctl->draws, draws);
    }
}

// toff / doff[0 .. n]: the exclusive sums of tokc / drawc; m = toff[n] tokens; x: the stream state the round starts from
__global__ void __launch_bounds__(BFS_THREADS) rw_move_kernel(rw_state S, const int32_t* __restrict__ live, int64_t n, const int64_t* __restrict__ toff,
                                                              const int64_t* __restrict__ doff, int64_t m, uint64_t x, int32_t* __restrict__ token_nxt,
                                                              int32_t* __restrict__ touched) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_deg[BFS_ITEMS + 2];
    __shared__ uint32_t s_db[BFS_ITEMS + 2];   // draw offsets: a round draws fewer than 2^32 times (two per token, V < 2^31)
    __shared__ int64_t s_split[2][2];
    __shared__ int32_t s_win[BFS_ITEMS];
    __shared__ unsigned int s_nwin;
    __shared__ rw_word s_base, s_x, s_d0;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_nwin = 0;
    const frontier_tile t = frontier_tile_search(toff, n, m, s_split);
    const int nv = frontier_stage(t, S.begin, live, n, toff, m, s_off, s_row, [&](int i, int32_t v, bool in) {
        s_deg[i] = in ? S.begin[v + 1] - S.begin[v] : 0;
        s_db[i] = (uint32_t) doff[t.v0 + i];   // (t.v0 + i <= t.v1 <= n)
    });
    if (tid == 0) {   // the tile's first token: its draw offset, and the state there; the others jump from it by < 2 * BFS_ITEMS + 2
        const rw_word d0 = (rw_word) s_db[0] + (rw_word) (t.e0 - s_off[0]) * (s_deg[0] ? 2 : 1);
        s_d0 = d0;
        s_x = rw_jump(S.tab, x, d0);
    }
    __syncthreads();
    for (int64_t base = t.e0; base < t.e1; base += BFS_THREADS) {   // (workgroup-uniform trip count)
        const int64_t k = base + tid;
        const bool on = k < t.e1;
        int32_t to = 0;
        bool first = false;
        if (on) {
            const int lo = frontier_slot(s_off, nv, k);
            const int32_t deg = s_deg[lo];
            const rw_word d = (rw_word) s_db[lo] + (rw_word) (k - s_off[lo]) * (deg ? 2 : 1);
            to = rw_token_move(S, s_row[lo], deg, rw_jump(S.tab, s_x, d - s_d0));
            first = atomicAdd(&token_nxt[to], 1) == 0;
        }
        wave_append(first, to, s_win, &s_nwin, lane);
    }
    __syncthreads();
    frontier_flush(s_win, s_nwin, &S.ctl->nnext, touched, &s_base);
}

struct rw_has_token {
    const int32_t* token;
    __host__ __device__ bool operator()(const int32_t& v) const { return token[v] > 0; }
};

// ------------------------------------------------------------------ whole rounds by one workgroup
// a[0 .. P), P a power of two, ascending (a in LDS or in memory)
__device__ __forceinline__ void rw_bitonic(int32_t* a, int64_t P) {
    for (int64_t k = 2; k <= P; k <<= 1)
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < P; i += RW_TAIL_THREADS) {
                const int64_t l = i ^ j;
                if (l > i) {
                    const int32_t p = a[i], q = a[l];
                    if ((p > q) == ((i & k) == 0)) {
                        a[i] = q;
                        a[l] = p;
                    }
                }
            }
            __syncthreads();
        }
}

// la[0 .. n): the live vertices in any order (la, lb: room for the power of two at or above the tokens); Token in tok_a, zeros
// in tok_b; pk[0 .. tokens]: scratch.  Runs rounds while count < N, at most max_r of them, and leaves x, count, nlive and
// rounds in the control block; after an odd number of rounds the roles of (la, lb) and (tok_a, tok_b) are swapped.
// Token and Selected are read and written past the L1 only (atomics, agent-scope loads and stores): Token's adds are served
// by the L2, and a plain load could find an old line in the L1.
__global__ void __launch_bounds__(RW_TAIL_THREADS) rw_tail_kernel(rw_state S, int32_t* la, int32_t* lb, int64_t n, int32_t* tok_a, int32_t* tok_b,
                                                                  rw_word* pk, int64_t N, int32_t max_r) {
    __shared__ int32_t s_sort[RW_SORT_LDS];
    __shared__ rw_word s_wave[RW_TAIL_THREADS / 64];
    __shared__ rw_word s_carry, s_x;
    __shared__ unsigned int s_nnext, s_fresh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        s_x = S.ctl->x;
        s_nnext = 0;
        s_fresh = 0;
    }
    int64_t count = (int64_t) S.ctl->count;
    int32_t rounds = 0;
    rw_word tdraws = 0;
    __syncthreads();
    while (count < N && rounds < max_r) {
        // the live list ascending
        int64_t P = 1;
        while (P < n) P <<= 1;
        int32_t* a = P <= RW_SORT_LDS ? s_sort : la;
        for (int64_t i = tid; i < P; i += RW_TAIL_THREADS)
            if (a != la || i >= n) a[i] = i < n ? la[i] : INT32_MAX;
        __syncthreads();
        rw_bitonic(a, P);
        // Selected, count, and the exclusive sums of (draws << 32 | tokens) in list order
        if (tid == 0) s_carry = 0;
        __syncthreads();
        for (int64_t base = 0; base < n; base += RW_TAIL_THREADS) {   // (workgroup-uniform trip count)
            const int64_t i = base + tid;
            rw_word w = 0;
            if (i < n) {
                const int32_t v = a[i];
                la[i] = v;
                const rw_word t = (rw_word) atomicExch(&tok_a[v], 0);
                w = ((S.begin[v + 1] == S.begin[v] ? t : 2 * t) << 32) | t;
                if (!__hip_atomic_load(&S.selected[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    __hip_atomic_store(&S.selected[v], (uint8_t) 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    atomicAdd(&s_fresh, 1u);
                }
            }
            rw_word incl = w;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const rw_word y = __shfl_up(incl, o, 64);
                if (lane >= o) incl += y;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            rw_word before = s_carry;
            for (int k = 0; k < wave; k++) before += s_wave[k];
            if (i < n) pk[i] = before + incl - w;
            __syncthreads();
            if (tid == RW_TAIL_THREADS - 1) s_carry = before + incl;
            __syncthreads();
        }
        const rw_word total = s_carry;
        const int64_t m = (int64_t) (total & 0xffffffffULL);
        const uint64_t x = s_x;
        count += (int64_t) s_fresh;
        __syncthreads();
        // the tokens
        for (int64_t base = 0; base < m; base += RW_TAIL_THREADS) {   // (workgroup-uniform trip count)
            const int64_t k = base + tid;
            const bool on = k < m;
            int32_t to = 0;
            bool first = false;
            if (on) {
                int64_t lo = 0, hi = n - 1;
                while (lo < hi) {
                    const int64_t mid = (lo + hi + 1) >> 1;
                    if ((int64_t) (pk[mid] & 0xffffffffULL) <= k) lo = mid; else hi = mid - 1;
                }
                const rw_word w = pk[lo];
                const int32_t v = la[lo];
                const int32_t b = S.begin[v], deg = S.begin[v + 1] - b;
                const rw_word d = (w >> 32) + (rw_word) (k - (int64_t) (w & 0xffffffffULL)) * (deg ? 2 : 1);
                to = rw_token_move(S, b, deg, rw_jump(S.tab, x, d));
                first = atomicAdd(&tok_b[to], 1) == 0;
            }
            wave_append(first, to, lb, &s_nnext, lane);
        }
        __syncthreads();
        n = (int64_t) s_nnext;
        rounds++;
        tdraws += total >> 32;
        __syncthreads();
        if (tid == 0) {
            s_x = rw_jump(S.tab, x, total >> 32);
            s_nnext = 0;
            s_fresh = 0;
        }
        int32_t* l = la; la = lb; lb = l;
        int32_t* tk = tok_a; tok_a = tok_b; tok_b = tk;
        __syncthreads();
    }
    if (tid == 0) {
        S.ctl->x = s_x;
        S.ctl->count = (rw_word) count;
        S.ctl->nlive = (rw_word) n;
        S.ctl->rounds = (rw_word) rounds;
        S.ctl->tdraws = tdraws;
    }
}

// ------------------------------------------------------------------ node sampling
// vertex v takes draw v + 1 from x: a thread jumps to its first vertex and then steps by the grid's stride with one map
__global__ void __launch_bounds__(RW_THREADS) rw_node_kernel(rw_state S, uint64_t x, rw_map by_stride, int by_degree, double dn, double deg_sum,
                                                             rw_word* __restrict__ count) {
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t y = rw_jump(S.tab, x, (uint64_t) v + 1);
    rw_word sel = 0;
    for (; v < S.V; v += stride) {
        const double dice = (double) y * (1.0 / 281474976710656.0);
        const double prob = by_degree ? ((double) (S.begin[v + 1] - S.begin[v]) / deg_sum) * dn : 1.0 / dn;
        const bool in = dice < prob;
        S.selected[v] = in ? 1 : 0;
        sel += in ? 1 : 0;
        y = rw_apply(by_stride, y);
    }
    sel = wave_sum(sel);   // (every lane arrives: the loop above has no barrier)
    if ((threadIdx.x & 63) == 0 && sel) atomicAdd(count, sel);
}

// ------------------------------------------------------------------ host
static int rw_table_upload(dbuf<rw_map>* tab) {
    rw_map h[48];
    h[0] = rw_steps(1);
    for (int k = 1; k < 48; k++) h[k] = rw_then(h[k - 1], h[k - 1]);
    GMX_CHECK(tab->alloc(48));
    GMX_HIP(hipMemcpy(tab->p, h, sizeof(h), hipMemcpyHostToDevice));
    return GMX_OK;
}

extern "C" int gmx_random_walk_sampling(gmx_graph_t* g, float p_size, float p_jump, int32_t num_tokens, int32_t max_rounds, uint64_t* rng_state,
                                        uint8_t* selected_host, int32_t* token_host, int64_t* count, int32_t* rounds, gmx_stats_t* stats) {
    static_assert(RW_THREADS == BFS_THREADS, "the frontier tile is staged by BFS_THREADS threads");
    GMX_REQUIRE(g && rng_state && selected_host && count && rounds, "random_walk_sampling: NULL argument");
    const int64_t V = g->V;
    GMX_REQUIRE(V > 0, "random_walk_sampling: the graph has no vertices");
    GMX_REQUIRE(num_tokens >= 1 && num_tokens <= V, "random_walk_sampling: num_tokens=%d outside [1, V=%lld]", num_tokens, (long long) V);
    GMX_REQUIRE(p_size == p_size && p_jump == p_jump, "random_walk_sampling: p_size or p_jump is not a number");
    GMX_REQUIRE(max_rounds >= 0, "random_walk_sampling: max_rounds=%d is negative", max_rounds);
    const float want = (float) V * p_size;   // the float multiply of the emitted C++
    GMX_REQUIRE(want <= (float) V + 1.0f, "random_walk_sampling: p_size=%g asks for more than the V=%lld vertices", (double) p_size, (long long) V);
    const int64_t N = want < 0 ? 0 : (int64_t) want;
    GMX_REQUIRE(N <= V, "random_walk_sampling: p_size=%g asks for more than the V=%lld vertices", (double) p_size, (long long) V);
    if (stats) memset(stats, 0, sizeof(*stats));
    // read at every call; the results do not depend on them
    const int64_t tail_from = gmx_env_int("GMX_RW_TAIL", RW_TAIL, 0, INT32_MAX);
    const int64_t log = gmx_env_int("GMX_RW_LOG", 0, 0, INT32_MAX);
    const char* oe = getenv("GMX_RW_ORDER");
    const int order = oe && !strcmp(oe, "sort") ? 1 : (oe && !strcmp(oe, "dense") ? 2 : 0);
    const int64_t T = num_tokens;

    int64_t cap = 1;
    while (cap < T) cap <<= 1;
    int64_t bmax = 2 * V + 4096;
    if (bmax > RW_BATCH_MAX) bmax = RW_BATCH_MAX;
    dbuf<rw_map> tab;
    dbuf<int32_t> tok0, tok1, l0, l1, pick, flag, incl, tokc;
    dbuf<int64_t> drawc, toff, doff;
    dbuf<rw_word> pk, nsel;
    dbuf<uint8_t> selected;
    dbuf<rw_ctl> ctl;
    dbuf<char> tmp;
    gmx_pinned<rw_ctl> h_ctl;
    GMX_CHECK(rw_table_upload(&tab));
    GMX_CHECK(tok0.alloc((size_t) V));
    GMX_CHECK(tok1.alloc((size_t) V));
    GMX_CHECK(selected.alloc((size_t) V));
    GMX_CHECK(l0.alloc((size_t) cap));
    GMX_CHECK(l1.alloc((size_t) cap));
    GMX_CHECK(pick.alloc((size_t) bmax));
    GMX_CHECK(flag.alloc((size_t) bmax));
    GMX_CHECK(incl.alloc((size_t) bmax));
    GMX_CHECK(tokc.alloc((size_t) T));
    GMX_CHECK(drawc.alloc((size_t) T));
    GMX_CHECK(toff.alloc((size_t) T + 1));
    GMX_CHECK(doff.alloc((size_t) T + 1));
    GMX_CHECK(pk.alloc((size_t) T + 1));
    GMX_CHECK(nsel.alloc(1));
    GMX_CHECK(ctl.alloc(1));
    GMX_CHECK(h_ctl.alloc(1));
    const unsigned sort_bits = (unsigned) gmx_bits_for(V);
    size_t tmp_bytes = 0, b = 0;
    GMX_HIP(rocprim::inclusive_scan(nullptr, b, incl.p, incl.p, (size_t) bmax, rocprim::plus<int32_t>(), 0));
    tmp_bytes = b > tmp_bytes ? b : tmp_bytes;
    GMX_HIP(rocprim::inclusive_scan(nullptr, b, drawc.p, doff.p + 1, (size_t) T, rocprim::plus<int64_t>(), 0));
    tmp_bytes = b > tmp_bytes ? b : tmp_bytes;
    for (int64_t k = T; k > 0; k >>= 1) {   // (a short list may take another sort than a long one)
        GMX_HIP(rocprim::radix_sort_keys(nullptr, b, l1.p, l0.p, (size_t) k, 0u, sort_bits, 0));
        tmp_bytes = b > tmp_bytes ? b : tmp_bytes;
    }
    GMX_HIP(rocprim::select(nullptr, b, rocprim::counting_iterator<int32_t>(0), l0.p, nsel.p, (size_t) V, rw_has_token{tok0.p}, 0));
    tmp_bytes = b > tmp_bytes ? b : tmp_bytes;
    GMX_CHECK(tmp.alloc(tmp_bytes));
    gmx_spans tm;

    rw_state S;
    S.begin = g->begin.p;
    S.node_idx = g->node_idx.p;
    S.tab = tab.p;
    S.selected = selected.p;
    S.ctl = ctl.p;
    S.V = V;
    S.p_jump = (double) p_jump;
    rw_ctl* h = h_ctl.p;
    int32_t* token = tok0.p;      // Token
    int32_t* token_nxt = tok1.p;  // TokenNxt: zeros between rounds; `first` of the initial set before that
    int32_t* la = l0.p;           // the live list, ascending
    int32_t* lb = l1.p;           // the touched list
    uint64_t x = *rng_state & RW_MASK;

    GMX_CHECK(tm.begin(tm.KERNEL));
    const double t_start = gmx_tick::now();
    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(rw_ctl), 0));
    GMX_HIP(hipMemsetAsync(token, 0, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(token_nxt, 0xff, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(selected.p, 0, (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(toff.p, 0, sizeof(int64_t), 0));
    GMX_HIP(hipMemsetAsync(doff.p, 0, sizeof(int64_t), 0));
    // ---- the initial set: batches of draws until num_tokens distinct vertices are in it
    rw_word draws_total = 0;
    int batches = 0;
    for (int64_t have = 0; have < T;) {
        const int64_t need = T - have;
        // about twice need / (the share of vertices still free): a guess, the loop runs as many batches as it takes
        int64_t B = 2 * need * V / (V - have) + 1024;
        if (B > bmax) B = bmax;
        const unsigned nb = (unsigned) ((B + RW_THREADS - 1) / RW_THREADS);
        hipLaunchKernelGGL(rw_init_draw_kernel, dim3(nb), dim3(RW_THREADS), 0, 0, S, x, B, (const int32_t*) token, pick.p, (uint32_t*) token_nxt);
        hipLaunchKernelGGL(rw_init_flag_kernel, dim3(nb), dim3(RW_THREADS), 0, 0, B, (const int32_t*) token, (const int32_t*) pick.p,
                           (const uint32_t*) token_nxt, flag.p);
        b = tmp_bytes;
        GMX_HIP(rocprim::inclusive_scan((void*) tmp.p, b, flag.p, incl.p, (size_t) B, rocprim::plus<int32_t>(), 0));
        hipLaunchKernelGGL(rw_init_take_kernel, dim3(nb), dim3(RW_THREADS), 0, 0, S, B, (int32_t) need, have, (const int32_t*) pick.p,
                           (const int32_t*) flag.p, (const int32_t*) incl.p, token, lb);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctl, ctl.p));
        batches++;
        have += (int64_t) h->newc;
        const rw_word used = h->cut ? h->cut : (rw_word) B;
        GMX_REQUIRE(h->cut ? have == T : have < T, "random_walk_sampling: the initial set lost count (internal)");
        x = rw_apply(rw_steps(used), x);
        draws_total += used;
    }
    GMX_HIP(hipMemsetAsync(token_nxt, 0, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(&ctl.p->cut, 0, 2 * sizeof(rw_word), 0));

    // lb[0 .. nn) -> la ascending
    int sort_rounds = 0, dense_rounds = 0;
    auto put_in_order = [&](int64_t nn) -> int {
        const bool by_sort = order == 1 || (order == 0 && nn * RW_SORT_SHARE <= V);
        size_t tb = tmp_bytes;
        if (by_sort) {
            GMX_HIP(rocprim::radix_sort_keys(nullptr, tb, lb, la, (size_t) nn, 0u, sort_bits, 0));   // (which sort runs depends on nn)
            GMX_REQUIRE(tb <= tmp_bytes, "random_walk_sampling: a sort of %lld keys wants %zu bytes, %zu were planned (internal)", (long long) nn, tb,
                        tmp_bytes);
            GMX_HIP(rocprim::radix_sort_keys((void*) tmp.p, tb, lb, la, (size_t) nn, 0u, sort_bits, 0));
            sort_rounds++;
        } else {
            GMX_HIP(rocprim::select((void*) tmp.p, tb, rocprim::counting_iterator<int32_t>(0), la, nsel.p, (size_t) V, rw_has_token{token}, 0));
            dense_rounds++;
        }
        return GMX_OK;
    };

    int64_t n = T, cnt = 0;
    int32_t grid_rounds = 0, tail_rounds = 0, tail_launches = 0;
    const bool in_tail = tail_from > 0 && T <= tail_from;
    if (N > 0 && max_rounds > 0 && !in_tail) GMX_CHECK(put_in_order(n));
    if (in_tail) {
        int32_t* l = la; la = lb; lb = l;   // the tail sorts its list itself
        h->x = x;
        GMX_HIP(hipMemcpyAsync(&ctl.p->x, &h->x, sizeof(rw_word), hipMemcpyHostToDevice, 0));
        GMX_HIP(hipStreamSynchronize(0));
    }
    while (cnt < N && grid_rounds + tail_rounds < max_rounds) {
        const double t_round0 = gmx_tick::now();
        if (in_tail) {
            const int32_t left = max_rounds - tail_rounds;
            hipLaunchKernelGGL(rw_tail_kernel, dim3(1), dim3(RW_TAIL_THREADS), 0, 0, S, la, lb, n, token, token_nxt, pk.p, N,
                               left < RW_TAIL_ROUNDS ? left : RW_TAIL_ROUNDS);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, ctl.p));
            tail_launches++;
            const int32_t r = (int32_t) h->rounds;
            if (r & 1) {
                int32_t* l = la; la = lb; lb = l;
                int32_t* tk = token; token = token_nxt; token_nxt = tk;
            }
            tail_rounds += r;
            draws_total += h->tdraws;
            n = (int64_t) h->nlive;
            cnt = (int64_t) h->count;
            if (log >= 2)
                fprintf(stderr, "gmx random_walk_sampling tail launch %d: rounds %d live %lld count %lld ms %.3f\n", tail_launches, r, (long long) n,
                        (long long) cnt, (gmx_tick::now() - t_round0) * 1e3);
            GMX_REQUIRE(r > 0, "random_walk_sampling: a tail launch ran no round (internal)");
            continue;
        }
        GMX_HIP(hipMemsetAsync(&ctl.p->draws, 0, 2 * sizeof(rw_word), 0));   // draws, nnext
        hipLaunchKernelGGL(rw_scan_kernel, dim3(grid_for(n, RW_THREADS)), dim3(RW_THREADS), 0, 0, S, (const int32_t*) la, n, token, tokc.p, drawc.p);
        b = tmp_bytes;
        GMX_HIP(rocprim::inclusive_scan((void*) tmp.p, b, tokc.p, toff.p + 1, (size_t) n, rocprim::plus<int64_t>(), 0));
        b = tmp_bytes;
        GMX_HIP(rocprim::inclusive_scan((void*) tmp.p, b, drawc.p, doff.p + 1, (size_t) n, rocprim::plus<int64_t>(), 0));
        hipLaunchKernelGGL(rw_move_kernel, dim3((unsigned) frontier_tiles(n, T)), dim3(BFS_THREADS), 0, 0, S, (const int32_t*) la, n,
                           (const int64_t*) toff.p, (const int64_t*) doff.p, T, x, token_nxt, lb);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctl, ctl.p));
        { int32_t* tk = token; token = token_nxt; token_nxt = tk; }
        const int64_t live = n;
        n = (int64_t) h->nnext;
        cnt = (int64_t) h->count;
        x = rw_apply(rw_steps(h->draws), x);
        draws_total += h->draws;
        grid_rounds++;
        const int was_sort = sort_rounds, was_dense = dense_rounds;
        if (cnt < N && grid_rounds < max_rounds) GMX_CHECK(put_in_order(n));   // (the last round's list is never read)
        if (log >= 2) {
            GMX_HIP(hipStreamSynchronize(0));
            fprintf(stderr, "gmx random_walk_sampling round %d: live %lld tokens %lld draws %llu next %lld %s count %lld ms %.3f\n", grid_rounds,
                    (long long) live, (long long) T, h->draws, (long long) n, sort_rounds > was_sort ? "sort" : (dense_rounds > was_dense ? "dense" : "none"), (long long) cnt,
                    (gmx_tick::now() - t_round0) * 1e3);
        }
    }
    if (in_tail && tail_launches) x = h->x;
    GMX_CHECK(tm.end(tm.KERNEL));
    const double t_end = gmx_tick::now();
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpyAsync(selected_host, selected.p, (size_t) V, hipMemcpyDeviceToHost, 0));
    if (token_host) GMX_HIP(hipMemcpyAsync(token_host, token, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));   // (the downloads have landed)
    *count = cnt;
    *rounds = grid_rounds + tail_rounds;
    *rng_state = x;
    if (stats) {
        stats->iterations = grid_rounds + tail_rounds;
        stats->edges_examined = (int64_t) (grid_rounds + tail_rounds) * T;
        stats->vertices_reached = cnt;
    }
    if (log >= 1)   // one line per call (tools/rw_prof.py and the tests parse it)
        fprintf(stderr, "gmx random_walk_sampling: V %lld tokens %lld; tail %lld; batches %d; rounds %d grid + %d tail; tail launches %d; "
                        "sort rounds %d dense rounds %d; draws %llu; count %lld; ms %.3f\n",
                (long long) V, (long long) T, (long long) tail_from, batches, grid_rounds, tail_rounds, tail_launches, sort_rounds, dense_rounds,
                draws_total, (long long) cnt, (t_end - t_start) * 1e3);
    return GMX_OK;
}

extern "C" int gmx_node_sampling(gmx_graph_t* g, int by_degree, int32_t N, uint64_t* rng_state, uint8_t* selected_host, int64_t* count,
                                 gmx_stats_t* stats) {
    GMX_REQUIRE(g && rng_state && count, "node_sampling: NULL argument");
    GMX_REQUIRE(selected_host || g->V == 0, "node_sampling: selected is NULL");
    if (stats) memset(stats, 0, sizeof(*stats));
    *count = 0;
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    dbuf<rw_map> tab;
    dbuf<uint8_t> selected;
    dbuf<rw_word> nsel;
    gmx_pinned<rw_word> h_nsel;
    GMX_CHECK(rw_table_upload(&tab));
    GMX_CHECK(selected.alloc((size_t) V));
    GMX_CHECK(nsel.alloc(1));
    GMX_CHECK(h_nsel.alloc(1));
    gmx_spans tm;
    rw_state S;
    S.begin = g->begin.p;
    S.node_idx = g->node_idx.p;
    S.tab = tab.p;
    S.selected = selected.p;
    S.ctl = nullptr;
    S.V = V;
    S.p_jump = 0;
    const uint64_t x = *rng_state & RW_MASK;
    const int nb = grid_for(V, RW_THREADS);
    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_HIP(hipMemsetAsync(nsel.p, 0, sizeof(rw_word), 0));
    hipLaunchKernelGGL(rw_node_kernel, dim3(nb), dim3(RW_THREADS), 0, 0, S, x, rw_steps((uint64_t) nb * RW_THREADS), by_degree, (double) N,
                       (double) g->E, nsel.p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(gmx_read_back(h_nsel, nsel.p));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpyAsync(selected_host, selected.p, (size_t) V, hipMemcpyDeviceToHost, 0));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));   // (the download has landed)
    *count = (int64_t) *h_nsel.p;
    *rng_state = rw_apply(rw_steps((uint64_t) V), x);
    if (stats) {
        stats->iterations = 1;
        stats->edges_examined = V;
        stats->vertices_reached = *count;
    }
    return GMX_OK;
}

void gmx_touch_walk() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) rw_tail_kernel);
}
