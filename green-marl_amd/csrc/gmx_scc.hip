// gmx_scc.hip -- strongly connected components: kosaraju(G, mem) of apps/src/kosaraju.gm, on gfx950.
//
// The reference finds the components with a sequential DFS (InDFS, phase 1) and a BFS over G^ per DFS root in finish
// order.  The partition and the count are unique; the device computes them with the forward-backward scheme of Hong,
// Rodia and Olukotun (SC'13) and numbers the components canonically instead of in DFS finish order (see gmx.h).
//
// lab[v]: -1 live, otherwise the smallest vertex id of v's SCC (the component's ROOT).  The steps only ever remove whole
// SCCs, and each labels them with their smallest vertex:
//   trim     a live vertex with no live in-neighbour or no live out-neighbour is a singleton.  Live in/out counters per
//            vertex; removing a vertex decrements its neighbours' counters (atomics) and the ones that reach zero form
//            the next worklist.  The first counts are the row lengths (self loops included: such a vertex is never
//            trimmed, which is only conservative), and only the vertices they seed go before the first FW-BW; later
//            recounts walk the live rows and skip self loops.
//   FW-BW    the pivot (live, largest in x out, ties to the smallest id): SCC(p) = FW(p) n BW(p).  The first one (the
//            giant SCC of a small-world graph) runs the hop_dist traversal engine unrestricted, forward on g and backward
//            on a transposed view of g; later ones (and graphs whose pivot rows are not sorted: the engine's root level
//            assumes sorted rows) walk live vertices only, BW inside the FW set.
//   colour   colour[v] = v on the live vertices, the minimum propagated along live -> live edges (changed-vertex
//            queue, atomicMin) until nothing changes; then every r with colour[r] == r is the smallest vertex of its
//            SCC, which is what a backward walk from r over live vertices of colour r reaches.  The propagation is
//            abandoned after SCC_COLOUR_HOPS hops (a long chain would make it quadratic); that removes nothing, and the
//            next round's FW-BW still does.
// Rounds of trim, FW-BW, trim, colour repeat until nothing is live.  Each worklist step is one launch plus a read-back
// of the queue length; once SCC_TAIL or fewer vertices are live, ONE single-workgroup launch runs the same rounds to the
// end (no launch per hop on chains).  Every queue append is claimed first (CAS on lab[], or a round stamp in mark[]),
// so no queue ever holds a vertex twice and V entries always suffice.
#include "gmx_internal.h"

#include <limits.h>
#include <rocprim/rocprim.hpp>

#define SCC_THREADS 256
#define SCC_TAIL_THREADS 1024
#define SCC_TAIL 65536          // live vertices from which the single-workgroup launch finishes
#define SCC_SMALL 16            // rows up to this length are walked one per lane, longer ones by the whole wave
#define SCC_COLOUR_HOPS 256     // propagation hops after which a colouring round is abandoned
#define SCC_LIVE (-1)
#define SCC_MARK (-2)           // claimed by the running FW-BW; relabelled with the component's minimum right after

enum { SCC_TRIM_OUT, SCC_TRIM_IN, SCC_FW, SCC_BW, SCC_CPROP, SCC_CBW };
enum { C_Q, C_MIN, C_FLAG, C_NCTR };   // device counters: queue length, FW-BW minimum, error flag

struct scc_arrays {
    const int32_t* beg;
    const int32_t* idx;
    const int32_t* rbeg;
    const int32_t* ridx;
    int32_t* lab;
    int32_t* cin;    // live in-neighbour slots
    int32_t* cout;   // live out-neighbour slots
    int32_t* col;
    int32_t* mark;   // round stamps (FW set, colour propagation queue)
    unsigned int* ctr;
    unsigned long long* edges;   // edge slots inspected
};

// wave-converged: appends v of every lane with p to q, one atomic per wave
__device__ __forceinline__ void scc_push(bool p, int32_t v, int32_t* __restrict__ q, unsigned int* __restrict__ cnt) {
    const unsigned long long m = __ballot(p);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_ctzll(__ballot(1));
    unsigned int at = 0;
    if (lane == leader) at = atomicAdd(cnt, (unsigned int) __builtin_popcountll(m));
    at = __shfl(at, leader, 64);
    if (p) q[at + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = v;
}

__device__ __forceinline__ int32_t scc_wave_max(int32_t x) {
    for (int o = 32; o; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
    return x;
}

// edge u -> w (forward ops) or w -> u (reverse ops) of live vertex u; cu = colour of u; true: w is appended (and claimed)
template <int OP>
__device__ __forceinline__ bool scc_edge(const scc_arrays& a, int32_t u, int32_t cu, int32_t w, int32_t tag) {
    if (w == u || a.lab[w] != SCC_LIVE) return false;
    if (OP == SCC_TRIM_OUT) return atomicSub(&a.cin[w], 1) == 1 && atomicCAS(&a.lab[w], SCC_LIVE, w) == SCC_LIVE;
    if (OP == SCC_TRIM_IN) return atomicSub(&a.cout[w], 1) == 1 && atomicCAS(&a.lab[w], SCC_LIVE, w) == SCC_LIVE;
    if (OP == SCC_FW) return a.mark[w] != tag && atomicExch(&a.mark[w], tag) != tag;
    if (OP == SCC_BW) return a.mark[w] == tag && atomicCAS(&a.lab[w], SCC_LIVE, SCC_MARK) == SCC_LIVE;
    if (OP == SCC_CPROP) return cu < a.col[w] && atomicMin(&a.col[w], cu) > cu && atomicExch(&a.mark[w], tag) != tag;
    /* SCC_CBW */ return a.col[w] == cu && atomicCAS(&a.lab[w], SCC_LIVE, cu) == SCC_LIVE;
}

// The rows of q[0, n) (forward rows for TRIM_OUT / FW / CPROP, reverse rows otherwise), wave `wave` of `nwaves`:
// SCC_SMALL-or-shorter rows one per lane, longer rows by all 64 lanes, one after the other.  Every loop is
// wave-uniform, so the appends can be ballot-aggregated.
template <int OP>
__device__ void scc_walk(const scc_arrays& a, const int32_t* __restrict__ q, int64_t n, int64_t wave, int64_t nwaves, int32_t tag,
                         int32_t* __restrict__ outq) {
    constexpr bool fwd = OP == SCC_TRIM_OUT || OP == SCC_FW || OP == SCC_CPROP;
    const int32_t* __restrict__ beg = fwd ? a.beg : a.rbeg;
    const int32_t* __restrict__ idx = fwd ? a.idx : a.ridx;
    const int lane = threadIdx.x & 63;
    long long slots = 0;
    for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
        const int64_t i = base + lane;
        const bool act = i < n;
        const int32_t u = act ? q[i] : 0;
        const int32_t b = act ? beg[u] : 0, e = act ? beg[u + 1] : 0;
        const int32_t cu = (act && (OP == SCC_CPROP || OP == SCC_CBW)) ? a.col[u] : 0;
        slots += e - b;
        const bool big = e - b > SCC_SMALL;
        const int32_t len = big ? 0 : e - b;
        const int32_t mx = scc_wave_max(len);
        for (int32_t k = 0; k < mx; k++) {
            bool p = false;
            int32_t w = 0;
            if (k < len) {
                w = idx[b + k];
                p = scc_edge<OP>(a, u, cu, w, tag);
            }
            scc_push(p, w, outq, &a.ctr[C_Q]);
        }
        unsigned long long m = __ballot(big);
        while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t uu = __shfl(u, src, 64), bb = __shfl(b, src, 64), ee = __shfl(e, src, 64), cc = __shfl(cu, src, 64);
            for (int32_t j0 = bb; j0 < ee; j0 += 64) {
                const int32_t j = j0 + lane;
                bool p = false;
                int32_t w = 0;
                if (j < ee) {
                    w = idx[j];
                    p = scc_edge<OP>(a, uu, cc, w, tag);
                }
                scc_push(p, w, outq, &a.ctr[C_Q]);
            }
        }
    }
    for (int o = 32; o; o >>= 1) slots += __shfl_xor(slots, o, 64);
    if (lane == 0 && slots) atomicAdd(a.edges, (unsigned long long) slots);
}

// first counts from the row lengths; the vertices with none are trimmed (lab = v).  Nothing is queued: their
// decrements are never spread -- the recount of the live rows after the first FW-BW (or at the start of the tail)
// starts afresh.  (A queue append per wave on ONE counter from every wave of a V-sized pass is the slow part: at
// RMAT-26 the 1 M same-address atomics took 11.6 ms, against 0.5 ms for the pass itself.)
__global__ void __launch_bounds__(SCC_THREADS) scc_init_kernel(scc_arrays a, int64_t V) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const int32_t din = a.rbeg[v + 1] - a.rbeg[v], dout = a.beg[v + 1] - a.beg[v];
        a.cin[v] = din;
        a.cout[v] = dout;
        a.mark[v] = 0;
        a.lab[v] = (din == 0 || dout == 0) ? (int32_t) v : SCC_LIVE;
    }
}
// the same live test as a predicate for rocprim::select (the V-sized compactions: one atomic per workgroup tile)
struct scc_is_live {
    const int32_t* lab;
    __device__ bool operator()(int32_t v) const { return lab[v] == SCC_LIVE; }
};

// the live vertices of list[0, n) (list == NULL: 0 .. n-1) -> out
__device__ void scc_compact(const scc_arrays& a, const int32_t* __restrict__ list, int64_t n, int64_t wave, int64_t nwaves, int32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
        const int64_t i = base + lane;
        int32_t v = 0;
        bool keep = false;
        if (i < n) {
            v = list ? list[i] : (int32_t) i;
            keep = a.lab[v] == SCC_LIVE;
        }
        scc_push(keep, v, out, &a.ctr[C_Q]);
    }
}

// live neighbour slots (self loops excluded) of one row; wave-uniform like scc_walk
__device__ __forceinline__ int32_t scc_count_row(const scc_arrays& a, const int32_t* __restrict__ beg, const int32_t* __restrict__ idx,
                                                 bool act, int32_t v, long long* slots) {
    const int lane = threadIdx.x & 63;
    const int32_t b = act ? beg[v] : 0, e = act ? beg[v + 1] : 0;
    *slots += e - b;
    const bool big = e - b > SCC_SMALL;
    int32_t c = 0;
    if (!big)
        for (int32_t j = b; j < e; j++) {
            const int32_t w = idx[j];
            c += (w != v && a.lab[w] == SCC_LIVE) ? 1 : 0;
        }
    unsigned long long m = __ballot(big);
    while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        const int32_t vv = __shfl(v, src, 64), bb = __shfl(b, src, 64), ee = __shfl(e, src, 64);
        int32_t part = 0;
        for (int32_t j = bb + lane; j < ee; j += 64) {
            const int32_t w = idx[j];
            part += (w != vv && a.lab[w] == SCC_LIVE) ? 1 : 0;
        }
        for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o, 64);
        if (lane == src) c = part;
    }
    return c;
}

// fresh live counters of the live vertices (a separate pass from the trim seeds: the counts read lab[])
__device__ void scc_recount(const scc_arrays& a, const int32_t* __restrict__ list, int64_t n, int64_t wave, int64_t nwaves) {
    const int lane = threadIdx.x & 63;
    long long slots = 0;
    for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
        const int64_t i = base + lane;
        const bool act = i < n;
        const int32_t v = act ? list[i] : 0;
        const int32_t ci = scc_count_row(a, a.rbeg, a.ridx, act, v, &slots);
        const int32_t co = scc_count_row(a, a.beg, a.idx, act, v, &slots);
        if (act) {
            a.cin[v] = ci;
            a.cout[v] = co;
        }
    }
    for (int o = 32; o; o >>= 1) slots += __shfl_xor(slots, o, 64);
    if (lane == 0 && slots) atomicAdd(a.edges, (unsigned long long) slots);
}

// live vertices without live in- or out-neighbours: trimmed and queued
__device__ void scc_seed(const scc_arrays& a, const int32_t* __restrict__ list, int64_t n, int64_t wave, int64_t nwaves, int32_t* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
        const int64_t i = base + lane;
        int32_t v = 0;
        bool trim = false;
        if (i < n) {
            v = list[i];
            trim = a.lab[v] == SCC_LIVE && (a.cin[v] == 0 || a.cout[v] == 0);
            if (trim) a.lab[v] = v;
        }
        scc_push(trim, v, q, &a.ctr[C_Q]);
    }
}

// pivot key: largest in x out (saturated to 32 bits), ties to the smallest id
__device__ __forceinline__ unsigned long long scc_pivot_key(const scc_arrays& a, int32_t v) {
    unsigned long long p = (unsigned long long) (uint32_t) a.cin[v] * (unsigned long long) (uint32_t) a.cout[v];
    if (p > 0xFFFFFFFFull) p = 0xFFFFFFFFull;
    return (p << 32) | (unsigned long long) (0xFFFFFFFFu - (uint32_t) v);
}
__device__ __forceinline__ unsigned long long scc_wave_max_u64(unsigned long long x) {
    for (int o = 32; o; o >>= 1) {
        const unsigned long long y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

// ---------------------------------------------------------------- multi-workgroup launches (one per worklist step)
#define SCC_WAVE_IDS                                                                   \
    const int64_t wave = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;      \
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6

template <int OP>
__global__ void __launch_bounds__(SCC_THREADS) scc_walk_kernel(scc_arrays a, const int32_t* __restrict__ q, int64_t n, int32_t tag, int32_t* __restrict__ outq) {
    SCC_WAVE_IDS;
    scc_walk<OP>(a, q, n, wave, nwaves, tag, outq);
}
// removal of the trimmed vertices q[0, n): both directions in one launch (the first half of the waves takes the out-rows)
__global__ void __launch_bounds__(SCC_THREADS) scc_trim_kernel(scc_arrays a, const int32_t* __restrict__ q, int64_t n, int32_t* __restrict__ outq) {
    SCC_WAVE_IDS;
    const int64_t half = nwaves / 2;
    if (wave < half) scc_walk<SCC_TRIM_OUT>(a, q, n, wave, half, 0, outq);
    else scc_walk<SCC_TRIM_IN>(a, q, n, wave - half, nwaves - half, 0, outq);
}
__global__ void __launch_bounds__(SCC_THREADS) scc_recount_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n) {
    SCC_WAVE_IDS;
    scc_recount(a, list, n, wave, nwaves);
}
__global__ void __launch_bounds__(SCC_THREADS) scc_seed_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n, int32_t* __restrict__ q) {
    SCC_WAVE_IDS;
    scc_seed(a, list, n, wave, nwaves, q);
}
__global__ void __launch_bounds__(SCC_THREADS) scc_pivot_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n, unsigned long long* __restrict__ best) {
    SCC_WAVE_IDS;
    unsigned long long k = 0;
    for (int64_t i = wave * 64 + (threadIdx.x & 63); i < n; i += nwaves * 64) {
        const unsigned long long x = scc_pivot_key(a, list[i]);
        k = x > k ? x : k;
    }
    k = scc_wave_max_u64(k);
    if ((threadIdx.x & 63) == 0 && k) atomicMax(best, k);
}
// start of a walk from one vertex: q[0] = v, and its mark (FW) or its label (BW)
__global__ void scc_start_kernel(scc_arrays a, int32_t v, int32_t tag, int32_t lab, int32_t* __restrict__ q) {
    q[0] = v;
    if (tag) a.mark[v] = tag;
    else a.lab[v] = lab;
    a.ctr[C_MIN] = 0x7FFFFFFFu;
}
// the FW-BW component from the two unrestricted traversals: reached both ways -> SCC_MARK, and its minimum
__global__ void __launch_bounds__(SCC_THREADS) scc_both_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n,
                                                               const int32_t* __restrict__ dfw, const int32_t* __restrict__ dbw) {
    SCC_WAVE_IDS;
    int32_t mn = INT_MAX;
    for (int64_t i = wave * 64 + (threadIdx.x & 63); i < n; i += nwaves * 64) {
        const int32_t v = list[i];
        if (dfw[v] != INT_MAX && dbw[v] != INT_MAX) {
            a.lab[v] = SCC_MARK;
            mn = min(mn, v);
        }
    }
    for (int o = 32; o; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if ((threadIdx.x & 63) == 0 && mn != INT_MAX) atomicMin(&a.ctr[C_MIN], (unsigned int) mn);
}
__global__ void __launch_bounds__(SCC_THREADS) scc_min_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n) {
    SCC_WAVE_IDS;
    int32_t mn = INT_MAX;
    for (int64_t i = wave * 64 + (threadIdx.x & 63); i < n; i += nwaves * 64) {
        const int32_t v = list[i];
        if (a.lab[v] == SCC_MARK) mn = min(mn, v);
    }
    for (int o = 32; o; o >>= 1) mn = min(mn, __shfl_xor(mn, o, 64));
    if ((threadIdx.x & 63) == 0 && mn != INT_MAX) atomicMin(&a.ctr[C_MIN], (unsigned int) mn);
}
__global__ void __launch_bounds__(SCC_THREADS) scc_fix_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n) {
    SCC_WAVE_IDS;
    const int32_t mn = (int32_t) a.ctr[C_MIN];
    for (int64_t i = wave * 64 + (threadIdx.x & 63); i < n; i += nwaves * 64) {
        const int32_t v = list[i];
        if (a.lab[v] == SCC_MARK) a.lab[v] = mn;
    }
}
__global__ void __launch_bounds__(SCC_THREADS) scc_colour_init_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n) {
    SCC_WAVE_IDS;
    for (int64_t i = wave * 64 + (threadIdx.x & 63); i < n; i += nwaves * 64) a.col[list[i]] = list[i];
}
__global__ void __launch_bounds__(SCC_THREADS) scc_roots_kernel(scc_arrays a, const int32_t* __restrict__ list, int64_t n, int32_t* __restrict__ q) {
    SCC_WAVE_IDS;
    const int lane = threadIdx.x & 63;
    for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
        const int64_t i = base + lane;
        int32_t v = 0;
        bool root = false;
        if (i < n) {
            v = list[i];
            root = a.col[v] == v;
            if (root) a.lab[v] = v;
        }
        scc_push(root, v, q, &a.ctr[C_Q]);
    }
}
// does v's forward row and its reverse row ascend (the hop_dist engine's root level needs that)
__global__ void scc_rows_sorted_kernel(scc_arrays a, int32_t v) {
    const int32_t* begs[2] = {a.beg, a.rbeg};
    const int32_t* idxs[2] = {a.idx, a.ridx};
    const int64_t t = (int64_t) blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t) gridDim.x * blockDim.x;
    for (int d = 0; d < 2; d++)
        for (int64_t j = begs[d][v] + t + 1; j < begs[d][v + 1]; j += stride)
            if (idxs[d][j - 1] > idxs[d][j]) a.ctr[C_FLAG] = 1u;
}

// ---------------------------------------------------------------- the tail: one workgroup to the end
// (global memory written by other waves is read only after a fence + barrier + fence)
__device__ __forceinline__ void scc_tail_sync() {
    __threadfence();
    __syncthreads();
    __threadfence();
}
__device__ __forceinline__ int64_t scc_tail_take(const scc_arrays& a, unsigned int* s_n) {
    scc_tail_sync();
    if (threadIdx.x == 0) *s_n = atomicExch(&a.ctr[C_Q], 0u);
    scc_tail_sync();
    return (int64_t) *s_n;
}

// live[0, n) (n <= SCC_TAIL), other three buffers free; out[0] = rounds run, out[1] = the next free stamp
__global__ void __launch_bounds__(SCC_TAIL_THREADS) scc_tail_kernel(scc_arrays a, int32_t* la, int64_t n, int32_t* lb, int32_t* qa, int32_t* qb,
                                                                     int32_t tag, int32_t* __restrict__ out) {
    __shared__ unsigned int s_n;
    __shared__ unsigned long long s_key;
    __shared__ int s_min;
    const int64_t wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    int32_t rounds = 0;
    for (;;) {
        // trim
        scc_recount(a, la, n, wave, nwaves);
        scc_tail_sync();
        scc_seed(a, la, n, wave, nwaves, qa);
        for (int64_t m = scc_tail_take(a, &s_n); m > 0; m = scc_tail_take(a, &s_n)) {
            scc_walk<SCC_TRIM_OUT>(a, qa, m, wave, nwaves, 0, qb);
            scc_walk<SCC_TRIM_IN>(a, qa, m, wave, nwaves, 0, qb);
            int32_t* t = qa; qa = qb; qb = t;
        }
        scc_compact(a, la, n, wave, nwaves, lb);
        n = scc_tail_take(a, &s_n);
        { int32_t* t = la; la = lb; lb = t; }
        if (n == 0) break;
        rounds++;
        // FW-BW from the pivot
        if (threadIdx.x == 0) {
            s_key = 0;
            s_min = INT_MAX;
        }
        __syncthreads();
        unsigned long long k = 0;
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
            const unsigned long long x = scc_pivot_key(a, la[i]);
            k = x > k ? x : k;
        }
        k = scc_wave_max_u64(k);
        if ((threadIdx.x & 63) == 0) atomicMax(&s_key, k);
        __syncthreads();
        const int32_t p = (int32_t) (0xFFFFFFFFu - (uint32_t) s_key);
        ++tag;
        if (threadIdx.x == 0) {
            a.mark[p] = tag;
            qa[0] = p;
        }
        int64_t m = 1;
        while (m > 0) {
            scc_tail_sync();
            scc_walk<SCC_FW>(a, qa, m, wave, nwaves, tag, qb);
            m = scc_tail_take(a, &s_n);
            int32_t* t = qa; qa = qb; qb = t;
        }
        if (threadIdx.x == 0) {
            a.lab[p] = SCC_MARK;
            qa[0] = p;
        }
        m = 1;
        while (m > 0) {
            scc_tail_sync();
            scc_walk<SCC_BW>(a, qa, m, wave, nwaves, tag, qb);
            m = scc_tail_take(a, &s_n);
            int32_t* t = qa; qa = qb; qb = t;
        }
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x)
            if (a.lab[la[i]] == SCC_MARK) atomicMin(&s_min, la[i]);
        scc_tail_sync();
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x)
            if (a.lab[la[i]] == SCC_MARK) a.lab[la[i]] = s_min;
        scc_tail_sync();
        scc_compact(a, la, n, wave, nwaves, lb);
        n = scc_tail_take(a, &s_n);
        { int32_t* t = la; la = lb; lb = t; }
        if (n == 0) break;
        // colouring
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) a.col[la[i]] = la[i];
        scc_tail_sync();
        const int32_t* src = la;
        m = n;
        int hops = 0;
        while (m > 0 && hops < SCC_COLOUR_HOPS) {
            ++tag;
            scc_walk<SCC_CPROP>(a, src, m, wave, nwaves, tag, qb);
            m = scc_tail_take(a, &s_n);
            int32_t* t = qa; qa = qb; qb = t;
            src = qa;
            hops++;
        }
        if (m == 0) {   // converged: the roots and their backward walks
            for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
                const int64_t i = base + (threadIdx.x & 63);
                int32_t v = 0;
                bool root = false;
                if (i < n) {
                    v = la[i];
                    root = a.col[v] == v;
                    if (root) a.lab[v] = v;
                }
                scc_push(root, v, qa, &a.ctr[C_Q]);
            }
            for (m = scc_tail_take(a, &s_n); m > 0; m = scc_tail_take(a, &s_n)) {
                scc_walk<SCC_CBW>(a, qa, m, wave, nwaves, 0, qb);
                int32_t* t = qa; qa = qb; qb = t;
            }
        }
        scc_tail_sync();
    }
    if (threadIdx.x == 0) {
        out[0] = rounds;
        out[1] = tag;
    }
}

// ---------------------------------------------------------------- relabel and statistics
__global__ void scc_root_flag_kernel(const int32_t* __restrict__ lab, int64_t V, int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) flag[v] = lab[v] == v ? 1 : 0;
}
__global__ void scc_comp_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ id, int64_t V, int32_t* __restrict__ comp,
                                unsigned int* __restrict__ ctr) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const int32_t r = lab[v];
        const bool ok = r >= 0 && r < V;
        if (!ok) ctr[C_FLAG] = 1u;   // (cannot happen: every vertex is labelled when the rounds end)
        comp[v] = ok ? id[r] : -1;
    }
}
// sizes of the components of the vertices in list[0, n) -- whole components, by root (lanes with the same root added
// together) -- and the largest of them.  Three launches: zero the roots' counters, count, take the maximum.
__global__ void scc_size_zero_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ list, int64_t n, int64_t V,
                                     int32_t* __restrict__ size) {
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const int32_t r = lab[list[i]];
        if (r >= 0 && r < V) size[r] = 0;
    }
}
__global__ void scc_size_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ list, int64_t n, int64_t V,
                                int32_t* __restrict__ size) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) & ~63ll; base < n; base += (int64_t) gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        int32_t r = i < n ? lab[list[i]] : -1;
        bool todo = r >= 0 && r < V;
        for (unsigned long long m = __ballot(todo); m; m = __ballot(todo)) {
            const int32_t rr = __shfl(r, __builtin_ctzll(m), 64);
            const unsigned long long same = __ballot(todo && r == rr);
            if (lane == __builtin_ctzll(m)) atomicAdd(&size[rr], (int32_t) __builtin_popcountll(same));
            if (r == rr) todo = false;
        }
    }
}
__global__ void scc_max_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ list, int64_t n, int64_t V,
                               const int32_t* __restrict__ size, unsigned int* __restrict__ ctr) {
    int32_t mx = 0;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x) {
        const int32_t r = lab[list[i]];
        if (r >= 0 && r < V) mx = max(mx, size[r]);
    }
    mx = scc_wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctr[C_MIN], (unsigned int) mx);
}

// development / test option: GMX_SCC_TAIL=<n> lowers the number of live vertices from which the single-workgroup launch
// takes over (0: never), so that small graphs run the multi-workgroup rounds as well
static int64_t scc_tail_limit() {
    const char* e = getenv("GMX_SCC_TAIL");
    if (!e) return SCC_TAIL;
    const long long v = atoll(e);
    return v < 0 ? 0 : (v > SCC_TAIL ? SCC_TAIL : (int64_t) v);
}

static int scc_grid(int64_t n, int max_blocks = 256 * 8) {
    int64_t b = (n + SCC_THREADS - 1) / SCC_THREADS;
    return (int) (b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

// g's arrays with the roles of the two CSRs swapped (hop_dist on it walks in-edges); its own traversal object and hints,
// kept with g and freed with it (gmx_graph_free), the arrays are g's
static gmx_graph* scc_transposed(gmx_graph* g) {
    if (!g->scc_transpose) {
        gmx_graph* t = new gmx_graph();
        t->V = g->V;
        t->E = g->E;
        t->has_reverse = true;
        t->rows_sorted = g->r_rows_sorted;
        t->r_rows_sorted = g->rows_sorted;
        t->device = g->device;
        t->begin.p = g->r_begin.p;
        t->begin.n = g->r_begin.n;
        t->node_idx.p = g->r_node_idx.p;
        t->node_idx.n = g->r_node_idx.n;
        t->r_begin.p = g->begin.p;
        t->r_begin.n = g->begin.n;
        t->r_node_idx.p = g->node_idx.p;
        t->r_node_idx.n = g->node_idx.n;
        g->scc_transpose = t;
    }
    return g->scc_transpose;
}

namespace {
struct scc_run {
    scc_arrays a{};
    int64_t V = 0;
    gmx_pinned<unsigned int> h_ctr;
    int32_t tag = 0;
    int64_t phase_removed[4] = {0, 0, 0, 0};   // trim, FW-BW, colour, tail
    double phase_ms[5] = {0, 0, 0, 0, 0};      // the same + relabel
    int read(unsigned int* dst, int which) {   // synchronises
        GMX_HIP(hipMemcpyAsync(h_ctr.p, &a.ctr[which], sizeof(unsigned int), hipMemcpyDeviceToHost, 0));
        GMX_HIP(hipStreamSynchronize(0));
        *dst = *h_ctr.p;
        return GMX_OK;
    }
    int clear_q() {
        GMX_HIP(hipMemsetAsync(&a.ctr[C_Q], 0, sizeof(unsigned int), 0));
        return GMX_OK;
    }
    // launch, then the length of the queue it wrote
    template <class F>
    int step(F launch, int64_t* m) {
        GMX_CHECK(clear_q());
        launch();
        GMX_HIP(hipGetLastError());
        unsigned int c = 0;
        GMX_CHECK(read(&c, C_Q));
        *m = c;
        return GMX_OK;
    }
};
}  // namespace

extern "C" int gmx_scc(gmx_graph_t* g, int32_t* comp_host, int64_t* num_comps, gmx_stats_t* stats_out) {
    GMX_REQUIRE(g && comp_host && num_comps, "NULL argument");
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    *num_comps = 0;
    if (!g->has_reverse) {
        gmx_set_error("gmx_scc needs the reverse CSR (the graph was uploaded with GMX_GRAPH_NO_REVERSE)");
        return GMX_ERR_STATE;
    }
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    const bool phase_log = getenv("GMX_SCC_PHASES") != nullptr;   // per-phase times (events) for tools/scc_prof.py
    const int64_t tail_lim = scc_tail_limit();
    gmx_ws_scope scope;
    wbuf<int32_t> lab, cin, cout, col, mark, la, lb, qa, qb, rest;
    wbuf<unsigned int> ctr;
    wbuf<unsigned long long> edges, best;
    wbuf<int32_t> tail_out;
    GMX_CHECK(lab.alloc(V));
    GMX_CHECK(cin.alloc(V));
    GMX_CHECK(cout.alloc(V));
    GMX_CHECK(col.alloc(V));
    GMX_CHECK(rest.alloc(V));
    GMX_CHECK(mark.alloc(V));
    GMX_CHECK(la.alloc(V));
    GMX_CHECK(lb.alloc(V));
    GMX_CHECK(qa.alloc(V));
    GMX_CHECK(qb.alloc(V));
    GMX_CHECK(ctr.alloc(C_NCTR));
    GMX_CHECK(edges.alloc(1));
    GMX_CHECK(best.alloc(1));
    GMX_CHECK(tail_out.alloc(2));
    size_t sel_bytes = 0, sel_bytes2 = 0;
    GMX_HIP(rocprim::select(nullptr, sel_bytes, rocprim::counting_iterator<int32_t>(0), la.p, ctr.p, (size_t) V, scc_is_live{lab.p}, 0));
    GMX_HIP(rocprim::select(nullptr, sel_bytes2, (const int32_t*) la.p, lb.p, ctr.p, (size_t) V, scc_is_live{lab.p}, 0));
    sel_bytes = std::max(sel_bytes, sel_bytes2);
    wbuf<char> sel_tmp;
    GMX_CHECK(sel_tmp.alloc(sel_bytes));
    scc_run R;
    R.V = V;
    R.a = scc_arrays{g->begin.p, g->node_idx.p, g->r_begin.p, g->r_node_idx.p, lab.p, cin.p, cout.p, col.p, mark.p, ctr.p, edges.p};
    GMX_CHECK(R.h_ctr.alloc(4));
    const scc_arrays& A = R.a;
    gmx_spans tm;
    GMX_HIP(hipMemsetAsync(ctr.p, 0, sizeof(unsigned int) * C_NCTR, 0));
    GMX_HIP(hipMemsetAsync(edges.p, 0, sizeof(unsigned long long), 0));
    GMX_CHECK(tm.begin(tm.KERNEL));
    // GMX_SCC_PHASES: an event at every phase boundary; the phases' shares of the timed span are added up at the end
    std::vector<std::pair<gmx_event, int>> phase_ev;
    auto phase_end = [&](int ph) {
        if (!phase_log) return;
        gmx_event e;
        if (e.create() != GMX_OK) return;
        (void) hipEventRecord(e, 0);
        phase_ev.emplace_back(std::move(e), ph);
    };

    int64_t live = V;   // vertices not yet removed
    int64_t m = 0, n = 0;
    int32_t rounds = 0;
    // trim rounds from the queue in qa[0, m): removed vertices are counted as they are queued
    auto trim_rounds = [&](int64_t m0) -> int {
        int64_t mm = m0;
        int32_t *q = qa.p, *nq = qb.p;
        while (mm > 0 && live > tail_lim) {
            GMX_CHECK(R.step([&] { hipLaunchKernelGGL(scc_trim_kernel, dim3(scc_grid(2 * mm)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) q, mm, nq); }, &mm));
            live -= mm;
            R.phase_removed[0] += mm;
            std::swap(q, nq);
        }
        return GMX_OK;
    };
    // the live list of list[0, cnt) (NULL: every vertex) -> la
    auto compact = [&](const int32_t* list, int64_t cnt) -> int {
        size_t tb = sel_bytes;
        if (list) GMX_HIP(rocprim::select((void*) sel_tmp.p, tb, list, la.p, &ctr.p[C_Q], (size_t) cnt, scc_is_live{lab.p}, 0));
        else GMX_HIP(rocprim::select((void*) sel_tmp.p, tb, rocprim::counting_iterator<int32_t>(0), la.p, &ctr.p[C_Q], (size_t) cnt, scc_is_live{lab.p}, 0));
        unsigned int c = 0;
        GMX_CHECK(R.read(&c, C_Q));
        n = live = c;
        return GMX_OK;
    };
    auto relist = [&]() -> int {   // la -> lb -> la
        GMX_HIP(hipMemcpyAsync(lb.p, la.p, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToDevice, 0));
        return compact(lb.p, n);
    };
    auto recount_trim = [&]() -> int {
        hipLaunchKernelGGL(scc_recount_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n);
        GMX_CHECK(R.step([&] { hipLaunchKernelGGL(scc_seed_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n, qa.p); }, &m));
        live -= m;
        R.phase_removed[0] += m;
        GMX_CHECK(trim_rounds(m));
        return relist();
    };

    // trim-1 from the row lengths: only its seeds (no in- or no out-edges) are removed before the first FW-BW.  The
    // decrements they would spread land mostly on the giant SCC, which the FW-BW removes anyway (RMAT-26: 38.8 M seeds,
    // most of whose out-edges lead into it); the recount after it (or the tail's) starts from the live rows.
    hipLaunchKernelGGL(scc_init_kernel, dim3(scc_grid(V)), dim3(SCC_THREADS), 0, 0, A, V);
    GMX_CHECK(compact(nullptr, V));
    R.phase_removed[0] += V - n;
    R.tag = 1;
    phase_end(0);
    bool engine_used = false;
    // the largest component (vertices_reached): the first FW-BW's, or one of the live set right after it (`rest`; every
    // component found later lies inside it) -- the vertices removed before are trimmed singletons
    int64_t giant = 0, nrest = -1;
    while (n > tail_lim) {
        rounds++;
        if (rounds > 1) {
            GMX_CHECK(recount_trim());
            phase_end(0);
            if (n <= tail_lim) break;
        }
        // FW-BW from the pivot
        const int64_t before = n;
        GMX_HIP(hipMemsetAsync(best.p, 0, sizeof(unsigned long long), 0));
        hipLaunchKernelGGL(scc_pivot_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n, best.p);
        unsigned long long key = 0;
        GMX_HIP(hipMemcpy(&key, best.p, sizeof(key), hipMemcpyDeviceToHost));
        const int32_t p = (int32_t) (0xFFFFFFFFu - (uint32_t) key);
        GMX_REQUIRE(p >= 0 && p < V, "scc: no pivot among %lld live vertices", (long long) n);
        unsigned int unsorted = 1;
        if (!engine_used) {
            GMX_HIP(hipMemsetAsync(&ctr.p[C_FLAG], 0, sizeof(unsigned int), 0));
            hipLaunchKernelGGL(scc_rows_sorted_kernel, dim3(256), dim3(SCC_THREADS), 0, 0, A, p);
            GMX_CHECK(R.read(&unsorted, C_FLAG));
            GMX_HIP(hipMemsetAsync(&ctr.p[C_FLAG], 0, sizeof(unsigned int), 0));   // (the flag reports lost vertices later)
        }
        if (!unsorted) {   // the giant SCC through the traversal engine, unrestricted
            engine_used = true;
            const int32_t *dfw = nullptr, *dbw = nullptr;
            int64_t e1 = 0, e2 = 0;
            GMX_CHECK(gmx_bfs_reach(g, p, &dfw, &e1));
            GMX_CHECK(gmx_bfs_reach(scc_transposed(g), p, &dbw, &e2));
            stats->edges_examined += e1 + e2;
            hipLaunchKernelGGL(scc_start_kernel, dim3(1), dim3(1), 0, 0, A, p, 0, SCC_LIVE, qa.p);   // (resets the minimum only)
            hipLaunchKernelGGL(scc_both_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n, dfw, dbw);
        } else {
            const int32_t tag = ++R.tag;
            hipLaunchKernelGGL(scc_start_kernel, dim3(1), dim3(1), 0, 0, A, p, tag, 0, qa.p);
            int32_t *q = qa.p, *nq = qb.p;
            for (m = 1; m > 0; std::swap(q, nq))
                GMX_CHECK(R.step([&] { hipLaunchKernelGGL(scc_walk_kernel<SCC_FW>, dim3(scc_grid(m)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) q, m, tag, nq); }, &m));
            hipLaunchKernelGGL(scc_start_kernel, dim3(1), dim3(1), 0, 0, A, p, 0, SCC_MARK, qa.p);
            q = qa.p;
            nq = qb.p;
            for (m = 1; m > 0; std::swap(q, nq))
                GMX_CHECK(R.step([&] { hipLaunchKernelGGL(scc_walk_kernel<SCC_BW>, dim3(scc_grid(m)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) q, m, tag, nq); }, &m));
            hipLaunchKernelGGL(scc_min_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n);
        }
        hipLaunchKernelGGL(scc_fix_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n);
        GMX_CHECK(relist());
        R.phase_removed[1] += before - n;
        if (nrest < 0) {
            giant = before - n;
            nrest = n;
            if (n) GMX_HIP(hipMemcpyAsync(rest.p, la.p, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToDevice, 0));
        }
        phase_end(1);
        if (n <= tail_lim) break;
        GMX_CHECK(recount_trim());
        phase_end(0);
        if (n <= tail_lim) break;
        // colouring
        const int64_t before_c = n;
        hipLaunchKernelGGL(scc_colour_init_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n);
        const int32_t* src = la.p;
        int32_t *q = qa.p, *nq = qb.p;
        int hops = 0;
        for (m = n; m > 0 && hops < SCC_COLOUR_HOPS; hops++) {
            const int32_t tag = ++R.tag;
            GMX_CHECK(R.step([&] { hipLaunchKernelGGL(scc_walk_kernel<SCC_CPROP>, dim3(scc_grid(m)), dim3(SCC_THREADS), 0, 0, A, src, m, tag, q); }, &m));
            src = q;
            std::swap(q, nq);
        }
        if (m == 0) {
            q = qa.p;
            nq = qb.p;
            GMX_CHECK(R.step([&] { hipLaunchKernelGGL(scc_roots_kernel, dim3(scc_grid(n)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) la.p, n, q); }, &m));
            for (; m > 0; std::swap(q, nq))
                GMX_CHECK(R.step([&] { hipLaunchKernelGGL(scc_walk_kernel<SCC_CBW>, dim3(scc_grid(m)), dim3(SCC_THREADS), 0, 0, A, (const int32_t*) q, m, 0, nq); }, &m));
            GMX_CHECK(relist());
        }
        R.phase_removed[2] += before_c - n;
        phase_end(2);
    }
    if (n > 0) {   // the rest in one workgroup
        if (nrest < 0) {
            nrest = n;
            GMX_HIP(hipMemcpyAsync(rest.p, la.p, sizeof(int32_t) * (size_t) n, hipMemcpyDeviceToDevice, 0));
        }
        GMX_CHECK(R.clear_q());
        hipLaunchKernelGGL(scc_tail_kernel, dim3(1), dim3(SCC_TAIL_THREADS), 0, 0, A, la.p, n, lb.p, qa.p, qb.p, R.tag, tail_out.p);
        GMX_HIP(hipGetLastError());
        int32_t to[2] = {0, 0};
        GMX_HIP(hipMemcpy(to, tail_out.p, sizeof(to), hipMemcpyDeviceToHost));
        rounds += to[0];
        R.phase_removed[3] += n;
        phase_end(3);
    }
    // relabel: ids by ascending root = ascending smallest vertex
    int32_t* flag = cin.p;
    int32_t* id = cout.p;
    int32_t* comp = col.p;
    hipLaunchKernelGGL(scc_root_flag_kernel, dim3(scc_grid(V)), dim3(SCC_THREADS), 0, 0, (const int32_t*) lab.p, V, flag);
    {
        size_t tb = 0;
        GMX_HIP(rocprim::exclusive_scan(nullptr, tb, flag, id, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
        wbuf<char> tmp;
        GMX_CHECK(tmp.alloc(tb));
        GMX_HIP(rocprim::exclusive_scan((void*) tmp.p, tb, flag, id, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
    }
    hipLaunchKernelGGL(scc_comp_kernel, dim3(scc_grid(V)), dim3(SCC_THREADS), 0, 0, (const int32_t*) lab.p, (const int32_t*) id, V, comp, ctr.p);
    GMX_HIP(hipGetLastError());
    phase_end(4);
    GMX_CHECK(tm.end(tm.KERNEL));
    int32_t last[2] = {0, 0};
    GMX_HIP(hipMemcpy(&last[0], id + V - 1, sizeof(int32_t), hipMemcpyDeviceToHost));
    GMX_HIP(hipMemcpy(&last[1], flag + V - 1, sizeof(int32_t), hipMemcpyDeviceToHost));
    unsigned int bad = 0;
    GMX_CHECK(R.read(&bad, C_FLAG));
    if (bad) {
        gmx_set_error("scc: a vertex was left without a component");
        return GMX_ERR_STATE;
    }
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(comp_host, comp, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));
    // statistics outside the timed part: the largest component
    unsigned int largest = 1;   // (V > 0: a trimmed vertex at least)
    if (nrest > 0) {
        GMX_HIP(hipMemsetAsync(&ctr.p[C_MIN], 0, sizeof(unsigned int), 0));
        hipLaunchKernelGGL(scc_size_zero_kernel, dim3(scc_grid(nrest)), dim3(SCC_THREADS), 0, 0, (const int32_t*) lab.p, (const int32_t*) rest.p, nrest, V, flag);
        hipLaunchKernelGGL(scc_size_kernel, dim3(scc_grid(nrest)), dim3(SCC_THREADS), 0, 0, (const int32_t*) lab.p, (const int32_t*) rest.p, nrest, V, flag);
        hipLaunchKernelGGL(scc_max_kernel, dim3(scc_grid(nrest)), dim3(SCC_THREADS), 0, 0, (const int32_t*) lab.p, (const int32_t*) rest.p, nrest, V,
                           (const int32_t*) flag, ctr.p);
        GMX_HIP(hipGetLastError());
        unsigned int mx = 0;
        GMX_CHECK(R.read(&mx, C_MIN));
        largest = std::max(largest, mx);
    }
    largest = std::max(largest, (unsigned int) giant);
    unsigned long long ed = 0;
    GMX_HIP(hipMemcpy(&ed, edges.p, sizeof(ed), hipMemcpyDeviceToHost));
    *num_comps = (int64_t) last[0] + last[1];
    stats->iterations = rounds;
    stats->vertices_reached = largest;
    stats->edges_examined += (int64_t) ed;
    if (phase_log) {
        hipEvent_t prev = tm.begin_event(tm.KERNEL);
        for (auto& e : phase_ev) {
            float t = 0;
            (void) hipEventElapsedTime(&t, prev, e.first);
            R.phase_ms[e.second] += t;
            prev = e.first;
        }
        fprintf(stderr,
                "gmx scc phases: trim %.3f ms (%lld removed), fwbw %.3f ms (%lld), colour %.3f ms (%lld), tail %.3f ms (%lld), "
                "relabel %.3f ms; rounds %d, engine %d\n",
                R.phase_ms[0], (long long) R.phase_removed[0], R.phase_ms[1], (long long) R.phase_removed[1], R.phase_ms[2],
                (long long) R.phase_removed[2], R.phase_ms[3], (long long) R.phase_removed[3], R.phase_ms[4], (int) rounds, engine_used ? 1 : 0);
    }
    return GMX_OK;
}

void gmx_touch_scc() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) scc_init_kernel);
}
