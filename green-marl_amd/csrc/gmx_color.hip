// gmx_color.hip -- greedy vertex colouring on gfx950: first fit in a fixed vertex order, computed by the Jones-Plassmann
// schedule in queue rounds.  The reference has no such program; the order, the result, the schedule that fixes depth[] and
// the statistics are the contract at gmx_coloring in gmx.h.
//
// "u is earlier than w" is one compare of two 64-bit words key[] = (priority, ~id).  One word pend[v] per vertex: the slots
// of v (out-row + in-row, other end != v) whose other end is earlier and not coloured yet.  It only falls, by atomic
// decrements of 1, so the decrement that returns 1 makes the vertex ready and queues it exactly once.
//   count     one pass over the forward slots: a slot u -> w, u != w, is a slot of both ends and counts for the later one.
//             npred[] keeps the counts as they were (they bound the colour); pend == 0 is round 0's queue.
//   colour    a ready vertex takes the smallest colour none of its neighbours holds.  Every coloured neighbour is an earlier
//             one and no neighbour is coloured in the same round, so color[] is read and written with plain accesses.
//             By row length L = outdeg + indeg: group (16 lanes a row, a 64-bit mask in registers), wave (a wave a row, a
//             bitmap of min(npred, L) + 1 bits in the wave's LDS slice), block (a workgroup a row, a bitmap of
//             GMX_COLOR_WINDOW bits, the row walked once per window of colours until one has a free colour).  A colour
//             outside the bitmap is ignored: the pigeonhole puts the answer below min(npred, L) + 1.
//   release   the rows of the round's queue go through the merge-path tile (gmx_frontier.h), forward then reverse: a slot
//             whose other end has no colour yet lowers its pend[], the decrement that returns 1 appends it to q[] and, by
//             its row length, to the wave or the block list.  A vertex is queued once in the whole run, so ONE array holds
//             every round's segment behind the other (as gmx_kcore's does) and each list likewise.
//   tail      while the queue holds at most GMX_COLOR_TAIL entries + row slots one workgroup runs colour + release rounds
//             with a barrier between them and hands back otherwise.
// The schedule does not depend on the order of the decrements: which round readies a vertex does not, and the colour is a
// function of the earlier neighbours' colours alone.  Only the order inside a segment varies.
#include "gmx_frontier.h"

#define CO_THREADS BFS_THREADS
#define CO_TAIL_THREADS 1024
#define CO_BLOCK_THREADS 1024     // the block regime's workgroup: a long row is a chain of gathers, 4096 slots a step
#define CO_TAIL 1024            // GMX_COLOR_TAIL: the tail launch takes over while the queue holds at most this many entries + slots
#define CO_TAIL_LANE 8          // the tail's release reads a row of at most this many slots with one lane, a longer one with a wave
#define CO_WAVE_MIN 65          // GMX_COLOR_WAVE_MIN: rows of at least this many slots leave the group regime (at most 65: the mask has 64 bits)
#define CO_WAVE_WORDS 256       // a wave's LDS slice: 8192 bits, which bounds GMX_COLOR_BLOCK_MIN
#define CO_BLOCK_MAX (CO_WAVE_WORDS * 32)
#define CO_BLOCK_MIN 256        // GMX_COLOR_BLOCK_MIN: rows of at least this many slots go to the block regime (the sweep's best at RMAT-20 to 24)
#define CO_WINDOW (1 << 18)     // GMX_COLOR_WINDOW: 32 KB of LDS, two workgroups a CU and more; also the knob's largest value
#define CO_SMALL 2048           // a queue of at most this many entries takes its offsets from color_offsets_kernel
#define CO_NONE 0xFFFFFFFFu

typedef unsigned long long co_word;

struct co_ctl {
    co_word qtail;       // tail of q[]: vertices made ready so far
    co_word wtail;       // tail of the wave list
    co_word btail;       // tail of the block list
    co_word slots[2];    // row slots (forward, reverse) of q[0, qtail)
    co_word passes;      // extra window passes of the block regime
    co_word class0;      // vertices of colour 0
    co_word left;        // vertices without a colour at the end (none)
    // what the tail hands back
    long long t_qs, t_qe, t_ws, t_we, t_bs, t_be, t_rounds, t_m[2];
    int32_t t_state, maxcolor;
};
enum { CO_DONE = 0, CO_HANDBACK = 1 };

struct co_state {
    const int32_t* beg[2];   // forward, reverse
    const int32_t* idx[2];
    int32_t* pend;
    int32_t* npred;
    int32_t* color;
    int32_t* depth;          // or NULL
    int32_t* q;
    int32_t* lw;             // the wave regime's vertices in the order they became ready
    int32_t* lb;             // the block regime's
    co_ctl* ctl;
    int64_t V;
    int32_t wave_min, block_min, window;
};

// LDS written by other lanes of this wave is read after this (a wave's LDS operations execute in order)
__device__ __forceinline__ void co_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int64_t co_row_len(const co_state& S, int32_t v) {
    return ((int64_t) S.beg[0][v + 1] - S.beg[0][v]) + ((int64_t) S.beg[1][v + 1] - S.beg[1][v]);
}
__device__ __forceinline__ int co_regime(const co_state& S, int64_t L) { return L >= S.block_min ? 2 : (L >= S.wave_min ? 1 : 0); }
// bits of the bitmap that holds v's answer: the earlier neighbours hold at most min(npred, L) different colours
__device__ __forceinline__ int64_t co_need(const co_state& S, int32_t v, int64_t L) {
    const int64_t np = S.npred[v];
    return (np < L ? np : L) + 1;
}

// what belongs to making v ready for round `round`; adds v's row slots to m[], returns v's regime
__device__ __forceinline__ int co_ready(const co_state& S, int32_t v, int32_t round, co_word* m) {
    if (S.depth) S.depth[v] = round;
    int64_t L = 0;
    for (int d = 0; d < 2; d++) {
        const int32_t len = S.beg[d][v + 1] - S.beg[d][v];
        if (len) atomicAdd(&m[d], (co_word) len);
        L += len;
    }
    return co_regime(S, L);
}
// a wave's lanes that made a vertex ready append it to queue[] and to its regime's list; every lane of the wave must be here
template <class QCount, class LCount>
__device__ __forceinline__ void co_append(const co_state& S, bool on, int32_t v, int32_t round, int32_t* queue, QCount* qcount, LCount* wcount,
                                          LCount* bcount, co_word* m, int lane) {
    int regime = 0;
    wave_append(on, v, queue, qcount, lane, [&] { regime = co_ready(S, v, round, m); });
    wave_append(regime == 1, v, S.lw, wcount, lane);
    wave_append(regime == 2, v, S.lb, bcount, lane);
}

// ---- count
// key[v]: larger = earlier.  prio == NULL: outdeg + indeg from the offsets, as an unsigned sum
__global__ void __launch_bounds__(CO_THREADS) color_key_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ r_begin,
                                                               const int32_t* __restrict__ prio, int64_t V, co_word* __restrict__ key) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const uint32_t p = prio ? (uint32_t) prio[v] ^ 0x80000000u : (uint32_t) (begin[v + 1] - begin[v]) + (uint32_t) (r_begin[v + 1] - r_begin[v]);
        key[v] = ((co_word) p << 32) | (co_word) (0xFFFFFFFFu - (uint32_t) v);
    }
}
// one pass over the forward slots, BFS_ITEMS at a time; the row of a slot is searched between the rows of the chunk's first
// and last slot (as kcore_slots_kernel does).  The later end of u -> w, u != w, waits for the earlier one.
__global__ void __launch_bounds__(CO_THREADS) color_count_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int64_t E,
                                                                 const co_word* __restrict__ key, int32_t* __restrict__ pend) {
    __shared__ int32_t s_row[2];
    for (int64_t c0 = (int64_t) blockIdx.x * BFS_ITEMS; c0 < E; c0 += (int64_t) gridDim.x * BFS_ITEMS) {
        const int64_t c1 = c0 + BFS_ITEMS < E ? c0 + BFS_ITEMS : E;
        if (threadIdx.x < 2) s_row[threadIdx.x] = csr_row_of(begin, V, (uint32_t) (threadIdx.x ? c1 - 1 : c0));
        __syncthreads();
        const int32_t r0 = s_row[0], r1 = s_row[1];
        for (int64_t e = c0 + threadIdx.x; e < c1; e += CO_THREADS) {
            const int32_t w = idx[e];
            int32_t lo = r0, hi = r1;
            while (lo < hi) {
                const int32_t mid = (int32_t) (((int64_t) lo + hi + 1) >> 1);
                if ((int64_t) begin[mid] <= e) lo = mid; else hi = mid - 1;
            }
            if (w != lo) atomicAdd(&pend[key[w] > key[lo] ? lo : w], 1);
        }
        __syncthreads();
    }
}
// npred = pend as counted; the vertices nobody is earlier than are round 0's queue.  A workgroup collects BFS_ITEMS
// entries in LDS and claims the tail once.
__global__ void __launch_bounds__(CO_THREADS) color_seed_kernel(co_state S) {
    __shared__ int32_t s_q[BFS_ITEMS];
    __shared__ unsigned int s_nq;
    __shared__ co_word s_m[2], s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t t0 = (int64_t) blockIdx.x * BFS_ITEMS; t0 < S.V; t0 += (int64_t) gridDim.x * BFS_ITEMS) {
        if (tid == 0) {
            s_nq = 0;
            s_m[0] = s_m[1] = 0;
        }
        __syncthreads();
        for (int j = 0; j < BFS_ITEMS / CO_THREADS; j++) {
            const int64_t i = t0 + j * CO_THREADS + tid;
            const int32_t v = i < S.V ? (int32_t) i : 0;
            const int32_t p = i < S.V ? S.pend[v] : 1;
            if (i < S.V) S.npred[v] = p;
            co_append(S, p == 0, v, 0, s_q, &s_nq, &S.ctl->wtail, &S.ctl->btail, s_m, lane);
        }
        __syncthreads();
        frontier_flush(s_q, s_nq, &S.ctl->qtail, S.q, &s_base, [&] {
            for (int d = 0; d < 2; d++)
                if (s_m[d]) atomicAdd(&S.ctl->slots[d], s_m[d]);
        });
        __syncthreads();
    }
}

// ---- colour
// use(c) for the colour c of the other end of every slot first, first + stride, ... of v's two rows (and for -1 where a
// step runs past the row's end); four slots' loads are in flight together: a row is a chain of gathers otherwise
template <class Use>
__device__ __forceinline__ void co_walk(const co_state& S, int32_t v, bool on, int first, int stride, Use use) {
    for (int d = 0; d < 2; d++) {
        const int32_t* __restrict__ idx = S.idx[d];
        const int64_t b = on ? S.beg[d][v] : 0, e = on ? S.beg[d][v + 1] : 0;
        for (int64_t x = b + first; x < e; x += 4 * (int64_t) stride) {
            int32_t c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t xk = x + (int64_t) k * stride;
                c[k] = xk < e ? idx[xk] : -1;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = c[k] >= 0 ? S.color[c[k]] : -1;
#pragma unroll
            for (int k = 0; k < 4; k++) use(c[k]);
        }
    }
}

// group: the four entries list[i0 .. i0 + 4) by the four 16-lane groups of a wave (i0 wave-uniform); rows of another
// regime are left to their list
__device__ __forceinline__ void co_color_group(const co_state& S, const int32_t* list, int64_t i0, int64_t n, int lane) {
    const int64_t i = i0 + (lane >> 4);
    const int sub = lane & 15;
    bool on = i < n;
    const int32_t v = on ? list[i] : 0;
    on = on && co_regime(S, co_row_len(S, v)) == 0;
    co_word mask = 0;
    co_walk(S, v, on, sub, 16, [&](int32_t c) {
        if (c >= 0 && c < 64) mask |= 1ULL << c;   // (64 and above: ignored, never shifted or wrapped)
    });
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mask |= __shfl_xor(mask, o, 16);
    if (on && sub == 0) S.color[v] = mask == ~0ULL ? 64 : (int32_t) __builtin_ctzll(~mask);
}
__global__ void __launch_bounds__(CO_THREADS) color_group_kernel(co_state S, const int32_t* __restrict__ list, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t) blockIdx.x * CO_THREADS + threadIdx.x) >> 6, nwaves = ((int64_t) gridDim.x * CO_THREADS) >> 6;
    for (int64_t i0 = wave * 4; i0 < n; i0 += nwaves * 4) co_color_group(S, list, i0, n, lane);
}

// wave: row v by one wave, bits[] its LDS slice of CO_WAVE_WORDS words (v's bitmap fits: L < block_min <= CO_BLOCK_MAX)
__device__ __forceinline__ void co_color_wave(const co_state& S, int32_t v, unsigned int* bits, int lane) {
    const int32_t need = (int32_t) co_need(S, v, co_row_len(S, v));
    const int nwords = (need + 31) >> 5;
    for (int i = lane; i < nwords; i += 64) bits[i] = 0;
    co_wave_sync();
    co_walk(S, v, true, lane, 64, [&](int32_t c) {
        if (c >= 0 && c < need) atomicOr(&bits[c >> 5], 1u << (c & 31));
    });
    co_wave_sync();
    int32_t found = -1;
    for (int base = 0; base < nwords; base += 64) {   // (wave-uniform)
        const unsigned int word = base + lane < nwords ? bits[base + lane] : CO_NONE;
        const unsigned long long mk = __ballot(word != CO_NONE);
        if (mk) {
            const int src = __builtin_ctzll(mk);
            found = (base + src) * 32 + __builtin_ctz(~__shfl(word, src, 64));
            break;
        }
    }
    if (lane == 0) S.color[v] = found;
    co_wave_sync();   // all lanes are done with the slice before the next row clears it
}
__global__ void __launch_bounds__(CO_THREADS) color_wave_kernel(co_state S, const int32_t* __restrict__ list, int64_t n) {
    __shared__ unsigned int s_bits[(CO_THREADS >> 6) * CO_WAVE_WORDS];
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t) blockIdx.x * CO_THREADS + threadIdx.x) >> 6, nwaves = ((int64_t) gridDim.x * CO_THREADS) >> 6;
    for (int64_t i = wave; i < n; i += nwaves) co_color_wave(S, list[i], s_bits + (threadIdx.x >> 6) * CO_WAVE_WORDS, lane);
}

// block: row v by the whole workgroup (every thread here with the same v), bits[] S.window bits of LDS.  Window k holds
// the colours [k W, (k + 1) W); the walk stops at the first window with a free colour: floor(color / W) extra passes.
__device__ __forceinline__ void co_color_block(const co_state& S, int32_t v, unsigned int* bits, unsigned int* s_found) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t need = co_need(S, v, co_row_len(S, v));
    int32_t color = -1;
    co_word extra = 0;
    for (int64_t lo = 0; lo < need; lo += S.window) {   // (workgroup-uniform)
        const int32_t nb = (int32_t) (need - lo < S.window ? need - lo : S.window);
        const int nwords = (nb + 31) >> 5;
        for (int i = tid; i < nwords; i += nt) bits[i] = 0;
        if (tid == 0) *s_found = CO_NONE;
        __syncthreads();
        co_walk(S, v, true, tid, nt, [&](int32_t color_w) {
            const int64_t c = (int64_t) color_w - lo;
            if (color_w >= 0 && c >= 0 && c < nb) atomicOr(&bits[c >> 5], 1u << (c & 31));
        });
        __syncthreads();
        for (int i = tid; i < nwords; i += nt) {
            const unsigned int word = bits[i];
            if (word != CO_NONE) {
                const unsigned int at = (unsigned int) i * 32 + __builtin_ctz(~word);
                if (at < (unsigned int) nb) atomicMin(s_found, at);   // (the last word's bits at and above nb are no colours of this window)
                break;
            }
        }
        __syncthreads();
        const unsigned int f = *s_found;
        __syncthreads();
        if (f != CO_NONE) {
            color = (int32_t) (lo + f);
            break;
        }
        extra++;
    }
    if (tid == 0) {
        S.color[v] = color;
        if (extra) atomicAdd(&S.ctl->passes, extra);
    }
}
__global__ void __launch_bounds__(CO_BLOCK_THREADS) color_block_kernel(co_state S, const int32_t* __restrict__ list, int64_t n) {
    extern __shared__ unsigned int s_dyn[];
    __shared__ unsigned int s_found;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) co_color_block(S, list[i], s_dyn, &s_found);
}

// ---- release on the grid
// the offsets of a short queue (n <= CO_SMALL entries), both directions in one launch of one workgroup: off[d][0 .. n] =
// the running sums of the rows' lengths, what gmx_frontier_offsets computes with a gather, a device scan and a memset per
// direction.  Most rounds are short (the dense core readies a few vertices a round) and a round is bound by its launches.
__global__ void __launch_bounds__(CO_THREADS) color_offsets_kernel(co_state S, const int32_t* __restrict__ queue, int n, int64_t* __restrict__ off0,
                                                                   int64_t* __restrict__ off1) {
    __shared__ int64_t s_wave[2][CO_THREADS >> 6];
    constexpr int K = CO_SMALL / CO_THREADS;   // consecutive entries a thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t len[2][K], sum[2] = {0, 0}, incl[2];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int i = tid * K + j;
        const int32_t v = i < n ? queue[i] : 0;
        for (int d = 0; d < 2; d++) {
            len[d][j] = i < n ? (int64_t) S.beg[d][v + 1] - S.beg[d][v] : 0;
            sum[d] += len[d][j];
        }
    }
    for (int d = 0; d < 2; d++) {
        int64_t x = sum[d];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        incl[d] = x;
        if (lane == 63) s_wave[d][wave] = x;
    }
    __syncthreads();
    for (int d = 0; d < 2; d++) {
        int64_t run = incl[d] - sum[d];
        for (int w = 0; w < wave; w++) run += s_wave[d][w];
        int64_t* __restrict__ off = d ? off1 : off0;
#pragma unroll
        for (int j = 0; j < K; j++) {
            const int i = tid * K + j;
            if (i < n) off[i] = run;
            run += len[d][j];
            if (i == n - 1) off[n] = run;
        }
    }
}

// one merge-path tile one merge-path tile of the rows (direction dir) of queue[0, n), the round just coloured
__global__ void __launch_bounds__(CO_THREADS) color_release_kernel(co_state S, int dir, const int32_t* __restrict__ queue, int64_t n,
                                                                   const int64_t* __restrict__ off, int64_t m, int32_t next_round) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_v[BFS_ITEMS + 2];
    __shared__ int32_t s_list[BFS_ITEMS];
    __shared__ int64_t s_split[2][2];
    __shared__ unsigned int s_n;
    __shared__ co_word s_m[2], s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_n = 0;
        s_m[0] = s_m[1] = 0;
    }
    const int32_t* __restrict__ idx = S.idx[dir];
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.beg[dir], queue, n, off, m, s_off, s_row, [&](int i, int32_t v, bool) { s_v[i] = v; });
    if (t.e1 <= t.e0) return;   // (workgroup-uniform)
    constexpr int K = BFS_ITEMS / CO_THREADS;
    int32_t w[K], c[K];
    bool act[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int64_t x = t.e0 + tid + (int64_t) j * CO_THREADS;
        const int64_t xc = x < t.e1 ? x : t.e0;   // (loads stay unconditional: a slot that exists)
        const int lo = frontier_slot(s_off, nv, xc);
        w[j] = idx[(int64_t) s_row[lo] + (xc - s_off[lo])];
        act[j] = x < t.e1 && w[j] != s_v[lo];
    }
#pragma unroll
    for (int j = 0; j < K; j++) c[j] = S.color[w[j]];
#pragma unroll
    for (int j = 0; j < K; j++) {
        bool last = false;
        if (act[j] && c[j] < 0) last = atomicSub(&S.pend[w[j]], 1) == 1;
        co_append(S, last, w[j], next_round, s_list, &s_n, &S.ctl->wtail, &S.ctl->btail, s_m, lane);
    }
    __syncthreads();
    frontier_flush(s_list, s_n, &S.ctl->qtail, S.q, &s_base, [&] {
        for (int dd = 0; dd < 2; dd++)
            if (s_m[dd]) atomicAdd(&S.ctl->slots[dd], s_m[dd]);
    });
}

// ---- the tail: one workgroup goes on from the host's state -- round `round` is to colour the queue segment [qs, qe), whose
// rows hold m0 + m1 slots, with its wave rows lw[ws, we) and its block rows lb[bs, be) -- until a round readies nobody
// (CO_DONE) or a queue holds more than tail_from entries + slots (CO_HANDBACK).  color[], depth[], q[] and the lists are
// plain stores of this workgroup, read behind its barrier; pend[] is touched by atomics alone.
__global__ void __launch_bounds__(CO_TAIL_THREADS) color_tail_kernel(co_state S, int32_t round, int64_t qs, int64_t qe, int64_t ws, int64_t we, int64_t bs,
                                                                     int64_t be, int64_t m0, int64_t m1, int64_t tail_from) {
    extern __shared__ unsigned int s_dyn[];   // the block window, or a slice per wave
    __shared__ unsigned int s_tail, s_wt, s_bt, s_found;
    __shared__ co_word s_m[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = blockDim.x >> 6;
    if (tid == 0) {
        s_tail = (unsigned int) qe;
        s_wt = (unsigned int) we;
        s_bt = (unsigned int) be;
        s_m[0] = s_m[1] = 0;
    }
    __syncthreads();
    co_word tot[2] = {0, 0};   // row slots of what this launch queued
    long long rounds = 0;
    int state = CO_DONE;
    while (qs < qe) {
        if ((qe - qs) + m0 + m1 > tail_from) {
            state = CO_HANDBACK;
            break;
        }
        for (int64_t i0 = qs + wave * 4; i0 < qe; i0 += nwaves * 4) co_color_group(S, S.q, i0, qe, lane);
        for (int64_t i = ws + wave; i < we; i += nwaves) co_color_wave(S, S.lw[i], s_dyn + wave * CO_WAVE_WORDS, lane);
        __syncthreads();
        for (int64_t i = bs; i < be; i++) co_color_block(S, S.lb[i], s_dyn, &s_found);
        __syncthreads();
        const auto load = [&](bool, int32_t v, int32_t) { return v; };
        for (int dir = 0; dir < 2; dir++) {
            const int32_t* __restrict__ idx = S.idx[dir];
            const auto slot = [&](bool on, int32_t u, int32_t e) {
                const int32_t w = on ? idx[e] : u;
                bool last = false;
                if (w != u && S.color[w] < 0) last = atomicSub(&S.pend[w], 1) == 1;
                co_append(S, last, w, round + 1, S.q, &s_tail, &s_wt, &s_bt, s_m, lane);
            };
            tail_rows<CO_TAIL_LANE>(S.q + qs, qe - qs, S.beg[dir], lane, wave, nwaves, load, slot);
        }
        __syncthreads();
        rounds++;
        round++;
        qs = qe;
        ws = we;
        bs = be;
        qe = (int64_t) s_tail;
        we = (int64_t) s_wt;
        be = (int64_t) s_bt;
        m0 = (int64_t) s_m[0];
        m1 = (int64_t) s_m[1];
        tot[0] += (co_word) m0;
        tot[1] += (co_word) m1;
        __syncthreads();
        if (tid == 0) s_m[0] = s_m[1] = 0;
        __syncthreads();
    }
    if (tid == 0) {
        co_ctl* c = S.ctl;
        c->qtail = (co_word) s_tail;
        c->wtail = (co_word) s_wt;
        c->btail = (co_word) s_bt;
        c->slots[0] += tot[0];
        c->slots[1] += tot[1];
        c->t_qs = qs;
        c->t_qe = qe;
        c->t_ws = ws;
        c->t_we = we;
        c->t_bs = bs;
        c->t_be = be;
        c->t_rounds = rounds;
        c->t_m[0] = m0;
        c->t_m[1] = m1;
        c->t_state = state;
    }
}

// ---- the largest colour, the size of class 0 and (never) the vertices left without a colour
__global__ void __launch_bounds__(CO_THREADS) color_finish_kernel(const int32_t* __restrict__ color, int64_t V, co_ctl* __restrict__ ctl) {
    int32_t mx = -1;
    co_word zero = 0, left = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const int32_t c = color[v];
        mx = max(mx, c);
        zero += c == 0;
        left += c < 0;
    }
    mx = wave_max(mx);
    zero = wave_sum(zero);
    left = wave_sum(left);
    if ((threadIdx.x & 63) == 0) {
        if (mx > 0) atomicMax(&ctl->maxcolor, mx);
        if (zero) atomicAdd(&ctl->class0, zero);
        if (left) atomicAdd(&ctl->left, left);
    }
}

// ------------------------------------------------------------------ host
extern "C" int gmx_coloring(gmx_graph_t* g, const int32_t* prio_host, int32_t* color_host, int32_t* depth_host, int32_t* num_colors,
                            gmx_stats_t* stats_out) {
    GMX_REQUIRE(color_host, "NULL argument");
    GMX_REQUIRE(g, "NULL argument");
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    if (num_colors) *num_colors = 0;
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    if (!g->has_reverse) {
        gmx_set_error("coloring: a vertex's neighbours are its out-row and its in-row: the reverse CSR is needed");
        return GMX_ERR_STATE;
    }
    // read at every call; neither the result nor the statistics depend on them
    const int64_t tail_from = gmx_env_int("GMX_COLOR_TAIL", CO_TAIL, 0, INT64_MAX);
    const int32_t wave_min = (int32_t) gmx_env_int("GMX_COLOR_WAVE_MIN", CO_WAVE_MIN, 0, CO_WAVE_MIN);
    const int32_t block_min = (int32_t) gmx_env_int("GMX_COLOR_BLOCK_MIN", CO_BLOCK_MIN, 0, CO_BLOCK_MAX);
    const int32_t window = (int32_t) (gmx_env_int("GMX_COLOR_WINDOW", CO_WINDOW, 64, CO_WINDOW) & ~(int64_t) 63);
    const bool phase_log = getenv("GMX_COLOR_PHASES") != nullptr;   // per-phase times for tools/color_prof.py

    gmx_ws_scope scope;
    wbuf<int32_t> prio, pend, npred, color, depth, q, lw, lb;
    wbuf<co_word> key;
    wbuf<co_ctl> ctl;
    if (prio_host) GMX_CHECK(prio.alloc(V));
    GMX_CHECK(key.alloc(V));
    GMX_CHECK(pend.alloc(V));
    GMX_CHECK(npred.alloc(V));
    GMX_CHECK(color.alloc(V));
    if (depth_host) GMX_CHECK(depth.alloc(V));
    GMX_CHECK(q.alloc(V));
    GMX_CHECK(lw.alloc(V));
    GMX_CHECK(lb.alloc(V));
    GMX_CHECK(ctl.alloc(1));

    co_state S;
    S.beg[0] = g->begin.p;
    S.idx[0] = g->node_idx.p;
    S.beg[1] = g->r_begin.p;
    S.idx[1] = g->r_node_idx.p;
    S.pend = pend.p;
    S.npred = npred.p;
    S.color = color.p;
    S.depth = depth_host ? depth.p : nullptr;
    S.q = q.p;
    S.lw = lw.p;
    S.lb = lb.p;
    S.ctl = ctl.p;
    S.V = V;
    S.wave_min = wave_min;
    S.block_min = block_min;
    S.window = window;

    frontier_scan fs[2];
    for (int d = 0; d < 2; d++) GMX_CHECK(gmx_frontier_scan_alloc(&fs[d], (size_t) V, 0));
    gmx_pinned<co_ctl> h_ctl;
    GMX_CHECK(h_ctl.alloc());
    const co_ctl* h = h_ctl.p;
    gmx_spans tm;
    const int gv = grid_for(V);
    enum { PH_COUNT, PH_GROUP, PH_WAVE, PH_BLOCK, PH_RELEASE, PH_TAIL, PH_N };
    float ph_ms[PH_N] = {0, 0, 0, 0, 0, 0};   // (GMX_COLOR_PHASES): device time around every step, which
    gmx_phase_clock phase;                    // synchronises: the profiler's mode only
    GMX_CHECK(phase.enable(phase_log));
    const size_t block_lds = (size_t) window / 8;
    const size_t tail_lds = std::max(block_lds, sizeof(unsigned int) * (CO_TAIL_THREADS >> 6) * CO_WAVE_WORDS);

    // ---- the priorities
    GMX_CHECK(tm.begin(tm.H2D));
    if (prio_host) GMX_HIP(hipMemcpy(prio.p, prio_host, sizeof(int32_t) * (size_t) V, hipMemcpyHostToDevice));
    GMX_CHECK(tm.end(tm.H2D));

    // ---- count
    GMX_CHECK(tm.begin(tm.KERNEL));
    phase.begin();
    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(co_ctl), 0));
    GMX_HIP(hipMemsetAsync(pend.p, 0, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(color.p, 0xff, sizeof(int32_t) * (size_t) V, 0));
    hipLaunchKernelGGL(color_key_kernel, dim3(gv), dim3(CO_THREADS), 0, 0, (const int32_t*) g->begin.p, (const int32_t*) g->r_begin.p,
                       prio_host ? (const int32_t*) prio.p : (const int32_t*) nullptr, V, key.p);
    if (E > 0)
        hipLaunchKernelGGL(color_count_kernel, dim3(grid_for(E, BFS_ITEMS)), dim3(CO_THREADS), 0, 0, (const int32_t*) g->begin.p,
                           (const int32_t*) g->node_idx.p, V, E, (const co_word*) key.p, pend.p);
    hipLaunchKernelGGL(color_seed_kernel, dim3(grid_for(V, BFS_ITEMS)), dim3(CO_THREADS), 0, 0, S);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_read_back(h_ctl, (const co_ctl*) ctl.p));
    phase.end(&ph_ms[PH_COUNT]);

    // ---- rounds: colour the segment [qs, qe) of every list, then release its rows
    int64_t qs = 0, qe = (int64_t) h->qtail, ws = 0, we = (int64_t) h->wtail, bs = 0, be = (int64_t) h->btail;
    int64_t at_qs[2] = {0, 0}, at_qe[2] = {(int64_t) h->slots[0], (int64_t) h->slots[1]};   // row slots of q[0, qs) and q[0, qe)
    int64_t grid_rounds = 0, tail_rounds = 0;
    int32_t round = 0;
    while (qs < qe) {
        const int64_t n = qe - qs;
        const int64_t m[2] = {at_qe[0] - at_qs[0], at_qe[1] - at_qs[1]};
        if (tail_from > 0 && n + m[0] + m[1] <= tail_from) {
            phase.begin();
            hipLaunchKernelGGL(color_tail_kernel, dim3(1), dim3(CO_TAIL_THREADS), tail_lds, 0, S, round, qs, qe, ws, we, bs, be, m[0], m[1], tail_from);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, (const co_ctl*) ctl.p));
            phase.end(&ph_ms[PH_TAIL]);
            tail_rounds += h->t_rounds;
            round += (int32_t) h->t_rounds;
            qs = h->t_qs;
            qe = h->t_qe;
            ws = h->t_ws;
            we = h->t_we;
            bs = h->t_bs;
            be = h->t_be;
            for (int d = 0; d < 2; d++) {
                at_qe[d] = (int64_t) h->slots[d];
                at_qs[d] = at_qe[d] - h->t_m[d];
            }
            if (h->t_state == CO_DONE) break;
            continue;   // CO_HANDBACK: the round it stopped at is too large for one workgroup and runs on the grid
        }
        phase.begin();
        hipLaunchKernelGGL(color_group_kernel, dim3(grid_for(n, CO_THREADS / 16)), dim3(CO_THREADS), 0, 0, S, (const int32_t*) (q.p + qs), n);
        phase.end(&ph_ms[PH_GROUP]);
        if (we > ws) {
            phase.begin();
            hipLaunchKernelGGL(color_wave_kernel, dim3(grid_for(we - ws, CO_THREADS / 64)), dim3(CO_THREADS), 0, 0, S, (const int32_t*) (lw.p + ws), we - ws);
            phase.end(&ph_ms[PH_WAVE]);
        }
        if (be > bs) {
            phase.begin();
            hipLaunchKernelGGL(color_block_kernel, dim3(grid_for(be - bs, 1)), dim3(CO_BLOCK_THREADS), block_lds, 0, S, (const int32_t*) (lb.p + bs), be - bs);
            phase.end(&ph_ms[PH_BLOCK]);
        }
        phase.begin();
        if (n <= CO_SMALL && m[0] + m[1] > 0)
            hipLaunchKernelGGL(color_offsets_kernel, dim3(1), dim3(CO_THREADS), 0, 0, S, (const int32_t*) (q.p + qs), (int) n, fs[0].off.p, fs[1].off.p);
        for (int d = 0; d < 2; d++) {
            if (m[d] == 0) continue;
            if (n > CO_SMALL) GMX_CHECK(gmx_frontier_offsets(S.beg[d], q.p + qs, n, &fs[d], nullptr, false));
            hipLaunchKernelGGL(color_release_kernel, dim3((unsigned) frontier_tiles(n, m[d])), dim3(CO_THREADS), 0, 0, S, d, (const int32_t*) (q.p + qs), n,
                               (const int64_t*) fs[d].off.p, m[d], round + 1);
        }
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctl, (const co_ctl*) ctl.p));
        phase.end(&ph_ms[PH_RELEASE]);
        grid_rounds++;
        round++;
        qs = qe;
        ws = we;
        bs = be;
        qe = (int64_t) h->qtail;
        we = (int64_t) h->wtail;
        be = (int64_t) h->btail;
        for (int d = 0; d < 2; d++) {
            at_qs[d] = at_qe[d];
            at_qe[d] = (int64_t) h->slots[d];
        }
    }
    hipLaunchKernelGGL(color_finish_kernel, dim3(gv), dim3(CO_THREADS), 0, 0, (const int32_t*) color.p, V, ctl.p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(gmx_read_back(h_ctl, (const co_ctl*) ctl.p));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(color_host, color.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    if (depth_host) GMX_HIP(hipMemcpy(depth_host, depth.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    if ((int64_t) h->qtail != V || h->left) {
        gmx_set_error("coloring: %lld of %lld vertices became ready, %lld have no colour", (long long) h->qtail, (long long) V, (long long) h->left);
        return GMX_ERR_HIP;
    }
    const int32_t colors = h->maxcolor + 1;
    if (num_colors) *num_colors = colors;
    stats->iterations = round;
    stats->vertices_reached = (int64_t) h->class0;
    stats->edges_examined = 6 * E;
    if (phase_log)
        fprintf(stderr, "gmx color phases: count %.3f ms, group %.3f ms, wave %.3f ms, block %.3f ms, release %.3f ms, tail %.3f ms\n", ph_ms[PH_COUNT],
                ph_ms[PH_GROUP], ph_ms[PH_WAVE], ph_ms[PH_BLOCK], ph_ms[PH_RELEASE], ph_ms[PH_TAIL]);
    if (getenv("GMX_COLOR_LOG"))
        fprintf(stderr,
                "gmx color: V %lld E %lld user_prio %d rounds %d grid_rounds %lld tail_rounds %lld group %lld wave %lld block %lld passes %lld colors %d class0 %lld\n",
                (long long) V, (long long) E, prio_host ? 1 : 0, (int) round, (long long) grid_rounds, (long long) tail_rounds,
                (long long) (V - (int64_t) h->wtail - (int64_t) h->btail), (long long) h->wtail, (long long) h->btail, (long long) h->passes, (int) colors,
                (long long) h->class0);
    return GMX_OK;
}

void gmx_touch_color() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) color_tail_kernel);
}
