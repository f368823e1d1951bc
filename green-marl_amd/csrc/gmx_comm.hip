// gmx_comm.hip -- label-propagation communities: communities(G, comm) of apps/src/communities.gm, on gfx950.
//
// comm[x] = x; then, until nothing changes, every vertex counts the labels of its out-neighbours (one count per slot)
// and, unless its own label has the highest count, takes the SMALLEST label with the highest count.  The reference
// updates comm in place from many threads; here a round is two half-rounds (gmx.h: half h(v, r) from a murmur3
// finaliser), each evaluated against one snapshot of comm and committed as a whole, which is one interleaving of the
// reference's loop and is deterministic.  Integer counts only; the choice is a pure function of the counts.
//
// A half-round is a chain of launches on the default stream, none of which the host waits for:
//   compact   dirty & in this half & out-degree > 0 -> three row lists by row length; those dirty bits are cleared
//   short     rows below WAVE_MIN slots: 16 lanes per row, labels in registers (two per lane per 32-slot chunk), counted
//             by all-pairs comparison with DPP row rotations; rows longer than a chunk repeat it per pair of chunks
//   wave      rows below BLOCK_MIN: one wave per row, open-addressing table (CAS key, ds_add count) in the wave's LDS slice
//   block     the rest: one workgroup per row, the same table in the workgroup's LDS
//   overflow  rows whose table filled (a row may hold as many distinct labels as slots: round 0): counted again in
//             passes over DISJOINT LABEL CLASSES (fmix32(label) mod 2^k == c), 2^k from the row length, the classes of a
//             row dealt over all workgroups and merged with 64-bit atomicMax; a class that still fills is split further
//   final     the overflowed rows' decisions
//   commit    store the new labels, set the dirty bits of the changed vertices' in-neighbours (reverse rows; the longest
//             ones in a launch of their own, a workgroup each)
//   close     add the half-round's counters into the round's totals record and zero them
// New labels go to a pending list (vertex, label) through per-wave LDS staging: one claim per COMM_STAGE entries.
// The host reads the totals record once per round (pinned memory) to learn whether anything changed.
#include "gmx_internal.h"

#define COMM_THREADS 256
#define COMM_COMPACT_THREADS 1024
#define COMM_CHUNK 32              // slots of a short row held in registers at a time (16 lanes x 2)
#define COMM_EMPTY (-1)
#define COMM_PROBES 64             // linear probes after which a table counts as full
#define COMM_STAGE 256             // pending entries staged per wave before one claim
#define COMM_SHARDS 32             // slot counters (adds to one word retire at ~90 per microsecond)
#define COMM_WAVE_MIN 33           // defaults of GMX_COMM_WAVE_MIN, GMX_COMM_BLOCK_MIN, GMX_COMM_LDS_SLOTS
#define COMM_BLOCK_MIN 256
#define COMM_LDS_SLOTS 4096
#define COMM_LDS_SLOTS_MIN 512
#define COMM_LDS_SLOTS_MAX 16384
#define COMM_REV_BLOCK 2048        // reverse rows longer than this are marked by a workgroup of their own
#define COMM_WAVE_SHARE 8          // a wave's table holds LDS_SLOTS / COMM_WAVE_SHARE slots

enum { K_SHORT, K_WAVE, K_BLOCK, K_OVF, K_PEND, K_BIG, K_SPLIT, K_NCTR };   // list lengths of the running half-round, and its class splits

struct comm_rec {   // totals of one round
    unsigned int changes;
    unsigned int evals[3];       // rows evaluated by regime
    unsigned int overflowed;     // rows whose table filled
    unsigned int splits;         // levels of a label class given up because a part filled (comm_overflow_kernel)
    unsigned long long slots;
};

struct comm_arrays {
    const int32_t* beg;
    const int32_t* idx;
    const int32_t* rbeg;   // NULL: no work list
    const int32_t* ridx;
    int32_t* comm;
    unsigned long long* dirty;       // [(V + 63) / 64]
    int32_t* list[3];                // [V] each
    int32_t* ovf;                    // [V] rows whose table filled
    unsigned long long* ovf_best;    // [V] by position in ovf: (count << 32 | ~label), maximum over the classes
    int32_t* ovf_own;                // [V] count of the row's own label
    int32_t* pend_v;                 // [V]
    int32_t* pend_l;
    int32_t* big;                    // [V] changed vertices with long reverse rows
    unsigned int* ctr;               // [K_NCTR]
    unsigned long long* shard;       // [COMM_SHARDS] slots of the listed rows
    int64_t V;
};

__device__ __forceinline__ uint32_t comm_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// (count, label) ordered by count, then by the SMALLER label
__device__ __forceinline__ unsigned long long comm_key(int32_t cnt, int32_t lab) {
    return ((unsigned long long) (uint32_t) cnt << 32) | (unsigned long long) (0xFFFFFFFFu - (uint32_t) lab);
}
__device__ __forceinline__ int32_t comm_key_label(unsigned long long k) { return (int32_t) (0xFFFFFFFFu - (uint32_t) k); }
__device__ __forceinline__ unsigned long long comm_max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
// LDS written by other lanes of this wave is read after this (a wave's LDS operations execute in order)
__device__ __forceinline__ void comm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------- pending list
struct comm_stage {
    int32_t* v;   // [COMM_STAGE] in the wave's LDS
    int32_t* l;
    int n;        // wave-uniform
};
__device__ __forceinline__ void comm_stage_flush(const comm_arrays& a, comm_stage& s) {
    if (s.n == 0) return;
    const int lane = threadIdx.x & 63;
    unsigned int at = 0;
    if (lane == 0) at = atomicAdd(&a.ctr[K_PEND], (unsigned int) s.n);
    at = __shfl(at, 0, 64);
    comm_wave_sync();
    for (int j = lane; j < s.n; j += 64) {
        a.pend_v[at + j] = s.v[j];
        a.pend_l[at + j] = s.l[j];
    }
    comm_wave_sync();
    s.n = 0;
}
// wave-converged
__device__ __forceinline__ void comm_stage_push(const comm_arrays& a, comm_stage& s, bool p, int32_t v, int32_t l) {
    const unsigned long long m = __ballot(p);
    if (!m) return;
    if (s.n + 64 > COMM_STAGE) comm_stage_flush(a, s);
    const int lane = threadIdx.x & 63;
    if (p) {
        const int k = s.n + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        s.v[k] = v;
        s.l[k] = l;
    }
    s.n += __builtin_popcountll(m);
}
// wave-converged, straight to the list (the few rows of the block and final kernels)
__device__ __forceinline__ void comm_push(const comm_arrays& a, bool p, int32_t v, int32_t l) {
    const unsigned long long m = __ballot(p);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_ctzll(m);
    unsigned int at = 0;
    if (lane == leader) at = atomicAdd(&a.ctr[K_PEND], (unsigned int) __builtin_popcountll(m));
    at = __shfl(at, leader, 64);
    if (p) {
        const unsigned int k = at + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        a.pend_v[k] = v;
        a.pend_l[k] = l;
    }
}

// ---------------------------------------------------------------- init, dirty bits, compaction
// comm = identity; dirty = every vertex with out-edges.  One wave per bitmap word.
__global__ void __launch_bounds__(COMM_THREADS) comm_init_kernel(comm_arrays a, int set_comm) {
    const int lane = threadIdx.x & 63;
    const int64_t nwords = (a.V + 63) >> 6;
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t w = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nwords; w += nwaves) {
        const int64_t v = w * 64 + lane;
        bool has = false;
        if (v < a.V) {
            has = a.beg[v + 1] > a.beg[v];
            if (set_comm) a.comm[v] = (int32_t) v;
        }
        const unsigned long long m = __ballot(has);
        if (lane == 0) a.dirty[w] = m;
    }
}

// dirty & (half < 0 or h(v) == half) -> list[class by row length]; clear: those bits are cleared.  A wave per bitmap word,
// list space claimed once per workgroup and class.
__global__ void __launch_bounds__(COMM_COMPACT_THREADS) comm_compact_kernel(comm_arrays a, uint32_t salt, int half, int32_t wave_min,
                                                                            int32_t block_min, int clear) {
    __shared__ unsigned int s_cnt[3], s_base[3];
    constexpr int WAVES = COMM_COMPACT_THREADS / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t nwords = (a.V + 63) >> 6;
    long long slots = 0;
    for (int64_t w0 = (int64_t) blockIdx.x * WAVES; w0 < nwords; w0 += (int64_t) gridDim.x * WAVES) {
        if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        const int64_t w = w0 + wid;
        const int64_t v = w * 64 + lane;
        const unsigned long long word = w < nwords ? a.dirty[w] : 0ull;
        bool sel = ((word >> lane) & 1ull) && v < a.V;
        if (sel && half >= 0) sel = (int) (comm_fmix32((uint32_t) v ^ salt) & 1u) == half;
        int32_t d = 0;
        if (sel) {
            d = a.beg[v + 1] - a.beg[v];
            sel = d > 0;
        }
        const unsigned long long msel = __ballot(sel);
        if (clear && lane == 0 && msel) a.dirty[w] = word & ~msel;
        if (sel) slots += d;
        const int cls = d >= block_min ? 2 : (d >= wave_min ? 1 : 0);
        unsigned int mine = 0;
        for (int c = 0; c < 3; c++) {
            const unsigned long long mc = __ballot(sel && cls == c);
            if (!mc) continue;
            unsigned int at = 0;
            if (lane == 0) at = atomicAdd(&s_cnt[c], (unsigned int) __builtin_popcountll(mc));
            at = __shfl(at, 0, 64);
            if (sel && cls == c) mine = at + __builtin_popcountll(mc & ((1ull << lane) - 1ull));
        }
        __syncthreads();
        if (threadIdx.x < 3 && s_cnt[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&a.ctr[threadIdx.x], s_cnt[threadIdx.x]);
        __syncthreads();
        if (sel) a.list[cls][s_base[cls] + mine] = (int32_t) v;
    }
    for (int o = 32; o; o >>= 1) slots += __shfl_xor(slots, o, 64);
    if (lane == 0 && slots) atomicAdd(&a.shard[(blockIdx.x * WAVES + wid) & (COMM_SHARDS - 1)], (unsigned long long) slots);
}

// ---------------------------------------------------------------- short rows: 16 lanes per row, comparison only
template <int N>
__device__ __forceinline__ int32_t comm_ror16(int32_t x) {   // the value of the lane N places on inside the 16-lane row
    return __builtin_amdgcn_update_dpp(0, x, 0x120 + N, 0xf, 0xf, false);
}
// c0 / c1 += how often l0 / l1 occur among the 32 labels (m0, m1) of the row's 16 lanes
#define COMM_ROT(N)                                                    \
    {                                                                  \
        const int32_t o0 = comm_ror16<N>(m0), o1 = comm_ror16<N>(m1); \
        c0 += (o0 == l0) + (o1 == l0);                                 \
        c1 += (o0 == l1) + (o1 == l1);                                 \
    }
__device__ __forceinline__ void comm_count32(int32_t l0, int32_t l1, int32_t m0, int32_t m1, int32_t& c0, int32_t& c1) {
    c0 += (m0 == l0) + (m1 == l0);
    c1 += (m0 == l1) + (m1 == l1);
    COMM_ROT(1) COMM_ROT(2) COMM_ROT(3) COMM_ROT(4) COMM_ROT(5) COMM_ROT(6) COMM_ROT(7) COMM_ROT(8)
    COMM_ROT(9) COMM_ROT(10) COMM_ROT(11) COMM_ROT(12) COMM_ROT(13) COMM_ROT(14) COMM_ROT(15)
}

__global__ void __launch_bounds__(COMM_THREADS) comm_short_kernel(comm_arrays a) {
    __shared__ int32_t s_stage[COMM_THREADS / 64][2 * COMM_STAGE];
    const int lane = threadIdx.x & 63, sub = lane & 15, wid = threadIdx.x >> 6;
    comm_stage st{s_stage[wid], s_stage[wid] + COMM_STAGE, 0};
    const int64_t n = a.ctr[K_SHORT];
    const int32_t* __restrict__ list = a.list[K_SHORT];
    const int64_t wave = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t base = wave * 4; base < n; base += nwaves * 4) {
        const int64_t i = base + (lane >> 4);
        const bool act = i < n;
        const int32_t v = act ? list[i] : 0;
        const int32_t b = act ? a.beg[v] : 0, len = act ? a.beg[v + 1] - b : 0;
        const int32_t own = act ? a.comm[v] : -1;
        int32_t mx = len;
        for (int o = 32; o; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
        unsigned long long best = 0;
        int32_t ownc = 0;
        // candidates: the chunk at ca; counted against every chunk of the row (the loops are wave-uniform: DPP reads
        // the neighbouring lanes)
        for (int32_t ca = 0; ca < mx; ca += COMM_CHUNK) {
            const int32_t l0 = ca + sub < len ? a.comm[a.idx[b + ca + sub]] : -1;
            const int32_t l1 = ca + 16 + sub < len ? a.comm[a.idx[b + ca + 16 + sub]] : -1;
            int32_t c0 = 0, c1 = 0;
            for (int32_t cb = 0; cb < mx; cb += COMM_CHUNK) {
                int32_t m0 = l0, m1 = l1;
                if (cb != ca) {
                    m0 = cb + sub < len ? a.comm[a.idx[b + cb + sub]] : -1;
                    m1 = cb + 16 + sub < len ? a.comm[a.idx[b + cb + 16 + sub]] : -1;
                }
                comm_count32(l0, l1, m0, m1, c0, c1);
            }
            if (l0 >= 0) {
                best = comm_max64(best, comm_key(c0, l0));
                if (l0 == own) ownc = c0;
            }
            if (l1 >= 0) {
                best = comm_max64(best, comm_key(c1, l1));
                if (l1 == own) ownc = c1;
            }
        }
        for (int o = 8; o; o >>= 1) {
            best = comm_max64(best, __shfl_xor(best, o, 64));
            ownc = max(ownc, __shfl_xor(ownc, o, 64));
        }
        const bool change = act && sub == 0 && len > 0 && ownc != (int32_t) (best >> 32);
        comm_stage_push(a, st, change, v, comm_key_label(best));
    }
    comm_stage_flush(a, st);
}

// ---------------------------------------------------------------- table rows: NT = 64 (a wave) or COMM_THREADS (the workgroup)
template <int NT>
__device__ __forceinline__ void comm_group_sync() {
    if (NT == 64) comm_wave_sync();
    else __syncthreads();
}

// One pass of NT threads over row [b, e): the labels of class c (fmix32(label) mod 2^lp == c) are counted in the table
// keys / cnts [cap] (cap a power of two), then every thread folds the table entries it scans into best / ownc.
// true: an insert found no slot within COMM_PROBES (the same answer in every thread); best / ownc are then untouched.
template <int NT>
__device__ bool comm_count_pass(const comm_arrays& a, int32_t b, int32_t e, int32_t* keys, int32_t* cnts, int32_t cap, int lp, uint32_t c,
                                int tid, int* s_full, int32_t own, unsigned long long& best, int32_t& ownc) {
    const int lane = threadIdx.x & 63;
    for (int32_t s = tid; s < cap; s += NT) {
        keys[s] = COMM_EMPTY;
        cnts[s] = 0;
    }
    if (tid == 0) *s_full = 0;
    comm_group_sync<NT>();
    const uint32_t mask = (uint32_t) cap - 1u, pmask = (1u << lp) - 1u;
    const int limit = cap < COMM_PROBES ? cap : COMM_PROBES;
    volatile int32_t* vkeys = keys;
    volatile int* vfull = s_full;
    constexpr int U = 4;   // slots per thread and step: the gathers of a step are in flight together
    for (int32_t j0 = b; j0 < e; j0 += NT * U) {   // (uniform over the wave: ballots inside)
        if (__builtin_amdgcn_readfirstlane(*vfull)) break;   // somebody found no slot: the pass is void anyway
        int32_t nb[U], labs[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int32_t j = j0 + u * NT + tid;
            nb[u] = j < e ? a.idx[j] : -1;
        }
#pragma unroll
        for (int u = 0; u < U; u++) labs[u] = nb[u] >= 0 ? a.comm[nb[u]] : -1;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int32_t lab = labs[u];
            const uint32_t h = comm_fmix32((uint32_t) lab);
            const bool in = lab >= 0 && (h & pmask) == c;
            // the lanes that hold the first lane's label add once for all of them (a converged row is one label)
            int add = in ? 1 : 0;
            const unsigned long long m = __ballot(in);
            if (m) {
                const int first = __builtin_ctzll(m);
                const int32_t flab = __shfl(lab, first, 64);
                const unsigned long long same = __ballot(in && lab == flab);
                if (in && lab == flab) add = lane == first ? __builtin_popcountll(same) : 0;
            }
            if (add) {
                uint32_t s = (h >> lp) & mask;
                int i = 0;
                for (; i < limit; i++) {
                    const int32_t k = vkeys[s];
                    if (k == lab) break;
                    if (k == COMM_EMPTY) {
                        const int32_t old = atomicCAS(&keys[s], COMM_EMPTY, lab);
                        if (old == COMM_EMPTY || old == lab) break;
                    }
                    s = (s + 1u) & mask;
                }
                if (i < limit) atomicAdd(&cnts[s], add);
                else *vfull = 1;
            }
        }
    }
    comm_group_sync<NT>();
    const bool f = *s_full != 0;
    if (!f)
        for (int32_t s = tid; s < cap; s += NT) {
            const int32_t k = keys[s];
            if (k >= 0) {
                const int32_t cn = cnts[s];
                best = comm_max64(best, comm_key(cn, k));
                if (k == own) ownc = cn;
            }
        }
    comm_group_sync<NT>();   // (the next pass clears the table)
    return f;
}

// the part of a table a row of len slots uses: at least four slots per row slot (clearing and scanning the rest is wasted)
__device__ __forceinline__ int32_t comm_table_for(int32_t len, int32_t cap) {
    while (cap > 64 && cap / 8 >= len) cap >>= 1;
    return cap;
}
__device__ __forceinline__ void comm_wave_reduce(unsigned long long& best, int32_t& ownc) {
    for (int o = 32; o; o >>= 1) {
        best = comm_max64(best, __shfl_xor(best, o, 64));
        ownc = max(ownc, __shfl_xor(ownc, o, 64));
    }
}
// every thread of the workgroup gets the maximum
__device__ __forceinline__ void comm_block_reduce(unsigned long long& best, int32_t& ownc, unsigned long long* s_best, int32_t* s_own) {
    comm_wave_reduce(best, ownc);
    if ((threadIdx.x & 63) == 0) {
        s_best[threadIdx.x >> 6] = best;
        s_own[threadIdx.x >> 6] = ownc;
    }
    __syncthreads();
    for (int w = 0; w < COMM_THREADS / 64; w++) {
        best = comm_max64(best, s_best[w]);
        ownc = max(ownc, s_own[w]);
    }
    __syncthreads();
}
// (one thread) row v's table filled: to the overflow list
__device__ __forceinline__ void comm_overflow(const comm_arrays& a, int32_t v) {
    const unsigned int at = atomicAdd(&a.ctr[K_OVF], 1u);
    a.ovf[at] = v;
    a.ovf_best[at] = 0ull;
    a.ovf_own[at] = 0;
}

// one wave per row; dynamic LDS: per wave keys[cap], cnts[cap], the staged pending entries and the full flag
__global__ void __launch_bounds__(COMM_THREADS) comm_wave_kernel(comm_arrays a, int32_t cap) {
    extern __shared__ int32_t comm_lds[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t* mine = comm_lds + (size_t) wid * (2 * cap + 2 * COMM_STAGE + 4);
    int32_t *keys = mine, *cnts = mine + cap;
    comm_stage st{mine + 2 * cap, mine + 2 * cap + COMM_STAGE, 0};
    int* s_full = mine + 2 * cap + 2 * COMM_STAGE;
    const int64_t n = a.ctr[K_WAVE];
    const int32_t* __restrict__ list = a.list[K_WAVE];
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t i = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
        const int32_t v = list[i];
        const int32_t b = a.beg[v], e = a.beg[v + 1], own = a.comm[v];
        unsigned long long best = 0;
        int32_t ownc = 0;
        const bool full = comm_count_pass<64>(a, b, e, keys, cnts, comm_table_for(e - b, cap), 0, 0u, lane, s_full, own, best, ownc);
        if (full) {
            if (lane == 0) comm_overflow(a, v);
            continue;
        }
        comm_wave_reduce(best, ownc);
        comm_stage_push(a, st, lane == 0 && ownc != (int32_t) (best >> 32), v, comm_key_label(best));
    }
    comm_stage_flush(a, st);
}

// one workgroup per row; dynamic LDS: keys[cap], cnts[cap]
__global__ void __launch_bounds__(COMM_THREADS) comm_block_kernel(comm_arrays a, int32_t cap) {
    extern __shared__ int32_t comm_lds[];
    __shared__ unsigned long long s_best[COMM_THREADS / 64];
    __shared__ int32_t s_own[COMM_THREADS / 64];
    __shared__ int s_full;
    int32_t *keys = comm_lds, *cnts = comm_lds + cap;
    const int64_t n = a.ctr[K_BLOCK];
    const int32_t* __restrict__ list = a.list[K_BLOCK];
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t v = list[i];
        const int32_t b = a.beg[v], e = a.beg[v + 1], own = a.comm[v];
        unsigned long long best = 0;
        int32_t ownc = 0;
        const bool full = comm_count_pass<COMM_THREADS>(a, b, e, keys, cnts, comm_table_for(e - b, cap), 0, 0u, threadIdx.x, &s_full, own, best, ownc);
        if (full) {
            if (threadIdx.x == 0) comm_overflow(a, v);
            continue;
        }
        comm_block_reduce(best, ownc, s_best, s_own);
        if (threadIdx.x < 64) comm_push(a, threadIdx.x == 0 && ownc != (int32_t) (best >> 32), v, comm_key_label(best));
    }
}

// The overflowed rows: row i is counted in 2^lp0 label classes, lp0 from its length (half a table of distinct labels per
// class if every slot differs), class c0 by workgroup c0 mod gridDim.  A class that fills all the same is split by the
// next hash bit until its parts fit (fmix32 is a bijection: at 31 bits a class holds two labels).  Merged by atomicMax.
__global__ void __launch_bounds__(COMM_THREADS) comm_overflow_kernel(comm_arrays a, int32_t cap) {
    extern __shared__ int32_t comm_lds[];
    __shared__ unsigned long long s_best[COMM_THREADS / 64];
    __shared__ int32_t s_own[COMM_THREADS / 64];
    __shared__ int s_full;
    int32_t *keys = comm_lds, *cnts = comm_lds + cap;
    __shared__ unsigned long long s_mine[COMM_THREADS / 64];
    const int64_t n = a.ctr[K_OVF];
    for (int64_t i0 = 0; i0 < n; i0 += COMM_THREADS) {
      // which of these COMM_THREADS rows have a class for this workgroup (row i's class c0 goes to workgroup (c0 + i) mod gridDim)
      {
        const int64_t i = i0 + threadIdx.x;
        bool has = false;
        if (i < n) {
            const int32_t v = a.ovf[i];
            const int32_t len = a.beg[v + 1] - a.beg[v];
            int lp0 = 0;
            while (lp0 < 31 && (len >> lp0) > cap / 2) lp0++;
            has = (uint32_t) ((blockIdx.x + gridDim.x - (uint32_t) (i % gridDim.x)) % gridDim.x) < (1u << lp0);
        }
        const unsigned long long m = __ballot(has);
        if ((threadIdx.x & 63) == 0) s_mine[threadIdx.x >> 6] = m;
        __syncthreads();
      }
      for (int k = 0; k < COMM_THREADS; k++) {
        if (!((s_mine[k >> 6] >> (k & 63)) & 1ull)) continue;
        const int64_t i = i0 + k;
        const int32_t v = a.ovf[i];
        const int32_t b = a.beg[v], e = a.beg[v + 1], own = a.comm[v];
        int lp0 = 0;
        while (lp0 < 31 && ((e - b) >> lp0) > cap / 2) lp0++;
        const uint32_t P0 = 1u << lp0;
        for (uint32_t c0 = (blockIdx.x + gridDim.x - (uint32_t) (i % gridDim.x)) % gridDim.x; c0 < P0; c0 += gridDim.x) {
            unsigned long long best = 0;
            int32_t ownc = 0;
            for (int lp = lp0; lp <= 31; lp++) {
                unsigned long long tb = 0;
                int32_t to = 0;
                bool full = false;
                const uint64_t P = 1ull << lp;
                for (uint64_t c = c0; c < P && !full; c += P0)
                    full = comm_count_pass<COMM_THREADS>(a, b, e, keys, cnts, cap, lp, (uint32_t) c, threadIdx.x, &s_full, own, tb, to);
                if (!full) {
                    best = tb;
                    ownc = to;
                    break;
                }
                if (threadIdx.x == 0) atomicAdd(&a.ctr[K_SPLIT], 1u);
            }
            comm_block_reduce(best, ownc, s_best, s_own);
            if (threadIdx.x == 0) {
                if (best) atomicMax(&a.ovf_best[i], best);
                if (ownc) atomicMax(&a.ovf_own[i], ownc);
            }
        }
      }
      __syncthreads();   // (s_mine is rewritten for the next batch)
    }
}
__global__ void __launch_bounds__(COMM_THREADS) comm_final_kernel(comm_arrays a) {
    const int64_t n = a.ctr[K_OVF];
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t base = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) & ~63ll; base < n; base += stride) {
        const int64_t i = base + (threadIdx.x & 63);
        bool change = false;
        int32_t v = 0, lab = 0;
        if (i < n) {
            const unsigned long long best = a.ovf_best[i];
            v = a.ovf[i];
            lab = comm_key_label(best);
            change = a.ovf_own[i] != (int32_t) (best >> 32);
        }
        comm_push(a, change, v, lab);
    }
}

// ---------------------------------------------------------------- commit and close
__device__ __forceinline__ void comm_mark(const comm_arrays& a, int32_t u) {
    const unsigned long long bit = 1ull << (u & 63);
    if (!(a.dirty[u >> 6] & bit)) atomicOr(&a.dirty[u >> 6], bit);
}
// comm[v] = l for the pending entries; with a reverse CSR the in-neighbours of v become dirty: reverse rows up to 16
// slots one per lane, up to COMM_REV_BLOCK by the whole wave, longer ones are listed for comm_commit_big_kernel (one wave
// walking a hub's in-row alone was the longest thing in a round)
__global__ void __launch_bounds__(COMM_THREADS) comm_commit_kernel(comm_arrays a) {
    const int lane = threadIdx.x & 63;
    const int64_t n = a.ctr[K_PEND];
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t base = (((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 64; base < n; base += nwaves * 64) {
        const int64_t i = base + lane;
        const bool act = i < n;
        const int32_t v = act ? a.pend_v[i] : 0;
        if (act) a.comm[v] = a.pend_l[i];
        if (!a.rbeg) continue;
        const int32_t b = act ? a.rbeg[v] : 0, e = act ? a.rbeg[v + 1] : 0;
        const bool big = e - b > 16 && e - b <= COMM_REV_BLOCK;
        if (e - b <= 16)
            for (int32_t j = b; j < e; j++) comm_mark(a, a.ridx[j]);
        const unsigned long long mh = __ballot(e - b > COMM_REV_BLOCK);
        if (mh) {
            unsigned int at = 0;
            if (lane == 0) at = atomicAdd(&a.ctr[K_BIG], (unsigned int) __builtin_popcountll(mh));
            at = __shfl(at, 0, 64);
            if (e - b > COMM_REV_BLOCK) a.big[at + __builtin_popcountll(mh & ((1ull << lane) - 1ull))] = v;
        }
        unsigned long long m = __ballot(big);
        while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const int32_t bb = __shfl(b, src, 64), ee = __shfl(e, src, 64);
            for (int32_t j = bb + lane; j < ee; j += 64) comm_mark(a, a.ridx[j]);
        }
    }
}
// the listed long reverse rows, one workgroup per row, four slots per thread in flight
__global__ void __launch_bounds__(COMM_THREADS) comm_commit_big_kernel(comm_arrays a) {
    const int64_t n = a.ctr[K_BIG];
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t v = a.big[i];
        const int32_t b = a.rbeg[v], e = a.rbeg[v + 1];
        for (int32_t j0 = b + (int32_t) threadIdx.x; j0 < e; j0 += 4 * COMM_THREADS) {
            int32_t u[4];
#pragma unroll
            for (int k = 0; k < 4; k++) u[k] = j0 + k * COMM_THREADS < e ? a.ridx[j0 + k * COMM_THREADS] : -1;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (u[k] >= 0) comm_mark(a, u[k]);
        }
    }
}
// one wave: the half-round's counters into rec, then zeroed
__global__ void comm_close_kernel(comm_arrays a, comm_rec* rec) {
    const int lane = threadIdx.x;
    unsigned long long s = lane < COMM_SHARDS ? a.shard[lane] : 0ull;
    if (lane < COMM_SHARDS) a.shard[lane] = 0ull;
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        rec->slots += s;
        rec->changes += a.ctr[K_PEND];
        for (int c = 0; c < 3; c++) rec->evals[c] += a.ctr[c];
        rec->overflowed += a.ctr[K_OVF];
        rec->splits += a.ctr[K_SPLIT];
        for (int c = 0; c < K_NCTR; c++) a.ctr[c] = 0u;
    }
}

// ---------------------------------------------------------------- host
static int comm_grid(int64_t items_per_block_work, int max_blocks) {
    return (int) (items_per_block_work < 1 ? 1 : (items_per_block_work > max_blocks ? max_blocks : items_per_block_work));
}

extern "C" int gmx_communities(gmx_graph_t* g, int32_t max_rounds, gmx_node_t* comm_host, int32_t* rounds_out, int32_t* converged_out,
                               gmx_stats_t* stats_out) {
    GMX_REQUIRE(g && comm_host, "NULL argument");
    GMX_REQUIRE(max_rounds >= 0, "max_rounds = %d is negative", (int) max_rounds);
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    if (rounds_out) *rounds_out = 0;
    if (converged_out) *converged_out = 1;
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    if (g->E == 0) {   // nobody has neighbours: the identity is the fixpoint
        for (int64_t v = 0; v < V; v++) comm_host[v] = (gmx_node_t) v;
        return GMX_OK;
    }
    // thresholds, read at every call: rows of fewer than WAVE_MIN slots are short, of BLOCK_MIN or more hubs
    const int32_t wave_min = (int32_t) gmx_env_int("GMX_COMM_WAVE_MIN", COMM_WAVE_MIN, 1, INT32_MAX);
    const int32_t block_min = (int32_t) gmx_env_int("GMX_COMM_BLOCK_MIN", COMM_BLOCK_MIN, 1, INT32_MAX);
    int32_t cap = COMM_LDS_SLOTS_MIN;   // the power of two at or below the request
    const int64_t want = gmx_env_int("GMX_COMM_LDS_SLOTS", COMM_LDS_SLOTS, COMM_LDS_SLOTS_MIN, COMM_LDS_SLOTS_MAX);
    while ((int64_t) cap * 2 <= want) cap *= 2;
    const int32_t wcap = cap / COMM_WAVE_SHARE;
    const bool worklist = g->has_reverse && gmx_env_int("GMX_COMM_WORKLIST", 1, 0, 1) != 0;
    const bool round_log = getenv("GMX_COMM_ROUNDS") != nullptr;   // per-round line for tools/comm_prof.py
    const size_t wave_lds = (size_t) (COMM_THREADS / 64) * (2 * (size_t) wcap + 2 * COMM_STAGE + 4) * sizeof(int32_t);
    const size_t block_lds = 2 * (size_t) cap * sizeof(int32_t);
    GMX_HIP(hipFuncSetAttribute((const void*) comm_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) wave_lds));
    GMX_HIP(hipFuncSetAttribute((const void*) comm_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) block_lds));
    GMX_HIP(hipFuncSetAttribute((const void*) comm_overflow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) block_lds));

    gmx_ws_scope scope;
    const int64_t nwords = (V + 63) >> 6;
    wbuf<int32_t> comm, l0, l1, l2, ovf, ovf_own, pend_v, pend_l, big;
    wbuf<unsigned long long> dirty, ovf_best, shard;
    wbuf<unsigned int> ctr;
    wbuf<comm_rec> rec;
    GMX_CHECK(comm.alloc(V));
    GMX_CHECK(l0.alloc(V));
    GMX_CHECK(l1.alloc(V));
    GMX_CHECK(l2.alloc(V));
    GMX_CHECK(ovf.alloc(V));
    GMX_CHECK(ovf_own.alloc(V));
    GMX_CHECK(pend_v.alloc(V));
    GMX_CHECK(pend_l.alloc(V));
    GMX_CHECK(big.alloc(V));
    GMX_CHECK(dirty.alloc(nwords));
    GMX_CHECK(ovf_best.alloc(V));
    GMX_CHECK(shard.alloc(COMM_SHARDS));
    GMX_CHECK(ctr.alloc(K_NCTR));
    GMX_CHECK(rec.alloc(1));
    comm_arrays A{};
    A.beg = g->begin.p;
    A.idx = g->node_idx.p;
    A.rbeg = worklist ? g->r_begin.p : nullptr;
    A.ridx = worklist ? g->r_node_idx.p : nullptr;
    A.comm = comm.p;
    A.dirty = dirty.p;
    A.list[0] = l0.p;
    A.list[1] = l1.p;
    A.list[2] = l2.p;
    A.ovf = ovf.p;
    A.ovf_best = ovf_best.p;
    A.ovf_own = ovf_own.p;
    A.pend_v = pend_v.p;
    A.pend_l = pend_l.p;
    A.big = big.p;
    A.ctr = ctr.p;
    A.shard = shard.p;
    A.V = V;
    gmx_pinned<comm_rec> h_rec;
    GMX_CHECK(h_rec.alloc());
    gmx_spans tm;
    gmx_phase_clock round_clock;   // GMX_COMM_ROUNDS: a round's two half-rounds
    GMX_CHECK(round_clock.enable(round_log));

    const int word_grid = comm_grid((nwords + COMM_THREADS / 64 - 1) / (COMM_THREADS / 64), 2048);
    const int compact_grid = comm_grid((nwords + COMM_COMPACT_THREADS / 64 - 1) / (COMM_COMPACT_THREADS / 64), 1024);
    const int row_grid = comm_grid((V + 15) / 16, 2048);    // short: 16 rows per workgroup
    const int wave_grid = comm_grid((V + 3) / 4, 1280);     // a wave per row
    const int block_grid = comm_grid(V, 1024);              // a workgroup per row / per label class
    const int list_grid = comm_grid((V + COMM_THREADS - 1) / COMM_THREADS, 2048);
    // one half-round (half < 0: both halves at once) on the default stream; nothing here waits for the device
    auto half_round = [&](uint32_t salt, int half, bool commit, comm_rec* into) -> int {
        hipLaunchKernelGGL(comm_compact_kernel, dim3(compact_grid), dim3(COMM_COMPACT_THREADS), 0, 0, A, salt, half, wave_min, block_min, commit ? 1 : 0);
        hipLaunchKernelGGL(comm_short_kernel, dim3(row_grid), dim3(COMM_THREADS), 0, 0, A);
        hipLaunchKernelGGL(comm_wave_kernel, dim3(wave_grid), dim3(COMM_THREADS), wave_lds, 0, A, wcap);
        hipLaunchKernelGGL(comm_block_kernel, dim3(block_grid), dim3(COMM_THREADS), block_lds, 0, A, cap);
        hipLaunchKernelGGL(comm_overflow_kernel, dim3(block_grid), dim3(COMM_THREADS), block_lds, 0, A, cap);
        hipLaunchKernelGGL(comm_final_kernel, dim3(list_grid), dim3(COMM_THREADS), 0, 0, A);
        if (commit) hipLaunchKernelGGL(comm_commit_kernel, dim3(list_grid), dim3(COMM_THREADS), 0, 0, A);
        if (commit && worklist) hipLaunchKernelGGL(comm_commit_big_kernel, dim3(block_grid), dim3(COMM_THREADS), 0, 0, A);
        hipLaunchKernelGGL(comm_close_kernel, dim3(1), dim3(64), 0, 0, A, into);
        GMX_HIP(hipGetLastError());
        return GMX_OK;
    };
    auto read_rec = [&]() -> int {   // synchronises
        GMX_HIP(hipMemcpyAsync(h_rec.p, rec.p, sizeof(comm_rec), hipMemcpyDeviceToHost, 0));
        GMX_HIP(hipStreamSynchronize(0));
        return GMX_OK;
    };

    GMX_HIP(hipMemsetAsync(ctr.p, 0, sizeof(unsigned int) * K_NCTR, 0));
    GMX_HIP(hipMemsetAsync(shard.p, 0, sizeof(unsigned long long) * COMM_SHARDS, 0));
    GMX_CHECK(tm.begin(tm.KERNEL));
    hipLaunchKernelGGL(comm_init_kernel, dim3(word_grid), dim3(COMM_THREADS), 0, 0, A, 1);
    int32_t rounds = 0;
    int64_t evals = 0, slots = 0;
    bool fixpoint = false;   // known: a round changed nothing
    for (int32_t r = 0; r < max_rounds && !fixpoint; r++) {
        round_clock.begin();
        if (!worklist && r > 0) hipLaunchKernelGGL(comm_init_kernel, dim3(word_grid), dim3(COMM_THREADS), 0, 0, A, 0);
        GMX_HIP(hipMemsetAsync(rec.p, 0, sizeof(comm_rec), 0));
        const uint32_t salt = (uint32_t) r * 0x9E3779B9u;
        GMX_CHECK(half_round(salt, 0, true, rec.p));
        GMX_CHECK(half_round(salt, 1, true, rec.p));
        const float round_ms = round_clock.end();
        GMX_CHECK(read_rec());
        const comm_rec& R = *h_rec.p;
        evals += (int64_t) R.evals[0] + R.evals[1] + R.evals[2];
        slots += (int64_t) R.slots;
        if (round_log)
            fprintf(stderr, "gmx communities round %d: evals %u short + %u wave + %u block (%u overflowed), slots %llu, changes %u, %.3f ms, splits %u\n",
                    (int) r, R.evals[0], R.evals[1], R.evals[2], R.overflowed, R.slots, R.changes, round_ms, R.splits);
        if (R.changes == 0) fixpoint = true;
        else rounds++;
    }
    if (!fixpoint) {   // cut by max_rounds: one evaluation pass over what is still dirty that writes nothing
        if (!worklist && max_rounds > 0) hipLaunchKernelGGL(comm_init_kernel, dim3(word_grid), dim3(COMM_THREADS), 0, 0, A, 0);
        GMX_HIP(hipMemsetAsync(rec.p, 0, sizeof(comm_rec), 0));
        GMX_CHECK(half_round(0u, -1, false, rec.p));
        GMX_CHECK(read_rec());
        fixpoint = h_rec.p->changes == 0;
    }
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(comm_host, comm.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));
    if (rounds_out) *rounds_out = rounds;
    if (converged_out) *converged_out = fixpoint ? 1 : 0;
    stats->iterations = rounds;
    stats->vertices_reached = evals;
    stats->edges_examined = slots;
    return GMX_OK;
}

void gmx_touch_comm() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) comm_init_kernel);
}
