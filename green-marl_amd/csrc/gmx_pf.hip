// gmx_pf.hip -- potential-friend sets: potential_friends(G, potFriend) of apps/src/potential_friends.gm, on gfx950.
//
//   PF(v) = ( union of row(u) over the slots u of row(v) )  minus  row(v)  minus  {v}
//
// as a CSR over the vertices v_lo <= v < v_hi, every set ascending and distinct (gmx.h).  Sets and integers only: the
// result is a function of the graph, whatever the schedule.  Rows are read in any order, with repeats.
//
// A call is a chain of launches on the default stream:
//   len       L(v) = sum of outdeg(u) over the slots u of row(v) (64-bit): the two-hop items of the row
//   compact   rows with L > 0 -> three lists by L (wave / block / bitmap); rows and items per list in sharded counters
//   evaluate  longest regime first, in COUNT mode (the set sizes) or in FILL mode (the sets, at exact offsets):
//     bitmap  one workgroup per row, a V-bit map in LDS (V <= GMX_PF_LDS_BITS) or in global memory (one map per workgroup
//             of the persistent grid): atomic OR per item, the bits of row(v) and v cleared, then ONE pass over the words
//             that counts (or scans and writes the ascending list) and zeroes them for the workgroup's next row
//     block   one workgroup per row, an open-addressing table of keys in LDS, seeded with row(v) and v as BLOCKED keys
//             (bit 31 set), so that membership in row(v) needs no sorted row; the surviving keys are compacted and
//             sorted in LDS (bitonic)
//     wave    the same with one wave per row and a table of LDS_SLOTS / PF_WAVE_SHARE slots
//     overflow  rows whose table filled (PF_PROBES) are listed and evaluated by the bitmap kernel: never a partial set.
//             Whether a table fills may depend on the insertion order, so the COUNT and the FILL pass each keep their own
//             overflow list; the set a row gets is the same on either path.
// Counts before fill: the sizing call runs len + compact + COUNT.  The filling call runs that, forms the prefix sums on
// the host (they are the caller's pf_begin), and then, for every batch of consecutive vertices whose lists fit the staging
// buffer (GMX_PF_BATCH_BYTES), compact + FILL + one download.
#include "gmx_internal.h"

#define PF_THREADS 256
#define PF_WAVES (PF_THREADS / 64)
#define PF_EMPTY (-1)
#define PF_BLOCKED 0x80000000u     // a key of row(v) or v itself: present, never emitted
#define PF_KEYMASK 0x7FFFFFFF
#define PF_PROBES 64               // linear probes after which a table counts as full
#define PF_SHARDS 32               // per-regime item counters (adds to one word retire at ~90 per microsecond)
#define PF_WAVE_SHARE 8            // a wave's table holds LDS_SLOTS / PF_WAVE_SHARE slots
#define PF_WAVE_MAX 128            // defaults of GMX_PF_WAVE_MAX, GMX_PF_BLOCK_MAX, GMX_PF_LDS_SLOTS, GMX_PF_LDS_BITS
#define PF_BLOCK_MAX 2048
#define PF_LDS_SLOTS 4096
#define PF_LDS_SLOTS_MIN 512
#define PF_LDS_SLOTS_MAX 16384
#define PF_LDS_BITS (1 << 20)      // 128 KiB of the CU's 160 KiB
#define PF_LDS_BITS_MAX (1 << 20)
#define PF_BATCH_BYTES (256ll << 20)
#define PF_GLOBAL_GRID 256         // workgroups (and bitmaps) of the global-bitmap grid

enum { P_WAVE, P_BLOCK, P_BITMAP, P_OVF, P_NCTR };

struct pf_arrays {
    const int32_t* beg;
    const int32_t* idx;
    int64_t V;
    int64_t v_lo;
    int64_t* len;                    // [n] L of row v_lo + i
    int64_t* cnt;                    // [n] |PF(v_lo + i)|
    const int64_t* off;              // [n + 1] prefix sums of cnt (FILL)
    int32_t* list[3];                // [n] each: positions i in the range
    int32_t* ovf;                    // [n]
    unsigned int* ctr;               // [P_NCTR]
    unsigned long long* shard;       // [3][PF_SHARDS] items of the listed rows
    int32_t* out;                    // staging of the running batch (FILL)
    int64_t out_base;                // off[first row of the batch]
};

__device__ __forceinline__ uint32_t pf_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
// LDS written by other lanes of this wave is read after this (a wave's LDS operations execute in order)
__device__ __forceinline__ void pf_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
template <int NT>
__device__ __forceinline__ void pf_group_sync() {
    if (NT == 64) pf_wave_sync();
    else __syncthreads();
}

// ---------------------------------------------------------------- prepare
// L of the rows [0, n) of the range: one wave per row
__global__ void __launch_bounds__(PF_THREADS) pf_len_kernel(pf_arrays a, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t i = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nwaves) {
        const int64_t v = a.v_lo + i;
        const int32_t b = a.beg[v], e = a.beg[v + 1];
        long long s = 0;
        for (int32_t j = b + lane; j < e; j += 64) {
            const int32_t u = a.idx[j];
            s += a.beg[u + 1] - a.beg[u];
        }
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) a.len[i] = s;
    }
}

// rows [i0, i1) with L > 0 -> list[class by L]; list space is claimed once per wave and class
__global__ void __launch_bounds__(PF_THREADS) pf_compact_kernel(pf_arrays a, int64_t i0, int64_t i1, int64_t wave_max, int64_t block_max, int zero_cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    long long items[3] = {0, 0, 0};
    for (int64_t base = i0 + (((int64_t) blockIdx.x * blockDim.x + threadIdx.x) & ~63ll); base < i1; base += stride) {
        const int64_t i = base + lane;
        const long long L = i < i1 ? a.len[i] : 0;
        const bool sel = L > 0;
        if (zero_cnt && i < i1 && !sel) a.cnt[i] = 0;
        const int cls = L > block_max ? P_BITMAP : (L > wave_max ? P_BLOCK : P_WAVE);
        for (int c = 0; c < 3; c++) {
            const unsigned long long mc = __ballot(sel && cls == c);
            if (!mc) continue;
            unsigned int at = 0;
            if (lane == 0) at = atomicAdd(&a.ctr[c], (unsigned int) __builtin_popcountll(mc));
            at = __shfl(at, 0, 64);
            if (sel && cls == c) {
                a.list[c][at + __builtin_popcountll(mc & ((1ull << lane) - 1ull))] = (int32_t) i;
                items[c] += L;
            }
        }
    }
    const int64_t wave = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    for (int c = 0; c < 3; c++) {
        long long s = items[c];
        for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0 && s) atomicAdd(&a.shard[c * PF_SHARDS + (wave & (PF_SHARDS - 1))], (unsigned long long) s);
    }
}

// ---------------------------------------------------------------- table rows: NT = 64 (a wave) or PF_THREADS (the workgroup)
// key w (stored as `store`: w, or w | PF_BLOCKED) into keys[mask + 1]; false: no slot within `limit` probes
__device__ __forceinline__ bool pf_insert(int32_t* keys, uint32_t mask, int limit, int32_t w, int32_t store) {
    volatile int32_t* vkeys = keys;
    uint32_t s = pf_fmix32((uint32_t) w) & mask;
    for (int i = 0; i < limit; i++) {
        const int32_t k = vkeys[s];
        if ((k & PF_KEYMASK) == w) return true;   // (PF_EMPTY & PF_KEYMASK is no vertex id)
        if (k == PF_EMPTY) {
            const int32_t old = atomicCAS(&keys[s], PF_EMPTY, store);
            if (old == PF_EMPTY || (old & PF_KEYMASK) == w) return true;
        }
        s = (s + 1u) & mask;
    }
    return false;
}
// the part of a table a row with m keys at most uses: at least two slots per key (clearing and scanning the rest is wasted)
__device__ __forceinline__ int32_t pf_table_for(long long m, int32_t cap) {
    while (cap > 64 && cap / 4 >= m) cap >>= 1;
    return cap;
}

// Row i of the range by NT threads.  keys[cap], sorted[cap] and *s_flag / *s_n are the group's LDS.  COUNT: a.cnt[i] is
// written; FILL: the ascending set goes to a.out.  true (in every thread): the table filled and nothing was written.
template <int NT>
__device__ bool pf_table_row(const pf_arrays& a, int64_t i, int32_t* keys, int32_t* sorted, int32_t cap, int tid, int* s_flag, int* s_n, bool fill) {
    const int lane = threadIdx.x & 63;
    const int32_t v = (int32_t) (a.v_lo + i);
    const int32_t b = a.beg[v], e = a.beg[v + 1];
    cap = pf_table_for(a.len[i] + (e - b) + 1, cap);
    const uint32_t mask = (uint32_t) cap - 1u;
    const int limit = cap < PF_PROBES ? cap : PF_PROBES;
    volatile int* vflag = s_flag;
    for (int32_t s = tid; s < cap; s += NT) keys[s] = PF_EMPTY;
    if (tid == 0) {
        *s_flag = 0;
        *s_n = 0;
    }
    pf_group_sync<NT>();
    // the blocked keys
    if (tid == 0) pf_insert(keys, mask, limit, v, (int32_t) ((uint32_t) v | PF_BLOCKED));
    for (int32_t j = b + tid; j < e; j += NT) {
        if (*vflag) break;
        const int32_t u = a.idx[j];
        if (!pf_insert(keys, mask, limit, u, (int32_t) ((uint32_t) u | PF_BLOCKED))) *vflag = 1;
    }
    pf_group_sync<NT>();
    const bool seeds_full = *vflag != 0;
    pf_group_sync<NT>();   // (everybody has read the flag before the next phase, or the next row, writes it)
    if (seeds_full) return true;
    // the two-hop items: a wave per slot of row(v), its lanes over row(u)
    const int wstep = NT / 64, wfirst = NT == 64 ? 0 : (int) (threadIdx.x >> 6);
    for (int32_t j0 = b; j0 < e; j0 += 64) {
        if (*vflag) break;   // somebody found no slot: the row is void anyway
        const int32_t u = j0 + lane < e ? a.idx[j0 + lane] : 0;
        const int32_t ub = a.beg[u], ue = j0 + lane < e ? a.beg[u + 1] : ub;
        const int m = e - j0 < 64 ? e - j0 : 64;
        for (int k = wfirst; k < m; k += wstep) {
            const int32_t rb = __shfl(ub, k, 64), re = __shfl(ue, k, 64);
            for (int32_t t = rb + lane; t < re; t += 64) {
                const int32_t w = a.idx[t];
                if (!pf_insert(keys, mask, limit, w, w)) *vflag = 1;
            }
        }
    }
    pf_group_sync<NT>();
    const bool full = *vflag != 0;
    pf_group_sync<NT>();
    if (full) return true;
    if (!fill) {
        int c = 0;
        for (int32_t s = tid; s < cap; s += NT) c += keys[s] >= 0;
        for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0 && c) atomicAdd(s_n, c);
        pf_group_sync<NT>();
        if (tid == 0) a.cnt[i] = *s_n;
        pf_group_sync<NT>();
        return false;
    }
    // survivors -> sorted[], padded to a power of two, bitonic sort, out
    for (int32_t s = tid; s < cap; s += NT) {
        const int32_t k = keys[s];
        if (k >= 0) sorted[atomicAdd(s_n, 1)] = k;
    }
    pf_group_sync<NT>();
    const int32_t n = *s_n;
    int32_t m = 2;
    while (m < n) m <<= 1;   // (n <= cap, both powers of two bound m <= cap)
    for (int32_t s = n + tid; s < m; s += NT) sorted[s] = INT32_MAX;
    pf_group_sync<NT>();
    for (int32_t k = 2; k <= m; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t t = tid; t < m; t += NT) {
                const int32_t x = t ^ j;
                if (x > t) {
                    const int32_t p = sorted[t], q = sorted[x];
                    if ((p > q) == ((t & k) == 0)) {
                        sorted[t] = q;
                        sorted[x] = p;
                    }
                }
            }
            pf_group_sync<NT>();
        }
    const int64_t o = a.off[i] - a.out_base;
    const int64_t room = a.off[i + 1] - a.off[i];   // (= n: the COUNT pass found the same set)
    for (int32_t t = tid; t < n && t < room; t += NT) a.out[o + t] = sorted[t];
    pf_group_sync<NT>();
    return false;
}

// (one thread) row i's table filled: to the overflow list
__device__ __forceinline__ void pf_overflow(const pf_arrays& a, int64_t i) { a.ovf[atomicAdd(&a.ctr[P_OVF], 1u)] = (int32_t) i; }

// one wave per row; dynamic LDS per wave: keys[cap], sorted[cap], flag, n
__global__ void __launch_bounds__(PF_THREADS) pf_wave_kernel(pf_arrays a, int64_t n, int32_t cap, int fill) {
    extern __shared__ int32_t pf_lds[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int32_t* mine = pf_lds + (size_t) wid * (2 * cap + 2);
    const int32_t* __restrict__ list = a.list[P_WAVE];
    const int64_t nwaves = ((int64_t) gridDim.x * blockDim.x) >> 6;
    for (int64_t k = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6; k < n; k += nwaves) {
        const int64_t i = list[k];
        if (pf_table_row<64>(a, i, mine, mine + cap, cap, lane, mine + 2 * cap, mine + 2 * cap + 1, fill != 0) && lane == 0) pf_overflow(a, i);
    }
}
// one workgroup per row; dynamic LDS: keys[cap], sorted[cap]
__global__ void __launch_bounds__(PF_THREADS) pf_block_kernel(pf_arrays a, int64_t n, int32_t cap, int fill) {
    extern __shared__ int32_t pf_lds[];
    __shared__ int s_flag, s_n;
    const int32_t* __restrict__ list = a.list[P_BLOCK];
    for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int64_t i = list[k];
        if (pf_table_row<PF_THREADS>(a, i, pf_lds, pf_lds + cap, cap, threadIdx.x, &s_flag, &s_n, fill != 0) && threadIdx.x == 0) pf_overflow(a, i);
    }
}

// ---------------------------------------------------------------- bitmap rows
// A word of a global map is only ever touched by device-scope operations (atomic OR / AND, these loads and stores): the
// CU's vector cache, which atomics bypass, never holds a copy that a later plain load could find stale.
template <bool LDS>
__device__ __forceinline__ uint32_t pf_word_load(uint32_t* p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void pf_word_zero(uint32_t* p) {
    if (LDS) *p = 0u;
    else __hip_atomic_store(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// One workgroup per listed row.  LDS = true: the map is the dynamic LDS; false: gmaps + blockIdx.x * nwords (zeroed by the
// host before the launch).  Either way the map is all zero between two rows: the pass that reads the words zeroes them.
template <bool LDS>
__global__ void __launch_bounds__(PF_THREADS) pf_bitmap_kernel(pf_arrays a, const int32_t* __restrict__ list, int64_t n, uint32_t* gmaps, int fill) {
    extern __shared__ int32_t pf_lds[];
    __shared__ long long s_part[PF_WAVES];
    __shared__ int s_wsum[PF_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t nwords = (a.V + 31) >> 5;
    const uint32_t tail = (a.V & 31) ? ((1u << (a.V & 31)) - 1u) : 0xFFFFFFFFu;   // the bits of the last word that are vertices
    uint32_t* bm;
    if (LDS) {
        bm = (uint32_t*) pf_lds;
        for (int64_t w = threadIdx.x; w < nwords; w += PF_THREADS) bm[w] = 0u;
    } else {
        bm = gmaps + (size_t) blockIdx.x * (size_t) nwords;
    }
    __syncthreads();
    for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const int64_t i = list[k];
        const int32_t v = (int32_t) (a.v_lo + i);
        const int32_t b = a.beg[v], e = a.beg[v + 1];
        // set: a wave per slot of row(v), its lanes over row(u)
        for (int32_t j0 = b; j0 < e; j0 += 64) {
            const int32_t u = j0 + lane < e ? a.idx[j0 + lane] : 0;
            const int32_t ub = a.beg[u], ue = j0 + lane < e ? a.beg[u + 1] : ub;
            const int m = e - j0 < 64 ? e - j0 : 64;
            for (int q = wid; q < m; q += PF_WAVES) {
                const int32_t rb = __shfl(ub, q, 64), re = __shfl(ue, q, 64);
                for (int32_t t = rb + lane; t < re; t += 64) {
                    const int32_t w = a.idx[t];
                    const uint32_t bit = 1u << (w & 31);
                    if (LDS || !(pf_word_load<false>(&bm[w >> 5]) & bit)) atomicOr(&bm[w >> 5], bit);
                }
            }
        }
        __syncthreads();
        // clear row(v) and v
        if (threadIdx.x == 0) atomicAnd(&bm[v >> 5], ~(1u << (v & 31)));
        for (int32_t j = b + (int32_t) threadIdx.x; j < e; j += PF_THREADS) {
            const int32_t u = a.idx[j];
            atomicAnd(&bm[u >> 5], ~(1u << (u & 31)));
        }
        __syncthreads();
        if (!fill) {
            long long c = 0;
            for (int64_t w = threadIdx.x; w < nwords; w += PF_THREADS) {
                uint32_t x = pf_word_load<LDS>(&bm[w]);
                if (x) pf_word_zero<LDS>(&bm[w]);
                if (w == nwords - 1) x &= tail;
                c += __builtin_popcount(x);
            }
            for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0) s_part[wid] = c;
            __syncthreads();
            if (threadIdx.x == 0) {
                long long s = 0;
                for (int q = 0; q < PF_WAVES; q++) s += s_part[q];
                a.cnt[i] = s;
            }
            __syncthreads();
            continue;
        }
        // ascending fill: PF_THREADS words per step, exclusive scan of their popcounts
        const int64_t o = a.off[i] - a.out_base, room = a.off[i + 1] - a.off[i];
        int64_t run = 0;
        for (int64_t w0 = 0; w0 < nwords; w0 += PF_THREADS) {
            const int64_t w = w0 + threadIdx.x;
            uint32_t x = 0u;
            if (w < nwords) {
                x = pf_word_load<LDS>(&bm[w]);
                if (x) pf_word_zero<LDS>(&bm[w]);
                if (w == nwords - 1) x &= tail;
            }
            const int c = __builtin_popcount(x);
            int inc = c;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(inc, d, 64);
                if (lane >= d) inc += y;
            }
            if (lane == 63) s_wsum[wid] = inc;
            __syncthreads();
            int before = 0, total = 0;
            for (int q = 0; q < PF_WAVES; q++) {
                if (q < wid) before += s_wsum[q];
                total += s_wsum[q];
            }
            int64_t pos = run + before + inc - c;
            while (x) {
                const int bit = __builtin_ctz(x);
                x &= x - 1u;
                if (pos < room) a.out[o + pos] = (int32_t) (w * 32 + bit);
                pos++;
            }
            run += total;
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- host
static int pf_grid(int64_t want, int max_blocks) { return (int) (want < 1 ? 1 : (want > max_blocks ? max_blocks : want)); }

struct pf_plan {
    int64_t wave_max, block_max, lds_bits, batch_bytes;
    int32_t cap, wcap;
    size_t wave_lds, block_lds, bitmap_lds;
    bool lds_map;
    uint32_t* gmaps;
    int global_grid;
    bool log;
};
struct pf_regimes {   // of one compact + evaluate
    unsigned int rows[P_NCTR];
    unsigned long long items[3];
};

// compact rows [i0, i1) and evaluate them (fill = 0: COUNT, 1: FILL into A.out); synchronises twice (list lengths)
static int pf_evaluate(pf_arrays& A, const pf_plan& P, int64_t i0, int64_t i1, int fill, unsigned int* d_ctr_host, unsigned long long* d_shard_host,
                       pf_regimes* reg) {
    const int64_t n = i1 - i0;
    GMX_HIP(hipMemsetAsync(A.ctr, 0, sizeof(unsigned int) * P_NCTR, 0));
    GMX_HIP(hipMemsetAsync(A.shard, 0, sizeof(unsigned long long) * 3 * PF_SHARDS, 0));
    hipLaunchKernelGGL(pf_compact_kernel, dim3(pf_grid((n + PF_THREADS - 1) / PF_THREADS, 2048)), dim3(PF_THREADS), 0, 0, A, i0, i1, P.wave_max,
                       P.block_max, fill ? 0 : 1);
    GMX_HIP(hipGetLastError());
    GMX_HIP(hipMemcpyAsync(d_ctr_host, A.ctr, sizeof(unsigned int) * P_NCTR, hipMemcpyDeviceToHost, 0));
    GMX_HIP(hipMemcpyAsync(d_shard_host, A.shard, sizeof(unsigned long long) * 3 * PF_SHARDS, hipMemcpyDeviceToHost, 0));
    GMX_HIP(hipStreamSynchronize(0));
    const int64_t nw = d_ctr_host[P_WAVE], nb = d_ctr_host[P_BLOCK], nm = d_ctr_host[P_BITMAP];
    for (int c = 0; c < 3; c++) {
        reg->rows[c] = d_ctr_host[c];
        reg->items[c] = 0;
        for (int s = 0; s < PF_SHARDS; s++) reg->items[c] += d_shard_host[c * PF_SHARDS + s];
    }
    auto bitmap = [&](const int32_t* list, int64_t rows) -> int {
        if (rows == 0) return GMX_OK;
        if (P.lds_map) {
            const int per_cu = (int) (163840 / (P.bitmap_lds + 256));
            hipLaunchKernelGGL(pf_bitmap_kernel<true>, dim3(pf_grid(rows, 256 * (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu)))), dim3(PF_THREADS), P.bitmap_lds, 0,
                               A, list, rows, (uint32_t*) nullptr, fill);
        } else {
            hipLaunchKernelGGL(pf_bitmap_kernel<false>, dim3(pf_grid(rows, P.global_grid)), dim3(PF_THREADS), 0, 0, A, list, rows, P.gmaps, fill);
        }
        GMX_HIP(hipGetLastError());
        return GMX_OK;
    };
    GMX_CHECK(bitmap(A.list[P_BITMAP], nm));
    if (nb) hipLaunchKernelGGL(pf_block_kernel, dim3(pf_grid(nb, 2048)), dim3(PF_THREADS), P.block_lds, 0, A, nb, P.cap, fill);
    if (nw) hipLaunchKernelGGL(pf_wave_kernel, dim3(pf_grid((nw + PF_WAVES - 1) / PF_WAVES, 2048)), dim3(PF_THREADS), P.wave_lds, 0, A, nw, P.wcap, fill);
    GMX_HIP(hipGetLastError());
    reg->rows[P_OVF] = 0;
    if (nb || nw) {
        GMX_HIP(hipMemcpyAsync(d_ctr_host, A.ctr, sizeof(unsigned int) * P_NCTR, hipMemcpyDeviceToHost, 0));
        GMX_HIP(hipStreamSynchronize(0));
        reg->rows[P_OVF] = d_ctr_host[P_OVF];
        GMX_CHECK(bitmap(A.ovf, d_ctr_host[P_OVF]));
    }
    if (P.log)
        fprintf(stderr, "gmx potential_friends %s rows [%lld, %lld): rows %u wave + %u block + %u bitmap (%u overflowed), items %llu wave + %llu block + %llu bitmap\n",
                fill ? "fill" : "count", (long long) i0, (long long) i1, reg->rows[P_WAVE], reg->rows[P_BLOCK], reg->rows[P_BITMAP], reg->rows[P_OVF],
                reg->items[P_WAVE], reg->items[P_BLOCK], reg->items[P_BITMAP]);
    return GMX_OK;
}

extern "C" int gmx_potential_friends(gmx_graph_t* g, gmx_node_t v_lo, gmx_node_t v_hi, int64_t* pf_begin_host, gmx_node_t* pf_idx_host, int64_t cap,
                                     int64_t* total_out, gmx_stats_t* stats_out) {
    GMX_REQUIRE(g && pf_begin_host, "NULL argument");
    GMX_REQUIRE(v_lo >= 0 && v_lo <= v_hi && (int64_t) v_hi <= g->V, "vertex range [%d, %d) outside [0, %lld]", (int) v_lo, (int) v_hi, (long long) g->V);
    GMX_REQUIRE(cap >= 0, "cap = %lld is negative", (long long) cap);
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V, n = (int64_t) v_hi - v_lo;
    for (int64_t i = 0; i <= n; i++) pf_begin_host[i] = 0;
    if (total_out) *total_out = 0;
    if (n == 0 || g->E == 0) return GMX_OK;

    // knobs, read at every call; the results do not depend on them
    pf_plan P{};
    P.wave_max = gmx_env_int("GMX_PF_WAVE_MAX", PF_WAVE_MAX, 0, INT64_MAX);
    P.block_max = gmx_env_int("GMX_PF_BLOCK_MAX", PF_BLOCK_MAX, 0, INT64_MAX);
    if (P.block_max < P.wave_max) P.block_max = P.wave_max;
    P.cap = PF_LDS_SLOTS_MIN;   // the power of two at or below the request
    const int64_t want = gmx_env_int("GMX_PF_LDS_SLOTS", PF_LDS_SLOTS, PF_LDS_SLOTS_MIN, PF_LDS_SLOTS_MAX);
    while ((int64_t) P.cap * 2 <= want) P.cap *= 2;
    P.wcap = P.cap / PF_WAVE_SHARE;
    P.lds_bits = gmx_env_int("GMX_PF_LDS_BITS", PF_LDS_BITS, 1, PF_LDS_BITS_MAX);
    P.batch_bytes = gmx_env_int("GMX_PF_BATCH_BYTES", PF_BATCH_BYTES, 4, INT64_MAX);
    P.log = getenv("GMX_PF_LOG") != nullptr;   // a line per evaluation for tools/pf_prof.py
    const int64_t nwords = (V + 31) >> 5;
    P.lds_map = V <= P.lds_bits;
    P.wave_lds = (size_t) PF_WAVES * (2 * (size_t) P.wcap + 2) * sizeof(int32_t);
    P.block_lds = 2 * (size_t) P.cap * sizeof(int32_t);
    P.bitmap_lds = (size_t) nwords * sizeof(uint32_t);
    GMX_HIP(hipFuncSetAttribute((const void*) pf_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) P.wave_lds));
    GMX_HIP(hipFuncSetAttribute((const void*) pf_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) P.block_lds));
    if (P.lds_map) GMX_HIP(hipFuncSetAttribute((const void*) pf_bitmap_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) P.bitmap_lds));

    gmx_ws_scope scope;
    wbuf<int64_t> len, cnt, off;
    wbuf<int32_t> l0, l1, l2, ovf, out;
    wbuf<unsigned int> ctr;
    wbuf<unsigned long long> shard;
    wbuf<uint32_t> gmaps;
    GMX_CHECK(len.alloc(n));
    GMX_CHECK(cnt.alloc(n));
    GMX_CHECK(l0.alloc(n));
    GMX_CHECK(l1.alloc(n));
    GMX_CHECK(l2.alloc(n));
    GMX_CHECK(ovf.alloc(n));
    GMX_CHECK(ctr.alloc(P_NCTR));
    GMX_CHECK(shard.alloc(3 * PF_SHARDS));
    if (!P.lds_map) {
        P.global_grid = pf_grid(n, PF_GLOBAL_GRID);
        GMX_CHECK(gmaps.alloc((size_t) P.global_grid * (size_t) nwords));
        GMX_HIP(hipMemsetAsync(gmaps.p, 0, (size_t) P.global_grid * (size_t) nwords * sizeof(uint32_t), 0));
        P.gmaps = gmaps.p;
    }
    pf_arrays A{};
    A.beg = g->begin.p;
    A.idx = g->node_idx.p;
    A.V = V;
    A.v_lo = v_lo;
    A.len = len.p;
    A.cnt = cnt.p;
    A.list[0] = l0.p;
    A.list[1] = l1.p;
    A.list[2] = l2.p;
    A.ovf = ovf.p;
    A.ctr = ctr.p;
    A.shard = shard.p;
    gmx_pinned<unsigned int> h_ctr;
    gmx_pinned<unsigned long long> h_shard;
    GMX_CHECK(h_ctr.alloc(P_NCTR));
    GMX_CHECK(h_shard.alloc(3 * PF_SHARDS));
    gmx_spans tm;   // the sizing pass, then a kernel + download lap per batch: each adds to its span's sum

    // counts
    pf_regimes reg;
    GMX_CHECK(tm.begin(tm.KERNEL));
    hipLaunchKernelGGL(pf_len_kernel, dim3(pf_grid((n + PF_WAVES - 1) / PF_WAVES, 4096)), dim3(PF_THREADS), 0, 0, A, n);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(pf_evaluate(A, P, 0, n, 0, h_ctr.p, h_shard.p, &reg));
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(pf_begin_host + 1, cnt.p, sizeof(int64_t) * (size_t) n, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));
    int64_t reached = 0;
    for (int64_t i = 0; i < n; i++) {
        reached += pf_begin_host[i + 1] > 0;
        pf_begin_host[i + 1] += pf_begin_host[i];
    }
    const int64_t total = pf_begin_host[n];
    if (total_out) *total_out = total;
    stats->edges_examined = (int64_t) (reg.items[0] + reg.items[1] + reg.items[2]);
    stats->vertices_reached = reached;
    if (!pf_idx_host || total > cap || total == 0) return GMX_OK;

    // fill, batch by batch over consecutive vertices; a row above the budget is a batch of its own
    const int64_t budget = P.batch_bytes / (int64_t) sizeof(int32_t) < 1 ? 1 : P.batch_bytes / (int64_t) sizeof(int32_t);
    int64_t staging = 0;
    for (int64_t i0 = 0; i0 < n;) {
        int64_t i1 = i0 + 1;
        while (i1 < n && pf_begin_host[i1 + 1] - pf_begin_host[i0] <= budget) i1++;
        if (pf_begin_host[i1] - pf_begin_host[i0] > staging) staging = pf_begin_host[i1] - pf_begin_host[i0];
        i0 = i1;
    }
    GMX_CHECK(off.alloc(n + 1));
    GMX_CHECK(out.alloc((size_t) staging));
    GMX_HIP(hipMemcpy(off.p, pf_begin_host, sizeof(int64_t) * (size_t) (n + 1), hipMemcpyHostToDevice));
    A.off = off.p;
    A.out = out.p;
    int32_t batches = 0;
    for (int64_t i0 = 0; i0 < n;) {
        int64_t i1 = i0 + 1;
        while (i1 < n && pf_begin_host[i1 + 1] - pf_begin_host[i0] <= budget) i1++;
        const int64_t items = pf_begin_host[i1] - pf_begin_host[i0];
        if (items > 0) {
            A.out_base = pf_begin_host[i0];
            GMX_CHECK(tm.begin(tm.KERNEL));
            GMX_CHECK(pf_evaluate(A, P, i0, i1, 1, h_ctr.p, h_shard.p, &reg));
            GMX_CHECK(tm.end(tm.KERNEL));
            GMX_CHECK(tm.begin(tm.D2H));
            GMX_HIP(hipMemcpy(pf_idx_host + pf_begin_host[i0], out.p, sizeof(int32_t) * (size_t) items, hipMemcpyDeviceToHost));
            GMX_CHECK(tm.end(tm.D2H));
            batches++;
        }
        i0 = i1;
    }
    stats->iterations = batches;
    return tm.finish(stats);
}

void gmx_touch_pf() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) pf_len_kernel);
}
