// gmx_bc_batch.hip -- comp_BC / bc_random with the sources as the fast axis (gmx_bc_batch, include/gmx.h).
//
// gmx_bc (gmx_bfs.hip) sweeps one seed at a time: per row slot an index load, a bitmap probe and a 4- or 8-byte gather for ONE
// seed.  Here W seeds (16, 32 or 64) share the sweeps: per vertex a row of W level bytes lvl[v][0..W) (0xFF = unreached) and a
// row of W float2 sd[v][0..W) (x = sigma, y = delta, as bc_visit_fw / bc_visit_rv keep them).  A lane owns one (row, column)
// sum, so one index load serves W seeds, a gather of lvl[w][.] or sd[w][.] is a fully used line, and the serial chain of float
// adds that the contract demands (every Sum in row-slot order) runs in W lanes side by side.
//
// Per batch: W traversals (the existing one, through gmx_bfs_reach) staged as bytes and transposed once -- or, with
// GMX_BCB_MSBFS and for gmx_bc_all (comp_BC of bc_adj.gm: every vertex a source; DESIGN.md 4.2g'), one bit-parallel
// multi-source traversal that writes the same bytes; then one forward pass
// per level from the roots (sigma) and one reverse pass per level from the deepest (delta), each a launch of its own -- every
// value a pass reads was written by an earlier launch, nothing is read and written in one launch -- and BC[v] += delta[v][b]
// for b ascending, which is the per-seed order of the emission.  A pass's rows come from a per-vertex (min, max) level pair
// and an exact look at the candidates' level rows; rows shorter than GMX_BCB_LONG_MIN slots are walked by a lane group each,
// the others by a workgroup each whose waves evaluate the terms into LDS for one wave to add in slot order.
#include "gmx_internal.h"
#include "gmx_frontier.h"

#include <limits.h>

#define BCB_UNREACHED 0xFFu
#define BCB_DEPTH_CAP 254       // deepest level a byte holds beside BCB_UNREACHED
#define BCB_MAX_PASSES (2 * (BCB_DEPTH_CAP + 1))
#define BCB_FIND_ITEMS 8        // vertices per thread of the row finder (one list append per workgroup and list)
#define BCB_SHORT_UNROLL 4      // slots of a short row in flight per lane
#define BCB_LONG_THREADS 1024   // long rows: wave 0 adds, the other 15 waves evaluate terms
#define BCB_LONG_PRODUCERS (BCB_LONG_THREADS / 64 - 1)
#define BCB_LONG_UNROLL 8       // 64-lane term rows in flight per producer wave
#define BCB_LONG_ROWS (BCB_LONG_PRODUCERS * BCB_LONG_UNROLL)   // 64-lane term rows of one LDS tile (two tiles: 60 KiB)

// ---------------------------------------------------------------- levels: dist[] -> stage[b][v] -> lvl[v][b]
// one traversal's dist[] as bytes, four vertices per thread; its depth and its reached count (one atomic each per workgroup)
__global__ void __launch_bounds__(BFS_THREADS)
bcb_stage_kernel(const int32_t* __restrict__ dist, int64_t V, uint32_t* __restrict__ stage_col, int32_t* __restrict__ depth, unsigned long long* __restrict__ reached) {
    __shared__ int32_t s_depth;
    __shared__ unsigned int s_reached;
    if (threadIdx.x == 0) { s_depth = 0; s_reached = 0; }
    __syncthreads();
    int32_t d_max = 0;
    unsigned int n = 0;
    const int64_t words = (V + 3) >> 2, stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t v = 4 * i + k;
            const int32_t d = v < V ? dist[v] : INT_MAX;
            uint32_t byte = BCB_UNREACHED;
            if (d != INT_MAX) {
                n++;
                d_max = d > d_max ? d : d_max;
                if (d <= BCB_DEPTH_CAP) byte = (uint32_t) d;   // (a deeper traversal sends its batch to the per-seed path)
            }
            out |= byte << (8 * k);
        }
        stage_col[i] = out;
    }
    atomicMax(&s_depth, d_max);
    atomicAdd(&s_reached, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax(depth, s_depth);
        atomicAdd(reached, (unsigned long long) s_reached);
    }
}

// stage[b][v] -> lvl[v][b] through an LDS tile of 256 vertices; columns from nb on (the last, partial batch) are unreached
// everywhere; minmax[v] = (deepest << 8 | shallowest) level of v over the columns (0x00FF: none)
template <int W>
__global__ void __launch_bounds__(256)
bcb_transpose_kernel(const uint32_t* __restrict__ stage, int64_t V, int64_t pitch_words, int32_t nb, uint32_t* __restrict__ lvl, uint16_t* __restrict__ minmax) {
    __shared__ uint32_t tile[W][65];   // [column][word of 4 vertices]
    const int t = threadIdx.x;
    const int64_t v0 = (int64_t) blockIdx.x * 256;
#pragma unroll
    for (int j = 0; j < W / 4; j++) {
        const int b = (t >> 6) + 4 * j;
        const int64_t word = (v0 >> 2) + (t & 63);
        tile[b][t & 63] = (b < nb && 4 * word < V) ? stage[(int64_t) b * pitch_words + word] : 0xFFFFFFFFu;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < W / 4; j++) {
        const int k = t + 256 * j;             // output word of the tile: vertex r, columns c .. c + 3
        const int r = (4 * k) / W, c = (4 * k) % W;
        uint32_t out = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) out |= ((tile[c + i][r >> 2] >> (8 * (r & 3))) & 0xFFu) << (8 * i);
        if (v0 + r < V) lvl[v0 * (W / 4) + k] = out;
    }
    if (v0 + t < V) {
        uint32_t mn = BCB_UNREACHED, mx = 0;
        for (int b = 0; b < nb; b++) {
            const uint32_t x = (tile[b][t >> 2] >> (8 * (t & 3))) & 0xFFu;
            if (x != BCB_UNREACHED) {
                mn = x < mn ? x : mn;
                mx = x > mx ? x : mx;
            }
        }
        minmax[v0 + t] = (uint16_t) (mx << 8 | mn);
    }
}

// ---------------------------------------------------------------- levels, all columns at once (GMX_BCB_MSBFS, gmx_bc_all)
// A bit-parallel multi-source traversal over the reverse CSR: per vertex one word of W bits in each of seen / front / next
// (bit b = column b; 64-bit words for W = 64, 32-bit ones below), carved out of the V * W bytes the staged levels take.
// A level is a pull: a vertex that still lacks a column ORs front[] over its reverse row, keeps the bits it has not seen,
// and writes only its own words, its own level bytes and its own minmax -- front[] of the others is written by no
// kernel of that level, so nothing is read and written in one launch and there is no atomic on the state.  The bytes are
// the staged path's because BFS levels are unique.  Rows shorter than GMX_BCB_MS_LONG_MIN slots are walked by their
// owner's lane (msb_level_kernel), the others are listed and walked by a wave each (msb_long_kernel); both stop once
// every missing column is covered.  Only the columns whose front is not empty can be found: a level ORs the words it
// writes into the next level's `active` word (one atomic per workgroup, read by the next launch), and a vertex that
// misses none of those skips its row -- a source that reaches little stops costing row walks once its front is empty.
template <int W> struct msb_word { typedef uint32_t type; };
template <> struct msb_word<64> { typedef uint64_t type; };

#define MSB_SHORT_UNROLL 4   // slots of a short row in flight per lane
#define MSB_LONG_UNROLL 4    // 64-slot pieces of a long row in flight per wave, then one cross-lane OR and the exit test
enum { MSB_ROWS_SHORT = 0, MSB_ROWS_LONG = 1, MSB_SLOTS = 2, MSB_SATURATED = 3, MSB_STATS = 4 };   // then found[level], then active[level]
#define MSB_ACTIVE (MSB_STATS + BCB_DEPTH_CAP + 2)   // active[l]: the columns with a vertex in level l's front (the OR of its words)
#define MSB_TALLY (MSB_ACTIVE + BCB_DEPTH_CAP + 3)

__device__ __forceinline__ int msb_popc(uint32_t x) { return __popc(x); }
__device__ __forceinline__ int msb_popc(uint64_t x) { return __popcll(x); }
__device__ __forceinline__ uint32_t msb_wave_or(uint32_t x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x |= (uint32_t) __shfl_xor((int) x, d, 64);
    return x;
}
__device__ __forceinline__ uint64_t msb_wave_or(uint64_t x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x |= (uint64_t) __shfl_xor((unsigned long long) x, d, 64);
    return x;
}

// a workgroup's counters into the batch's tally, and the columns it found into the next level's active word: one atomic
// per workgroup and non-zero value (s_t: MSB_STATS counters, the new pairs, the new columns)
__device__ __forceinline__ void msb_tally(unsigned long long* s_t, unsigned long long* __restrict__ tally, int32_t l, unsigned long long rows, int which,
                                          unsigned long long slots, unsigned long long sat, unsigned long long pairs, unsigned long long columns) {
    if (rows) atomicAdd(&s_t[which], rows);
    if (slots) atomicAdd(&s_t[MSB_SLOTS], slots);
    if (sat) atomicAdd(&s_t[MSB_SATURATED], sat);
    if (pairs) atomicAdd(&s_t[MSB_STATS], pairs);
    columns = msb_wave_or((uint64_t) columns);
    if ((threadIdx.x & 63) == 0 && columns) atomicOr(&s_t[MSB_STATS + 1], columns);
    __syncthreads();
    if (threadIdx.x <= MSB_STATS && s_t[threadIdx.x]) atomicAdd(&tally[threadIdx.x == MSB_STATS ? MSB_STATS + l : (int) threadIdx.x], s_t[threadIdx.x]);
    if (threadIdx.x == MSB_STATS + 1 && s_t[threadIdx.x]) atomicOr(&tally[MSB_ACTIVE + l + 1], s_t[threadIdx.x]);
}

// everything unreached; the mask words clear
template <int W>
__global__ void __launch_bounds__(BFS_THREADS)
msb_clear_kernel(int64_t V, typename msb_word<W>::type* __restrict__ seen, typename msb_word<W>::type* __restrict__ front, uint32_t* __restrict__ lvl, uint16_t* __restrict__ minmax) {
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < V * (W / 4); i += stride) lvl[i] = 0xFFFFFFFFu;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) {
        seen[v] = 0;
        front[v] = 0;
        minmax[v] = 0x00FFu;
    }
}

// level 0: one wave, lane b = column b.  Duplicate seeds are independent columns on one vertex: every lane of that vertex
// gathers all its columns' bits and the lanes store the same word
template <int W>
__global__ void __launch_bounds__(64)
msb_seed_kernel(const int32_t* __restrict__ seeds, int32_t nb, typename msb_word<W>::type* __restrict__ seen, typename msb_word<W>::type* __restrict__ front,
                uint8_t* __restrict__ lvl, uint16_t* __restrict__ minmax, unsigned long long* __restrict__ tally) {
    typedef typename msb_word<W>::type word;
    const int b = threadIdx.x;
    const int32_t mine = b < nb ? seeds[b] : -1;
    word m = 0;
    for (int j = 0; j < nb; j++) {   // (wave-uniform)
        const int32_t other = __shfl(mine, j, 64);
        if (other == mine) m |= (word) 1 << j;
    }
    if (b < nb) {
        seen[mine] = m;
        front[mine] = m;
        lvl[(int64_t) mine * W + b] = 0;
        minmax[mine] = 0;
    }
    if (b == 0) tally[MSB_ACTIVE + 1] = nb >= 64 ? ~0ull : (1ull << nb) - 1;   // every column has its root in level 1's front
}

// what a vertex does with the columns a level found for it (its own words and bytes only)
template <int W>
__device__ __forceinline__ void msb_settle(int64_t v, typename msb_word<W>::type s, typename msb_word<W>::type nw, int32_t l, bool store,
                                           typename msb_word<W>::type* __restrict__ seen, uint16_t* __restrict__ minmax) {
    if (!nw) return;
    seen[v] = s | nw;
    if (store) {
        const uint32_t mn = minmax[v] & 0xFFu;   // levels ascend: the first one found is the shallowest
        minmax[v] = (uint16_t) ((uint32_t) l << 8 | (mn == BCB_UNREACHED ? (uint32_t) l : mn));
    }
}

// level l, every vertex: saturated ones (no column missing whose front is not empty: the others can find nothing) only clear
// their next word; rows of at least long_min slots go to long_list (one append per wave); the others are walked here.  store = 0 is the probe of the level past the depth
// cap: it says whether that level is empty and stores no level byte
template <int W>
__global__ void __launch_bounds__(BFS_THREADS)
msb_level_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, typename msb_word<W>::type live, int32_t l, int32_t long_min, int store,
                 typename msb_word<W>::type* __restrict__ seen, const typename msb_word<W>::type* __restrict__ front, typename msb_word<W>::type* __restrict__ next,
                 uint8_t* __restrict__ lvl, uint16_t* __restrict__ minmax, int32_t* __restrict__ long_list, unsigned int* __restrict__ long_count,
                 unsigned long long* __restrict__ tally) {
    typedef typename msb_word<W>::type word;
    __shared__ unsigned long long s_t[MSB_STATS + 2];
    if (threadIdx.x <= MSB_STATS + 1) s_t[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long rows = 0, slots = 0, sat = 0, pairs = 0;
    word columns = 0;
    const word active = live & (word) tally[MSB_ACTIVE + l];
    const int lane = threadIdx.x & 63;
    for (int64_t v0 = (int64_t) blockIdx.x * BFS_THREADS; v0 < V; v0 += (int64_t) gridDim.x * BFS_THREADS) {   // (workgroup-uniform)
        const int64_t v = v0 + threadIdx.x;
        word s = 0, unseen = 0;
        int32_t rb = 0, re = 0;
        if (v < V) {
            s = seen[v];
            unseen = active & ~s;
            if (unseen) {
                rb = begin[v];
                re = begin[v + 1];
            } else {
                sat++;
                next[v] = 0;
            }
        }
        const bool is_long = unseen && (re - rb >= long_min || long_min <= 1);
        const unsigned long long votes = __ballot(is_long);
        if (votes) {
            unsigned int base = 0;
            if (lane == __ffsll((long long) votes) - 1) base = atomicAdd(long_count, (unsigned int) __popcll(votes));
            base = (unsigned int) __shfl((int) base, __ffsll((long long) votes) - 1, 64);
            if (is_long) long_list[base + __popcll(votes & ((1ull << lane) - 1))] = (int32_t) v;
        }
        if (!unseen || is_long) continue;
        word acc = 0;
        int32_t e = rb;
        for (; e + MSB_SHORT_UNROLL <= re && (acc & unseen) != unseen; e += MSB_SHORT_UNROLL) {
            int32_t w[MSB_SHORT_UNROLL];
#pragma unroll
            for (int j = 0; j < MSB_SHORT_UNROLL; j++) w[j] = idx[e + j];
#pragma unroll
            for (int j = 0; j < MSB_SHORT_UNROLL; j++) acc |= front[w[j]];
        }
        for (; e < re && (acc & unseen) != unseen; e++) acc |= front[idx[e]];
        rows++;
        slots += (unsigned long long) (e - rb);
        const word nw = acc & unseen;
        next[v] = nw;
        msb_settle<W>(v, s, nw, l, store != 0, seen, minmax);
        pairs += (unsigned long long) msb_popc(nw);
        columns |= nw;
        if (store)
            for (word left = nw; left; left &= left - 1) lvl[v * W + (msb_popc((word) ((left & (~left + 1)) - 1)))] = (uint8_t) l;
    }
    msb_tally(s_t, tally, l, rows, MSB_ROWS_SHORT, slots, sat, pairs, columns);
}

// level l, the listed rows: a wave per row, lane = slot, MSB_LONG_UNROLL pieces of 64 slots in flight, then the OR across the
// lanes (order-free, so exact) and the exit test; lane b stores column b's level byte
template <int W>
__global__ void __launch_bounds__(BFS_THREADS)
msb_long_kernel(const int32_t* __restrict__ list, const unsigned int* __restrict__ count, const int32_t* __restrict__ begin, const int32_t* __restrict__ idx,
                typename msb_word<W>::type live, int32_t l, int store, typename msb_word<W>::type* __restrict__ seen, const typename msb_word<W>::type* __restrict__ front,
                typename msb_word<W>::type* __restrict__ next, uint8_t* __restrict__ lvl, uint16_t* __restrict__ minmax, unsigned long long* __restrict__ tally) {
    typedef typename msb_word<W>::type word;
    __shared__ unsigned long long s_t[MSB_STATS + 2];
    if (threadIdx.x <= MSB_STATS + 1) s_t[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long rows = 0, slots = 0, pairs = 0;
    word columns = 0;
    const word active = live & (word) tally[MSB_ACTIVE + l];
    const int lane = threadIdx.x & 63;
    const unsigned int n = *count, nwaves = gridDim.x * (BFS_THREADS >> 6);
    for (unsigned int k = blockIdx.x * (BFS_THREADS >> 6) + (threadIdx.x >> 6); k < n; k += nwaves) {   // (wave-uniform)
        const int64_t v = list[k];
        const int32_t rb = begin[v], re = begin[v + 1];
        const word s = seen[v], unseen = active & ~s;
        word acc = 0;
        int32_t base = rb;
        while (base < re) {
            word f[MSB_LONG_UNROLL];
#pragma unroll
            for (int j = 0; j < MSB_LONG_UNROLL; j++) {
                const int32_t e = base + 64 * j + lane;
                f[j] = e < re ? front[idx[e]] : (word) 0;
            }
#pragma unroll
            for (int j = 0; j < MSB_LONG_UNROLL; j++) acc |= f[j];
            acc = msb_wave_or(acc);
            base = re - base > 64 * MSB_LONG_UNROLL ? base + 64 * MSB_LONG_UNROLL : re;
            if ((acc & unseen) == unseen) break;
        }
        const word nw = acc & unseen;
        if (store && lane < W && ((nw >> lane) & 1)) lvl[v * W + lane] = (uint8_t) l;
        if (lane == 0) {
            next[v] = nw;
            msb_settle<W>(v, s, nw, l, store != 0, seen, minmax);
            rows++;
            slots += (unsigned long long) (base - rb);
            pairs += (unsigned long long) msb_popc(nw);
            columns |= nw;
        }
    }
    msb_tally(s_t, tally, l, rows, MSB_ROWS_LONG, slots, 0, pairs, columns);
}

// s.sigma = 1 of every column (with skip_root the root is not visited and keeps it; without, pass 0 overwrites it with an
// empty sum, which is this fork's bc.gm)
__global__ void bcb_seed_kernel(float2* __restrict__ sd, const int32_t* __restrict__ seeds, int32_t nb, int W) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nb) sd[(int64_t) seeds[b] * W + b].x = 1.0f;
}

// ---------------------------------------------------------------- the rows of a pass
// the vertices with some column at level l, split by the length of the row the pass walks; counts[0 / 1] = short / long rows
// listed, *slots += their row slots.  A workgroup stages its finds in LDS and appends once per list.
template <int W>
__global__ void __launch_bounds__(BFS_THREADS)
bcb_find_kernel(const uint16_t* __restrict__ minmax, const uint32_t* __restrict__ lvl, const int32_t* __restrict__ begin, int64_t V, int32_t l, int32_t long_min,
                int32_t* __restrict__ short_list, int32_t* __restrict__ long_list, unsigned int* __restrict__ counts, unsigned long long* __restrict__ slots) {
    __shared__ int32_t s_list[2][BFS_THREADS * BCB_FIND_ITEMS];
    __shared__ unsigned int s_n[2], s_base[2];
    __shared__ unsigned long long s_slots;
    const int64_t per_block = (int64_t) BFS_THREADS * BCB_FIND_ITEMS;
    for (int64_t v0 = (int64_t) blockIdx.x * per_block; v0 < V; v0 += (int64_t) gridDim.x * per_block) {   // (workgroup-uniform)
        if (threadIdx.x == 0) { s_n[0] = s_n[1] = 0; s_slots = 0; }
        __syncthreads();
        unsigned long long my_slots = 0;
#pragma unroll
        for (int k = 0; k < BCB_FIND_ITEMS; k++) {
            const int64_t v = v0 + k * BFS_THREADS + threadIdx.x;
            if (v >= V) continue;
            const uint32_t mm = minmax[v];
            if ((int32_t) (mm & 0xFFu) > l || (int32_t) (mm >> 8) < l) continue;
            bool hit = false;
#pragma unroll
            for (int j = 0; j < W / 4; j++) {
                const uint32_t x = lvl[v * (W / 4) + j];
#pragma unroll
                for (int i = 0; i < 4; i++) hit |= ((x >> (8 * i)) & 0xFFu) == (uint32_t) l;
            }
            if (!hit) continue;
            const int32_t deg = begin[v + 1] - begin[v];
            const int which = deg >= long_min || long_min <= 1;   // (1: every row, the empty ones too)
            s_list[which][atomicAdd(&s_n[which], 1u)] = (int32_t) v;
            my_slots += (unsigned long long) deg;
        }
        if (my_slots) atomicAdd(&s_slots, my_slots);
        __syncthreads();
        if (threadIdx.x < 2 && s_n[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&counts[threadIdx.x], s_n[threadIdx.x]);
        if (threadIdx.x == 2 && s_slots) atomicAdd(slots, s_slots);
        __syncthreads();
        for (unsigned int i = threadIdx.x; i < s_n[0]; i += BFS_THREADS) short_list[s_base[0] + i] = s_list[0][i];
        for (unsigned int i = threadIdx.x; i < s_n[1]; i += BFS_THREADS) long_list[s_base[1] + i] = s_list[1][i];
        __syncthreads();
    }
}

// ---------------------------------------------------------------- the sums
// One term of column `col`: forward, sigma of the up-neighbour; reverse, bc_visit_rv::term's own expression (gmx_bfs.hip;
// the build keeps -ffp-contract=off, so this is a divide, an add and a multiply, each rounded, as the emission has them)
template <bool FWD>
__device__ __forceinline__ float bcb_term(float sv, float2 q) {
    if (FWD) return q.x;
    return sv / q.x * (1 + q.y);
}

// short rows: 64 / W rows per wave, lane = (row of the wave, column); every lane walks its row, BCB_SHORT_UNROLL slots in flight
// (the index loads of a lane group are one address; lvl[w][.] and sd[w][.] are rows of W bytes and W float2).
// A column that does not pass is SKIPPED (S stays), by a select on the sum: no assumption about the terms is needed here.
template <int W, bool FWD>
__global__ void __launch_bounds__(BFS_THREADS)
bcb_short_kernel(const int32_t* __restrict__ list, const unsigned int* __restrict__ count, const int32_t* __restrict__ begin, const int32_t* __restrict__ idx,
                 const uint8_t* __restrict__ lvl, float2* __restrict__ sd, int32_t l, int32_t want) {
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, col = lane % W, r = lane / W;
    const unsigned int n = *count, nwaves = gridDim.x * (BFS_THREADS >> 6);
    for (unsigned int k = blockIdx.x * (BFS_THREADS >> 6) + (threadIdx.x >> 6); (unsigned long long) k * G < n; k += nwaves) {
        const unsigned int i = k * G + r;
        if (i >= n) continue;
        const int32_t v = list[i];
        const int32_t rb = begin[v], re = begin[v + 1];
        const int64_t vo = (int64_t) v * W + col;
        const bool act = lvl[vo] == l;
        const float sv = FWD ? 0.0f : sd[vo].x;
        float S = 0.0f;
        int32_t e = rb;
        for (; e + BCB_SHORT_UNROLL <= re; e += BCB_SHORT_UNROLL) {
            int32_t w[BCB_SHORT_UNROLL];
            int32_t lw[BCB_SHORT_UNROLL];
            float2 q[BCB_SHORT_UNROLL];
#pragma unroll
            for (int j = 0; j < BCB_SHORT_UNROLL; j++) w[j] = idx[e + j];
#pragma unroll
            for (int j = 0; j < BCB_SHORT_UNROLL; j++) lw[j] = lvl[(int64_t) w[j] * W + col];
#pragma unroll
            for (int j = 0; j < BCB_SHORT_UNROLL; j++) q[j] = (act && lw[j] == want) ? sd[(int64_t) w[j] * W + col] : make_float2(1.0f, 0.0f);
#pragma unroll
            for (int j = 0; j < BCB_SHORT_UNROLL; j++) {
                const float next = S + bcb_term<FWD>(sv, q[j]);
                S = (act && lw[j] == want) ? next : S;
            }
        }
        for (; e < re; e++) {
            const int32_t w = idx[e];
            if (act && lvl[(int64_t) w * W + col] == want) S = S + bcb_term<FWD>(sv, sd[(int64_t) w * W + col]);
        }
        if (act) {
            if (FWD) sd[vo].x = S;
            else sd[vo].y = S;
        }
    }
}

// long rows: one workgroup per row.  Waves 1 .. 15 evaluate the terms of consecutive slots into an LDS tile [slot][W]
// (lane = (slot of the wave's 64 / W, column): a tile row of 64 lanes is 64 consecutive words, no bank conflict), 8 tile rows in
// flight per wave and the next step's indices already requested; wave 0 adds the previous tile in slot order, lane = column
// (consecutive words again).  Two tiles, one barrier per step: a step's producers write the tile the adder finished before
// the previous barrier.  Only the adds of a (row, column) are a serial chain; 64 of them run side by side.
// A column that does not pass is stored as +0.0f and ADDED.  That is bit-safe only because these sums start at +0.0f and their
// terms are never negative (path counts; sigma > 0 and delta >= 0 on reached vertices) or are NaN (this fork's form, 0 / 0):
// S is then +0.0f, positive or NaN, and S + (+0.0f) has S's bits -- the NONNEG argument of bfs_ordered_add_dense (gmx_bfs.hip).
template <int W, bool FWD>
__global__ void __launch_bounds__(BCB_LONG_THREADS)
bcb_long_kernel(const int32_t* __restrict__ list, const unsigned int* __restrict__ count, const int32_t* __restrict__ begin, const int32_t* __restrict__ idx,
                const uint8_t* __restrict__ lvl, float2* __restrict__ sd, int32_t l, int32_t want) {
    constexpr int G = 64 / W;
    constexpr int CHUNK = BCB_LONG_ROWS * G;   // slots of a tile
    __shared__ float tile[2][BCB_LONG_ROWS * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane % W, r = lane / W;
    const unsigned int n = *count;
    for (unsigned int k = blockIdx.x; k < n; k += gridDim.x) {   // (workgroup-uniform)
        const int32_t v = list[k];
        const int32_t rb = begin[v], deg = begin[v + 1] - rb;
        const int64_t vo = (int64_t) v * W + col;
        const bool act = lvl[vo] == l;
        const float sv = FWD ? 0.0f : sd[vo].x;
        const int32_t steps = (deg + CHUNK - 1) / CHUNK;
        float S = 0.0f;
        int32_t w[BCB_LONG_UNROLL], wn[BCB_LONG_UNROLL];
        const int32_t first = (wave - 1) * BCB_LONG_UNROLL * G + r;   // the lane's first slot of a tile
        if (wave > 0) {
#pragma unroll
            for (int j = 0; j < BCB_LONG_UNROLL; j++) {
                const int32_t s = first + j * G;
                w[j] = deg > 0 ? idx[rb + (s < deg ? s : deg - 1)] : 0;   // (an empty row, GMX_BCB_LONG_MIN=1: no slot to read)
            }
        }
        for (int32_t c = 0; c <= steps; c++) {
            if (wave > 0 && c < steps) {
                const int32_t s0 = c * CHUNK + first;
                int32_t lw[BCB_LONG_UNROLL];
                float2 q[BCB_LONG_UNROLL];
                bool pass[BCB_LONG_UNROLL];
#pragma unroll
                for (int j = 0; j < BCB_LONG_UNROLL; j++) {   // (the next step's slots, clamped into the row)
                    const int32_t s = s0 + CHUNK + j * G;
                    wn[j] = idx[rb + (s < deg ? s : deg - 1)];
                }
#pragma unroll
                for (int j = 0; j < BCB_LONG_UNROLL; j++) lw[j] = lvl[(int64_t) w[j] * W + col];
#pragma unroll
                for (int j = 0; j < BCB_LONG_UNROLL; j++) {
                    pass[j] = act && s0 + j * G < deg && lw[j] == want;
                    q[j] = pass[j] ? sd[(int64_t) w[j] * W + col] : make_float2(1.0f, 0.0f);
                }
#pragma unroll
                for (int j = 0; j < BCB_LONG_UNROLL; j++) {
                    tile[c & 1][((wave - 1) * BCB_LONG_UNROLL + j) * 64 + lane] = pass[j] ? bcb_term<FWD>(sv, q[j]) : 0.0f;
                    w[j] = wn[j];
                }
            }
            if (wave == 0 && c > 0 && lane < W) {
                const float* t = tile[(c - 1) & 1];
                const int32_t left = deg - (c - 1) * CHUNK, ns = left < CHUNK ? left : CHUNK;
                int32_t s = 0;
                for (; s + 8 <= ns; s += 8) {
                    float x[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) x[j] = t[(s + j) * W + lane];
#pragma unroll
                    for (int j = 0; j < 8; j++) S = S + x[j];
                }
                for (; s < ns; s++) S = S + t[s * W + lane];
            }
            __syncthreads();
        }
        if (wave == 0 && lane < W && act) {
            if (FWD) sd[vo].x = S;
            else sd[vo].y = S;
        }
    }
}

// v.BC += v.delta of every seed of the batch that reaches v, in seed order (columns ascending); with skip_root not for the
// seed itself (the one vertex at level 0 of its column)
template <int W>
__global__ void __launch_bounds__(BFS_THREADS)
bcb_accumulate_kernel(const uint32_t* __restrict__ lvl, const float2* __restrict__ sd, int64_t V, int32_t skip_root, float* __restrict__ bc) {
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) {
        float x = bc[v];
        bool any = false;
#pragma unroll
        for (int j = 0; j < W / 4; j++) {
            const uint32_t four = lvl[v * (W / 4) + j];
            if (four == 0xFFFFFFFFu) continue;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t lv = (four >> (8 * i)) & 0xFFu;
                if (lv == BCB_UNREACHED || (skip_root && lv == 0)) continue;
                x = x + sd[v * W + 4 * j + i].y;
                any = true;
            }
        }
        if (any) bc[v] = x;
    }
}

// ---------------------------------------------------------------- host side
// device bytes of a batch of width W on V vertices: sd 8, lvl 1 and the staged levels 1 per (vertex, column); two row lists,
// minmax and a little padding per vertex (the rule include/gmx.h states for GMX_BCB_MEM_MB)
static size_t bcb_bytes(int64_t V, int W) { return (size_t) V * (10 * (size_t) W + 10) + 4096 * (size_t) W; }

struct bcb_totals { long long rows_short = 0, rows_long = 0, slots = 0; };

static void bcb_trace(bool on, int64_t batch, int32_t nb, int W, int32_t depth, bool batched, const bcb_totals& t) {
    if (on) fprintf(stderr, "gmx bc_batch batch %lld: seeds %d width %d depth %d path %s rows %lld short + %lld long, slots %lld\n", (long long) batch, nb, W,
                    depth, batched ? "batched" : "per-seed", t.rows_short, t.rows_long, t.slots);
}

struct bcb_knobs {
    int32_t max_depth, long_min, ms_long_min;
    bool trace, msbfs;
};

// The levels of one batch by the multi-source traversal: lvl, minmax, the deepest level and the reached (vertex, column)
// pairs, roots included.  One host synchronisation per level (the level's count of new pairs).  *batched = false: level
// max_depth + 1 is not empty (no byte of it was stored); the batch then runs per seed.  `masks` is the stage buffer.
template <int W>
static int bcb_msbfs(gmx_graph* g, const int32_t* seeds_dev, int32_t nb, const bcb_knobs& kn, void* masks, uint32_t* lvl, uint16_t* minmax, int32_t* long_list,
                     unsigned int* long_counts, unsigned long long* tally, int32_t* deepest_out, int64_t* reached_out, bool* batched_out) {
    typedef typename msb_word<W>::type word;
    const int64_t V = g->V;
    word* seen = (word*) masks;
    word* front = seen + V;
    word* next = front + V;
    const word live = nb >= W ? ~(word) 0 : (word) (((word) 1 << nb) - 1);
    const int level_grid = grid_for(V, BFS_THREADS, 256 * 8);
    const int long_grid = grid_for(V, BFS_THREADS >> 6, 256 * 8);
    GMX_HIP(hipMemsetAsync(tally, 0, sizeof(unsigned long long) * MSB_TALLY, 0));
    GMX_HIP(hipMemsetAsync(long_counts, 0, sizeof(unsigned int) * (BCB_DEPTH_CAP + 2), 0));
    hipLaunchKernelGGL((msb_clear_kernel<W>), dim3(grid_for(V * (W / 4))), dim3(BFS_THREADS), 0, 0, V, seen, front, lvl, minmax);
    hipLaunchKernelGGL((msb_seed_kernel<W>), dim3(1), dim3(64), 0, 0, seeds_dev, nb, seen, front, (uint8_t*) lvl, minmax, tally);
    int32_t deepest = 0;
    int64_t reached = nb;
    bool batched = true;
    for (int32_t l = 1;; l++) {
        const int store = l <= kn.max_depth;
        hipLaunchKernelGGL((msb_level_kernel<W>), dim3(level_grid), dim3(BFS_THREADS), 0, 0, (const int32_t*) g->r_begin.p, (const int32_t*) g->r_node_idx.p, V, live, l,
                           kn.ms_long_min, store, seen, (const word*) front, next, (uint8_t*) lvl, minmax, long_list, long_counts + l, tally);
        hipLaunchKernelGGL((msb_long_kernel<W>), dim3(long_grid), dim3(BFS_THREADS), 0, 0, (const int32_t*) long_list, (const unsigned int*) (long_counts + l),
                           (const int32_t*) g->r_begin.p, (const int32_t*) g->r_node_idx.p, live, l, store, seen, (const word*) front, next, (uint8_t*) lvl, minmax, tally);
        GMX_HIP(hipGetLastError());
        unsigned long long found = 0;
        GMX_HIP(hipMemcpy(&found, tally + MSB_STATS + l, sizeof(found), hipMemcpyDeviceToHost));
        if (!found) break;
        deepest = l;
        if (!store) {   // deeper than the cap (l = max_depth + 1 <= 255)
            batched = false;
            break;
        }
        reached += (int64_t) found;
        word* t = front;
        front = next;
        next = t;
    }
    *deepest_out = deepest;
    *reached_out = reached;
    *batched_out = batched;
    return GMX_OK;
}

static int bcb_msbfs_trace(bool on, int64_t batch, int32_t levels, const unsigned long long* tally) {
    if (!on) return GMX_OK;
    unsigned long long h[MSB_STATS];
    GMX_HIP(hipMemcpy(h, tally, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "gmx bc_batch msbfs batch %lld: levels %d rows %llu short + %llu long slots %llu saturated %llu\n", (long long) batch, levels, h[MSB_ROWS_SHORT],
            h[MSB_ROWS_LONG], h[MSB_SLOTS], h[MSB_SATURATED]);
    return GMX_OK;
}

// the batches of width W; bc (device) is zeroed and then accumulates in seed order.  tm's kernel span begins once the work
// buffers exist (no allocation after it)
template <int W>
static int bcb_run(gmx_graph* g, const gmx_node_t* seeds, const int32_t* seeds_dev, int32_t nseeds, int skip_root, const bcb_knobs& kn, float* bc,
                   gmx_spans& tm, int64_t* reached_out, int64_t* slots_out) {
    const int64_t V = g->V;
    const int64_t pitch_words = ((V + 255) / 256) * 64;   // a staged column, in words of four vertices
    dbuf<float2> sd;
    dbuf<uint32_t> lvl, stage;
    dbuf<uint16_t> minmax;
    dbuf<int32_t> short_list, long_list, depth;
    dbuf<unsigned int> counts;             // [pass][2] rows listed
    dbuf<unsigned long long> tally;        // [0] slots walked, [1 + b] vertices column b reaches
    dbuf<unsigned long long> ms_tally;     // the multi-source traversal's counters: MSB_STATS of them, then the new pairs of every level
    GMX_CHECK(sd.alloc((size_t) V * W));
    GMX_CHECK(lvl.alloc((size_t) V * (W / 4)));
    GMX_CHECK(stage.alloc((size_t) pitch_words * W));
    GMX_CHECK(minmax.alloc((size_t) V));
    GMX_CHECK(short_list.alloc((size_t) V));
    GMX_CHECK(long_list.alloc((size_t) V));
    GMX_CHECK(depth.alloc(W));
    GMX_CHECK(counts.alloc(2 * BCB_MAX_PASSES));
    GMX_CHECK(tally.alloc(1 + W));
    if (kn.msbfs) GMX_CHECK(ms_tally.alloc(MSB_TALLY));
    std::vector<unsigned int> h_counts(2 * BCB_MAX_PASSES);
    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_HIP(hipMemsetAsync(bc, 0, sizeof(float) * (size_t) V, 0));   // G.BC = 0
    const uint8_t* lvl8 = (const uint8_t*) lvl.p;
    const int vblocks = (int) ((V + 255) / 256);
    const int find_grid = grid_for(V, BFS_THREADS * BCB_FIND_ITEMS, 256 * 8);
    const int short_grid = grid_for((V + 64 / W - 1) / (64 / W), BFS_THREADS / 64, 256 * 8);
    const int long_grid = grid_for(V, 1, 256 * 2);
    int64_t reached = 0, slots = 0;
    for (int64_t off = 0, batch = 0; off < nseeds; off += W, batch++) {
        const int32_t nb = (int32_t) (nseeds - off < W ? nseeds - off : W);
        GMX_HIP(hipMemsetAsync(depth.p, 0, sizeof(int32_t) * W, 0));
        GMX_HIP(hipMemsetAsync(tally.p, 0, sizeof(unsigned long long) * (1 + W), 0));
        // the traversals, one seed at a time; a seed deeper than the cap ends them: the batch then runs per seed
        int32_t deepest = 0;
        int64_t batch_reached = 0;
        bool batched = true;
        if (kn.msbfs) GMX_CHECK(bcb_msbfs<W>(g, seeds_dev + off, nb, kn, stage.p, lvl.p, minmax.p, long_list.p, counts.p, ms_tally.p, &deepest, &batch_reached, &batched));
        for (int32_t b = 0; b < nb && batched && !kn.msbfs; b++) {
            const int32_t* dist = nullptr;
            int64_t edges = 0;
            GMX_CHECK(gmx_bfs_reach(g, seeds[off + b], &dist, &edges));
            hipLaunchKernelGGL(bcb_stage_kernel, dim3(grid_for((V + 3) / 4)), dim3(BFS_THREADS), 0, 0, dist, V, stage.p + (int64_t) b * pitch_words, depth.p + b, tally.p + 1 + b);
            int32_t d = 0;
            unsigned long long r = 0;
            GMX_HIP(hipMemcpy(&d, depth.p + b, sizeof(d), hipMemcpyDeviceToHost));
            GMX_HIP(hipMemcpy(&r, tally.p + 1 + b, sizeof(r), hipMemcpyDeviceToHost));
            deepest = d > deepest ? d : deepest;
            batch_reached += (int64_t) r;
            batched = d <= kn.max_depth;
        }
        bcb_totals tot;
        if (!batched) {
            GMX_CHECK(gmx_bc_seeds(g, seeds + off, nb, skip_root, bc, false, nullptr, &batch_reached));
            reached += batch_reached;
            bcb_trace(kn.trace, batch, nb, W, deepest, false, tot);
            if (kn.msbfs) GMX_CHECK(bcb_msbfs_trace(kn.trace, batch, deepest, ms_tally.p));
            continue;
        }
        reached += batch_reached;
        if (!kn.msbfs) hipLaunchKernelGGL((bcb_transpose_kernel<W>), dim3(vblocks), dim3(256), 0, 0, (const uint32_t*) stage.p, V, pitch_words, nb, lvl.p, minmax.p);
        hipLaunchKernelGGL(bcb_seed_kernel, dim3(1), dim3(64), 0, 0, sd.p, seeds_dev + off, nb, W);
        const int32_t l0 = skip_root ? 1 : 0;   // with skip_root the roots (level 0 of their column) are not visited
        const int32_t npass = deepest >= l0 ? 2 * (deepest - l0 + 1) : 0;
        GMX_HIP(hipMemsetAsync(counts.p, 0, sizeof(unsigned int) * 2 * (size_t) (npass > 0 ? npass : 1), 0));
        int32_t pass = 0;
        for (int32_t l = l0; l <= deepest; l++, pass++) {   // sigma: the reverse rows, sources one level up
            unsigned int* cnt = counts.p + 2 * pass;
            hipLaunchKernelGGL((bcb_find_kernel<W>), dim3(find_grid), dim3(BFS_THREADS), 0, 0, (const uint16_t*) minmax.p, (const uint32_t*) lvl.p, (const int32_t*) g->r_begin.p, V, l,
                               kn.long_min, short_list.p, long_list.p, cnt, tally.p);
            hipLaunchKernelGGL((bcb_short_kernel<W, true>), dim3(short_grid), dim3(BFS_THREADS), 0, 0, (const int32_t*) short_list.p, (const unsigned int*) cnt,
                               (const int32_t*) g->r_begin.p, (const int32_t*) g->r_node_idx.p, lvl8, sd.p, l, l - 1);
            hipLaunchKernelGGL((bcb_long_kernel<W, true>), dim3(long_grid), dim3(BCB_LONG_THREADS), 0, 0, (const int32_t*) long_list.p, (const unsigned int*) (cnt + 1),
                               (const int32_t*) g->r_begin.p, (const int32_t*) g->r_node_idx.p, lvl8, sd.p, l, l - 1);
        }
        for (int32_t l = deepest; l >= l0; l--, pass++) {   // delta: the forward rows, targets one level down
            unsigned int* cnt = counts.p + 2 * pass;
            const int32_t want = l < deepest ? l + 1 : 256;   // (nothing lies below the deepest level; 255 would match BCB_UNREACHED)
            hipLaunchKernelGGL((bcb_find_kernel<W>), dim3(find_grid), dim3(BFS_THREADS), 0, 0, (const uint16_t*) minmax.p, (const uint32_t*) lvl.p, (const int32_t*) g->begin.p, V, l,
                               kn.long_min, short_list.p, long_list.p, cnt, tally.p);
            hipLaunchKernelGGL((bcb_short_kernel<W, false>), dim3(short_grid), dim3(BFS_THREADS), 0, 0, (const int32_t*) short_list.p, (const unsigned int*) cnt,
                               (const int32_t*) g->begin.p, (const int32_t*) g->node_idx.p, lvl8, sd.p, l, want);
            hipLaunchKernelGGL((bcb_long_kernel<W, false>), dim3(long_grid), dim3(BCB_LONG_THREADS), 0, 0, (const int32_t*) long_list.p, (const unsigned int*) (cnt + 1),
                               (const int32_t*) g->begin.p, (const int32_t*) g->node_idx.p, lvl8, sd.p, l, want);
        }
        hipLaunchKernelGGL((bcb_accumulate_kernel<W>), dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, (const uint32_t*) lvl.p, (const float2*) sd.p, V, (int32_t) (skip_root != 0), bc);
        GMX_HIP(hipGetLastError());
        unsigned long long batch_slots = 0;
        GMX_HIP(hipMemcpy(&batch_slots, tally.p, sizeof(batch_slots), hipMemcpyDeviceToHost));
        slots += (int64_t) batch_slots;
        if (kn.trace) {
            if (npass > 0) GMX_HIP(hipMemcpy(h_counts.data(), counts.p, sizeof(unsigned int) * 2 * (size_t) npass, hipMemcpyDeviceToHost));
            for (int32_t p = 0; p < npass; p++) {
                tot.rows_short += h_counts[2 * (size_t) p];
                tot.rows_long += h_counts[2 * (size_t) p + 1];
            }
            tot.slots = (long long) batch_slots;
            bcb_trace(true, batch, nb, W, deepest, true, tot);
            if (kn.msbfs) GMX_CHECK(bcb_msbfs_trace(true, batch, deepest, ms_tally.p));
        }
    }
    *reached_out = reached;
    *slots_out = slots;
    return GMX_OK;
}

#define BCB_DEFAULT_WIDTH 64   // width = 0 without GMX_BCB_WIDTH: the best median at RMAT-24 (the measured table)

// gmx_bc_batch and gmx_bc_all behind their argument checks; msbfs_default: GMX_BCB_MSBFS when the environment does not set it
static int bcb_call(gmx_graph_t* g, const gmx_node_t* seeds, int32_t nseeds, int skip_root, int32_t width, float* bc_host, gmx_stats_t* stats, int msbfs_default) {
    const int64_t V = g->V;
    bcb_knobs kn;
    kn.max_depth = (int32_t) gmx_env_int("GMX_BCB_MAX_DEPTH", BCB_DEPTH_CAP, 0, BCB_DEPTH_CAP);   // (the environment lowers it, never raises it)
    kn.long_min = (int32_t) gmx_env_int("GMX_BCB_LONG_MIN", 256, 1, INT_MAX);
    kn.trace = gmx_env_int("GMX_BCB_TRACE", 0, 0, 1) != 0;
    kn.msbfs = gmx_env_int("GMX_BCB_MSBFS", msbfs_default, 0, 1) != 0;
    kn.ms_long_min = (int32_t) gmx_env_int("GMX_BCB_MS_LONG_MIN", 256, 1, INT_MAX);
    int W = width;
    if (W == 0) {
        W = (int) gmx_env_int("GMX_BCB_WIDTH", BCB_DEFAULT_WIDTH, 0, 1 << 20);
        GMX_REQUIRE(W == 1 || W == 16 || W == 32 || W == 64, "GMX_BCB_WIDTH=%d: 1, 16, 32 or 64", W);
        while (W > 16 && W / 2 >= nseeds) W /= 2;   // (no wider than the seeds need)
    }
    if (W > 1) {   // a batch has to fit: halve the width down to 16, then the per-seed path
        size_t free_b = 0, total_b = 0;
        GMX_HIP(hipMemGetInfo(&free_b, &total_b));
        const int64_t cap_mb = gmx_env_int("GMX_BCB_MEM_MB", -1, 0, INT64_MAX >> 20);
        const size_t room = cap_mb >= 0 && (size_t) cap_mb << 20 < free_b ? (size_t) cap_mb << 20 : free_b;
        while (W >= 16 && bcb_bytes(V, W) > room) W /= 2;
        if (W < 16) W = 1;
    }
    if (W == 1) {   // the existing per-seed path, whole
        GMX_CHECK(gmx_bc(g, seeds, nseeds, skip_root, bc_host, stats));
        bcb_trace(kn.trace, 0, nseeds, 1, 0, false, bcb_totals());
        return GMX_OK;
    }
    dbuf<float> bc;
    dbuf<int32_t> seeds_dev;
    GMX_CHECK(bc.alloc((size_t) V));
    GMX_CHECK(seeds_dev.alloc((size_t) nseeds));
    if (nseeds) GMX_HIP(hipMemcpy(seeds_dev.p, seeds, sizeof(int32_t) * (size_t) nseeds, hipMemcpyHostToDevice));
    gmx_spans tm;
    int64_t reached = 0, slots = 0;
    if (W == 16) GMX_CHECK(bcb_run<16>(g, seeds, seeds_dev.p, nseeds, skip_root, kn, bc.p, tm, &reached, &slots));
    else if (W == 32) GMX_CHECK(bcb_run<32>(g, seeds, seeds_dev.p, nseeds, skip_root, kn, bc.p, tm, &reached, &slots));
    else GMX_CHECK(bcb_run<64>(g, seeds, seeds_dev.p, nseeds, skip_root, kn, bc.p, tm, &reached, &slots));
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.finish(stats));
    GMX_HIP(hipMemcpy(bc_host, bc.p, sizeof(float) * (size_t) V, hipMemcpyDeviceToHost));
    if (stats) {
        stats->iterations = nseeds;
        stats->vertices_reached = reached;
        stats->edges_examined = slots;
    }
    return GMX_OK;
}

extern "C" int gmx_bc_batch(gmx_graph_t* g, const gmx_node_t* seeds, int32_t nseeds, int skip_root, int32_t width, float* bc_host, gmx_stats_t* stats) {
    GMX_REQUIRE(g && bc_host && (seeds || nseeds == 0) && nseeds >= 0, "bad argument");
    GMX_REQUIRE(width == 0 || width == 1 || width == 16 || width == 32 || width == 64, "width %d: 0, 1, 16, 32 or 64", width);
    GMX_REQUIRE(g->has_reverse, "comp_BC needs the reverse CSR (UpNbrs)");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (g->V == 0) return GMX_OK;
    for (int32_t i = 0; i < nseeds; i++) GMX_REQUIRE(seeds[i] >= 0 && seeds[i] < g->V, "seed %d out of range", seeds[i]);
    return bcb_call(g, seeds, nseeds, skip_root, width, bc_host, stats, 0);
}

// comp_BC(G, BC) of bc_adj.gm: every vertex a source, in node order
extern "C" int gmx_bc_all(gmx_graph_t* g, int skip_root, int32_t width, float* bc_host, gmx_stats_t* stats) {
    GMX_REQUIRE(g && bc_host, "bad argument");
    GMX_REQUIRE(width == 0 || width == 1 || width == 16 || width == 32 || width == 64, "width %d: 0, 1, 16, 32 or 64", width);
    GMX_REQUIRE(g->has_reverse, "comp_BC needs the reverse CSR (UpNbrs)");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (g->V == 0) return GMX_OK;
    GMX_REQUIRE(g->V <= INT32_MAX, "too many vertices");
    std::vector<gmx_node_t> seeds((size_t) g->V);
    for (int64_t v = 0; v < g->V; v++) seeds[(size_t) v] = (gmx_node_t) v;
    return bcb_call(g, seeds.data(), (int32_t) g->V, skip_root, width, bc_host, stats, 1);
}

void gmx_touch_bc_batch() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) bcb_stage_kernel);
}
