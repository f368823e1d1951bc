// gmx_close.hip -- closeness, harmonic centrality and eccentricity (gmx_closeness, include/gmx.h).
//
// Distance centralities need no per-column state: a vertex only has to know HOW MANY columns (sources) reached it at level
// l.  So the bit-parallel multi-source traversal of gmx_bc_all (gmx_bc_batch.hip, msb_*) is run here without level bytes,
// hence without a depth cap, and wide: seen / front / next hold B words of 64 bits per vertex, vertex-major ([V][B], B = 1,
// 2 or 4), so a neighbour's front is one aligned load of 8 B bytes and one sweep of the rows carries 64 B sources.  A level
// is a pull: a vertex that still lacks a column whose front is not empty ORs front[] over its row (the forward row for
// GMX_CLOSE_OUT, the reverse row for _IN, one after the other for _BOTH), keeps the bits it has not seen and folds their
// popcount into its own four accumulators:  reach += cnt, far += cnt * l, ecc = max(ecc, l), harm += cnt * floor(2^32 / l).
// It writes only its own words -- front[] of the others is written by no kernel of that level -- so there is no atomic on
// the state or on a result, every result is an integer sum or maximum, and the bytes are those of a one-thread BFS under
// every width, knob and row regime.  Rows shorter than GMX_CLOSE_LONG_MIN slots are walked by their owner's lane
// (close_level_kernel), the others are listed and walked by a wave each (close_long_kernel); both stop once every missing
// column is covered.  Only columns whose front is not empty can be found: a level ORs the words it writes into the next
// level's `active` words (one atomic per workgroup and word), and a vertex that misses none of those only clears its next
// words.  The per-level words (new pairs, active, listed rows) live in a ring of CL_RING slots, so depth is unbounded: level
// l reads slot l % CL_RING, writes slot (l + 1) % CL_RING and clears slot (l + 2) % CL_RING, which held level l + 2 - CL_RING's
// words.  The host launches GMX_CLOSE_BATCH levels (at most CL_RING - 2) and then reads their new-pair counts in one copy:
// a level past the sweep's last finds every vertex saturated and changes nothing.
#include "gmx_internal.h"
#include "gmx_frontier.h"

#include <limits.h>

#define CL_SHORT_UNROLL 4   // slots of a short row in flight per lane
#define CL_LONG_UNROLL 4    // 64-slot pieces of a long row in flight per wave, then one cross-lane OR and the exit test
#define CL_MAX_WORDS 4
#define CL_RING 6           // slots of the per-level ring: the levels of a batch, the one they write ahead and the one they clear
// the control block, in 64-bit words: four counters that run over the whole call, then the ring
enum { CL_LANE = 0, CL_WAVE = 1, CL_SAT = 2, CL_SLOTS = 3, CL_FOUND = 4, CL_LONGN = CL_FOUND + CL_RING, CL_ACTIVE = CL_LONGN + CL_RING,
       CL_CTL = CL_ACTIVE + CL_RING * CL_MAX_WORDS };

template <int B>
struct alignas(B == 1 ? 8 : 16) cl_vec {
    uint64_t w[B];
};

template <int B>
__device__ __forceinline__ bool cl_covers(const cl_vec<B>& acc, const cl_vec<B>& want) {
    uint64_t miss = 0;
#pragma unroll
    for (int j = 0; j < B; j++) miss |= want.w[j] & ~acc.w[j];
    return miss == 0;
}
__device__ __forceinline__ uint64_t cl_wave_or(uint64_t x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x |= (uint64_t) __shfl_xor((unsigned long long) x, d, 64);
    return x;
}
__device__ __forceinline__ unsigned int cl_wave_sum(unsigned int x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += (unsigned int) __shfl_xor((int) x, d, 64);
    return x;
}

// the rows with at least long_min slots (the rows a level can list at most): sizes the wave kernel's grid, once per call
__global__ void __launch_bounds__(BFS_THREADS)
close_count_long_kernel(const int32_t* __restrict__ begin0, const int32_t* __restrict__ begin1, int64_t V, int32_t long_min, unsigned long long* __restrict__ out) {
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned int n = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) {
        const int64_t deg = (int64_t) (begin0[v + 1] - begin0[v]) + (begin1 ? (int64_t) (begin1[v + 1] - begin1[v]) : 0);
        n += deg >= long_min || long_min <= 1;
    }
    n = cl_wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, (unsigned long long) n);
}

// a sweep's level 0: the ring cleared, column c on its source (sources == NULL: vertex first + c).  Duplicate sources are
// independent columns on one vertex, so the bits are ORed in; this is the only atomic on the state, and it is order-free
template <int B>
__global__ void __launch_bounds__(64 * CL_MAX_WORDS)
close_seed_kernel(const int32_t* __restrict__ sources, int64_t first, int32_t nb, uint64_t* __restrict__ seen, uint64_t* __restrict__ front, unsigned long long* __restrict__ ctl) {
    const int c = threadIdx.x;
    if (c >= CL_FOUND && c < CL_CTL) {
        const int j = c - (CL_ACTIVE + B);   // word j of level 1's active: every column has its root in level 1's front
        const int left = nb - 64 * j;
        ctl[c] = (j >= 0 && j < B && left > 0) ? (left >= 64 ? ~0ull : (1ull << left) - 1) : 0ull;
    }
    if (c < nb) {
        const int64_t s = sources ? (int64_t) sources[first + c] : first + c;
        atomicOr((unsigned long long*) &seen[s * B + (c >> 6)], 1ull << (c & 63));
        atomicOr((unsigned long long*) &front[s * B + (c >> 6)], 1ull << (c & 63));
    }
}

// what a vertex does with the columns a level found for it: its own words and its own accumulators only
template <int B>
__device__ __forceinline__ unsigned int cl_settle(int64_t v, const cl_vec<B>& s, const cl_vec<B>& nw, int32_t l, uint64_t r_of_l, cl_vec<B>* __restrict__ seen,
                                                  cl_vec<B>* __restrict__ next, int64_t* __restrict__ far, int32_t* __restrict__ reach, int32_t* __restrict__ ecc,
                                                  uint64_t* __restrict__ harm) {
    unsigned int cnt = 0;
#pragma unroll
    for (int j = 0; j < B; j++) cnt += (unsigned int) __popcll(nw.w[j]);
    next[v] = nw;
    if (cnt) {
        cl_vec<B> t;
#pragma unroll
        for (int j = 0; j < B; j++) t.w[j] = s.w[j] | nw.w[j];
        seen[v] = t;
        reach[v] += (int32_t) cnt;
        far[v] += (int64_t) cnt * l;
        const int32_t e = ecc[v];
        ecc[v] = e > l ? e : l;   // (levels ascend within a sweep; the maximum is across sweeps)
        harm[v] += (uint64_t) cnt * r_of_l;
    }
    return cnt;
}

// a workgroup's counters into the control block and the columns it found into the next level's active words: one atomic
// per workgroup and non-zero value.  lanes / waves / sat are what lane 0 of each wave holds for the wave, slots / pairs / cols per lane
template <int B>
__device__ __forceinline__ void cl_tally(unsigned long long* s_t, unsigned long long* __restrict__ ctl, int32_t l, unsigned int lanes, unsigned int waves, unsigned int sat,
                                         unsigned int slots, unsigned int pairs, const cl_vec<B>& cols) {
    slots = cl_wave_sum(slots);
    pairs = cl_wave_sum(pairs);
    uint64_t c[B];
#pragma unroll
    for (int j = 0; j < B; j++) c[j] = cl_wave_or(cols.w[j]);
    if ((threadIdx.x & 63) == 0) {
        if (lanes) atomicAdd(&s_t[0], (unsigned long long) lanes);
        if (waves) atomicAdd(&s_t[1], (unsigned long long) waves);
        if (sat) atomicAdd(&s_t[2], (unsigned long long) sat);
        if (slots) atomicAdd(&s_t[3], (unsigned long long) slots);
        if (pairs) atomicAdd(&s_t[4], (unsigned long long) pairs);
#pragma unroll
        for (int j = 0; j < B; j++)
            if (c[j]) atomicOr(&s_t[5 + j], (unsigned long long) c[j]);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 5 + B && s_t[t]) {
        if (t < 4) atomicAdd(&ctl[t], s_t[t]);
        else if (t == 4) atomicAdd(&ctl[CL_FOUND + l % CL_RING], s_t[t]);
        else atomicOr(&ctl[CL_ACTIVE + ((l + 1) % CL_RING) * B + (t - 5)], s_t[t]);
    }
}

// level l, every vertex: saturated ones (no column missing whose front is not empty) only clear their next words; rows of
// at least long_min slots go to long_list (one append per wave); the others are walked here, row 0 and then (NR = 2: BOTH)
// row 1, CL_SHORT_UNROLL slots in flight
template <int B, int NR>
__global__ void __launch_bounds__(BFS_THREADS)
close_level_kernel(const int32_t* __restrict__ begin0, const int32_t* __restrict__ idx0, const int32_t* __restrict__ begin1, const int32_t* __restrict__ idx1, int64_t V,
                   int32_t l, uint64_t r_of_l, int32_t long_min, cl_vec<B>* __restrict__ seen, const cl_vec<B>* __restrict__ front, cl_vec<B>* __restrict__ next,
                   int64_t* __restrict__ far, int32_t* __restrict__ reach, int32_t* __restrict__ ecc, uint64_t* __restrict__ harm, int32_t* __restrict__ long_list,
                   unsigned long long* __restrict__ ctl) {
    __shared__ unsigned long long s_t[5 + CL_MAX_WORDS];
    if (threadIdx.x < 5 + CL_MAX_WORDS) s_t[threadIdx.x] = 0;
    if (blockIdx.x == 0) {   // the ring slot of level l + 2: the host has read what level l + 2 - CL_RING left there
        const int slot = (l + 2) % CL_RING;
        if (threadIdx.x == 0) ctl[CL_FOUND + slot] = 0;
        if (threadIdx.x == 1) ctl[CL_LONGN + slot] = 0;
        if (threadIdx.x >= 2 && threadIdx.x < 2 + B) ctl[CL_ACTIVE + slot * B + (threadIdx.x - 2)] = 0;
    }
    __syncthreads();
    cl_vec<B> active, cols;
#pragma unroll
    for (int j = 0; j < B; j++) {
        active.w[j] = ctl[CL_ACTIVE + (l % CL_RING) * B + j];
        cols.w[j] = 0;
    }
    unsigned long long* long_count = ctl + CL_LONGN + l % CL_RING;
    unsigned int lanes = 0, sat = 0, slots = 0, pairs = 0;
    const int lane = threadIdx.x & 63;
    for (int64_t v0 = (int64_t) blockIdx.x * BFS_THREADS; v0 < V; v0 += (int64_t) gridDim.x * BFS_THREADS) {   // (workgroup-uniform)
        const int64_t v = v0 + threadIdx.x;
        cl_vec<B> s, unseen;
        uint64_t any = 0;
        int32_t rb[NR], re[NR];
        int64_t deg = 0;
        bool saturated = false;
#pragma unroll
        for (int j = 0; j < B; j++) s.w[j] = unseen.w[j] = 0;
        if (v < V) {
            s = seen[v];
#pragma unroll
            for (int j = 0; j < B; j++) {
                unseen.w[j] = active.w[j] & ~s.w[j];
                any |= unseen.w[j];
            }
            if (any) {
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    const int32_t* __restrict__ bg = r ? begin1 : begin0;
                    rb[r] = bg[v];
                    re[r] = bg[v + 1];
                    deg += re[r] - rb[r];
                }
            } else {
                saturated = true;
                cl_vec<B> zero;
#pragma unroll
                for (int j = 0; j < B; j++) zero.w[j] = 0;
                next[v] = zero;
            }
        }
        const bool is_long = any && (deg >= long_min || long_min <= 1);
        const unsigned long long votes = __ballot(is_long);
        sat += (unsigned int) __popcll(__ballot(saturated));
        lanes += (unsigned int) __popcll(__ballot(any && !is_long));
        if (votes) {
            unsigned long long base = 0;
            const int leader = __ffsll((long long) votes) - 1;
            if (lane == leader) base = atomicAdd(long_count, (unsigned long long) __popcll(votes));
            base = (unsigned long long) __shfl((long long) base, leader, 64);
            if (is_long) long_list[base + __popcll(votes & ((1ull << lane) - 1))] = (int32_t) v;   // (at most V entries: a vertex is listed once a level)
        }
        if (!any || is_long) continue;
        cl_vec<B> acc;
#pragma unroll
        for (int j = 0; j < B; j++) acc.w[j] = 0;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int32_t* __restrict__ idx = r ? idx1 : idx0;
            int32_t e = rb[r];
            for (; e + CL_SHORT_UNROLL <= re[r] && !cl_covers<B>(acc, unseen); e += CL_SHORT_UNROLL) {
                int32_t w[CL_SHORT_UNROLL];
                cl_vec<B> f[CL_SHORT_UNROLL];
#pragma unroll
                for (int j = 0; j < CL_SHORT_UNROLL; j++) w[j] = idx[e + j];
#pragma unroll
                for (int j = 0; j < CL_SHORT_UNROLL; j++) f[j] = front[w[j]];
#pragma unroll
                for (int j = 0; j < CL_SHORT_UNROLL; j++)
#pragma unroll
                    for (int k = 0; k < B; k++) acc.w[k] |= f[j].w[k];
            }
            for (; e < re[r] && !cl_covers<B>(acc, unseen); e++) {
                const cl_vec<B> f = front[idx[e]];
#pragma unroll
                for (int k = 0; k < B; k++) acc.w[k] |= f.w[k];
            }
            slots += (unsigned int) (e - rb[r]);
        }
        cl_vec<B> nw;
#pragma unroll
        for (int j = 0; j < B; j++) {
            nw.w[j] = acc.w[j] & unseen.w[j];
            cols.w[j] |= nw.w[j];
        }
        pairs += cl_settle<B>(v, s, nw, l, r_of_l, seen, next, far, reach, ecc, harm);
    }
    cl_tally<B>(s_t, ctl, l, lanes, 0, sat, slots, pairs, cols);   // (the listed rows are counted by the kernel that walks them)
}

// level l, the listed rows: a wave per row, lane = slot, CL_LONG_UNROLL pieces of 64 slots in flight, then the OR across the
// lanes (order-free, so exact) and the exit test per word; under BOTH the walk goes on from the forward row into the reverse row
template <int B, int NR>
__global__ void __launch_bounds__(BFS_THREADS)
close_long_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ begin0, const int32_t* __restrict__ idx0, const int32_t* __restrict__ begin1,
                  const int32_t* __restrict__ idx1, int32_t l, uint64_t r_of_l, cl_vec<B>* __restrict__ seen, const cl_vec<B>* __restrict__ front, cl_vec<B>* __restrict__ next,
                  int64_t* __restrict__ far, int32_t* __restrict__ reach, int32_t* __restrict__ ecc, uint64_t* __restrict__ harm, unsigned long long* __restrict__ ctl) {
    __shared__ unsigned long long s_t[5 + CL_MAX_WORDS];
    if (threadIdx.x < 5 + CL_MAX_WORDS) s_t[threadIdx.x] = 0;
    __syncthreads();
    cl_vec<B> active, cols;
#pragma unroll
    for (int j = 0; j < B; j++) {
        active.w[j] = ctl[CL_ACTIVE + (l % CL_RING) * B + j];
        cols.w[j] = 0;
    }
    unsigned int rows = 0, slots = 0, pairs = 0;
    const int lane = threadIdx.x & 63;
    const unsigned int n = (unsigned int) ctl[CL_LONGN + l % CL_RING], nwaves = gridDim.x * (BFS_THREADS >> 6);
    for (unsigned int k = blockIdx.x * (BFS_THREADS >> 6) + (threadIdx.x >> 6); k < n; k += nwaves) {   // (wave-uniform)
        const int64_t v = list[k];
        const cl_vec<B> s = seen[v];
        cl_vec<B> unseen, acc;
#pragma unroll
        for (int j = 0; j < B; j++) {
            unseen.w[j] = active.w[j] & ~s.w[j];
            acc.w[j] = 0;
        }
        unsigned int walked = 0;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int32_t* __restrict__ bg = r ? begin1 : begin0;
            const int32_t* __restrict__ idx = r ? idx1 : idx0;
            const int32_t rb = bg[v], re = bg[v + 1];
            int32_t base = rb;
            while (base < re && !cl_covers<B>(acc, unseen)) {
                cl_vec<B> f[CL_LONG_UNROLL];
#pragma unroll
                for (int j = 0; j < CL_LONG_UNROLL; j++) {
                    const int32_t e = base + 64 * j + lane;
                    if (e < re) {
                        f[j] = front[idx[e]];
                    } else {
#pragma unroll
                        for (int q = 0; q < B; q++) f[j].w[q] = 0;
                    }
                }
#pragma unroll
                for (int q = 0; q < B; q++) {
                    uint64_t x = acc.w[q];
#pragma unroll
                    for (int j = 0; j < CL_LONG_UNROLL; j++) x |= f[j].w[q];
                    acc.w[q] = cl_wave_or(x);
                }
                base = re - base > 64 * CL_LONG_UNROLL ? base + 64 * CL_LONG_UNROLL : re;
            }
            walked += (unsigned int) (base - rb);
        }
        if (lane == 0) {
            cl_vec<B> nw;
#pragma unroll
            for (int j = 0; j < B; j++) {
                nw.w[j] = acc.w[j] & unseen.w[j];
                cols.w[j] |= nw.w[j];
            }
            pairs += cl_settle<B>(v, s, nw, l, r_of_l, seen, next, far, reach, ecc, harm);
            slots += walked;
            rows++;
        }
    }
    cl_tally<B>(s_t, ctl, l, 0, rows, 0, slots, pairs, cols);
}

// ---------------------------------------------------------------- host side
struct cl_call {
    gmx_graph* g;
    int mode;
    const int32_t* sources_dev;   // NULL: every vertex
    int64_t nsources;
    int32_t long_min, batch;      // batch: levels launched per host read
    int long_grid;                // 0: no row can be listed, the wave kernel is never launched
    uint64_t* state;              // seen, front, next: [3][V][B]
    int64_t* far;
    int32_t *reach, *ecc, *long_list;
    uint64_t* harm;
    unsigned long long* ctl;
    gmx_pinned<unsigned long long>* h_word;
    int64_t sweeps, levels, pairs;
};

template <int B, int NR>
static int cl_run(cl_call& c) {
    const gmx_graph* g = c.g;
    const int64_t V = g->V;
    const bool fwd = c.mode != GMX_CLOSE_IN;   // row 0: the forward row for OUT and BOTH
    const int32_t* begin0 = fwd ? g->begin.p : g->r_begin.p;
    const int32_t* idx0 = fwd ? g->node_idx.p : g->r_node_idx.p;
    const int32_t* begin1 = NR == 2 ? g->r_begin.p : nullptr;
    const int32_t* idx1 = NR == 2 ? g->r_node_idx.p : nullptr;
    const int level_grid = grid_for(V, BFS_THREADS, 256 * 8);
    const size_t plane = (size_t) V * B;
    for (int64_t first = 0; first < c.nsources; first += 64 * B) {
        const int32_t nb = (int32_t) (c.nsources - first < 64 * B ? c.nsources - first : 64 * B);
        uint64_t* seen = c.state;
        uint64_t* front = c.state + plane;
        uint64_t* next = c.state + 2 * plane;
        GMX_HIP(hipMemsetAsync(seen, 0, sizeof(uint64_t) * 2 * plane, 0));   // (next is written whole by every level)
        hipLaunchKernelGGL((close_seed_kernel<B>), dim3(1), dim3(64 * CL_MAX_WORDS), 0, 0, c.sources_dev, first, nb, seen, front, c.ctl);
        c.sweeps++;
        for (int32_t l0 = 1, done = 0; !done; l0 += c.batch) {
            if (l0 > INT32_MAX - c.batch) {
                gmx_set_error("closeness: level overflow");
                return GMX_ERR_STATE;
            }
            for (int32_t l = l0; l < l0 + c.batch; l++) {
                const uint64_t r_of_l = ((uint64_t) 1 << 32) / (uint64_t) l;
                hipLaunchKernelGGL((close_level_kernel<B, NR>), dim3(level_grid), dim3(BFS_THREADS), 0, 0, begin0, idx0, begin1, idx1, V, l, r_of_l, c.long_min,
                                   (cl_vec<B>*) seen, (const cl_vec<B>*) front, (cl_vec<B>*) next, c.far, c.reach, c.ecc, c.harm, c.long_list, c.ctl);
                if (c.long_grid)
                    hipLaunchKernelGGL((close_long_kernel<B, NR>), dim3(c.long_grid), dim3(BFS_THREADS), 0, 0, (const int32_t*) c.long_list, begin0, idx0, begin1, idx1, l,
                                       r_of_l, (cl_vec<B>*) seen, (const cl_vec<B>*) front, (cl_vec<B>*) next, c.far, c.reach, c.ecc, c.harm, c.ctl);
                uint64_t* t = front;
                front = next;
                next = t;
            }
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(*c.h_word, c.ctl + CL_FOUND, CL_RING));   // the batch's new pairs: the one host read of these levels
            c.levels += c.batch;
            for (int32_t l = l0; l < l0 + c.batch && !done; l++) {
                const unsigned long long found = c.h_word->p[l % CL_RING];
                if (!found) done = 1;   // (the levels behind it found every vertex saturated)
                c.pairs += (int64_t) found;
            }
        }
    }
    return GMX_OK;
}

template <int B>
static int cl_run_mode(cl_call& c) {
    return c.mode == GMX_CLOSE_BOTH ? cl_run<B, 2>(c) : cl_run<B, 1>(c);
}

#define CL_DEFAULT_WORDS 4   // GMX_CLOSE_WORDS when the environment does not set it (the measured table)
#define CL_DEFAULT_BATCH 4   // GMX_CLOSE_BATCH likewise
#define CL_DEFAULT_LONG_MIN 128   // GMX_CLOSE_LONG_MIN likewise

extern "C" int gmx_closeness(gmx_graph_t* g, int mode, const gmx_node_t* sources, int32_t nsources, int64_t* far_host, int32_t* reach_host, int32_t* ecc_host,
                             uint64_t* harm_host, gmx_stats_t* stats_out) {
    GMX_REQUIRE(g, "NULL argument");
    GMX_REQUIRE(mode >= GMX_CLOSE_OUT && mode <= GMX_CLOSE_BOTH, "closeness: mode %d is none of GMX_CLOSE_OUT, _IN, _BOTH", mode);
    GMX_REQUIRE(!sources || nsources >= 0, "closeness: nsources %d", nsources);
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    if (mode != GMX_CLOSE_OUT && !g->has_reverse) {
        gmx_set_error("closeness: modes IN and BOTH need the reverse CSR");
        return GMX_ERR_STATE;
    }
    GMX_REQUIRE(V <= INT32_MAX, "too many vertices");
    const int64_t n = sources ? nsources : V;
    if (sources)
        for (int32_t i = 0; i < nsources; i++) GMX_REQUIRE(sources[i] >= 0 && sources[i] < V, "closeness: source %d out of range", sources[i]);
    int B = (int) gmx_env_int("GMX_CLOSE_WORDS", CL_DEFAULT_WORDS, 0, 1 << 20);
    GMX_REQUIRE(B == 1 || B == 2 || B == 4, "GMX_CLOSE_WORDS=%d: 1, 2 or 4", B);
    while (B > 1 && 64 * (B / 2) >= n) B /= 2;   // (no wider than the sources need)
    const bool log = gmx_env_int("GMX_CLOSE_LOG", 0, 0, 1) != 0;

    gmx_ws_scope scope;
    wbuf<uint64_t> state, harm;
    wbuf<int64_t> far;
    wbuf<int32_t> reach, ecc, long_list, sources_dev;
    wbuf<unsigned long long> ctl;
    GMX_CHECK(state.alloc(3 * (size_t) V * B));
    GMX_CHECK(harm.alloc((size_t) V));
    GMX_CHECK(far.alloc((size_t) V));
    GMX_CHECK(reach.alloc((size_t) V));
    GMX_CHECK(ecc.alloc((size_t) V));
    GMX_CHECK(long_list.alloc((size_t) V));
    GMX_CHECK(ctl.alloc(CL_CTL + 1));
    if (sources) GMX_CHECK(sources_dev.alloc((size_t) nsources));
    gmx_pinned<unsigned long long> h_word;
    GMX_CHECK(h_word.alloc(CL_CTL + 1));
    gmx_spans tm;

    cl_call c;
    c.g = g;
    c.mode = mode;
    c.sources_dev = sources ? sources_dev.p : nullptr;
    c.nsources = n;
    c.long_min = (int32_t) gmx_env_int("GMX_CLOSE_LONG_MIN", CL_DEFAULT_LONG_MIN, 1, INT_MAX);
    c.batch = (int32_t) gmx_env_int("GMX_CLOSE_BATCH", CL_DEFAULT_BATCH, 1, CL_RING - 2);
    c.state = state.p;
    c.far = far.p;
    c.reach = reach.p;
    c.ecc = ecc.p;
    c.harm = harm.p;
    c.long_list = long_list.p;
    c.ctl = ctl.p;
    c.h_word = &h_word;
    c.sweeps = c.levels = c.pairs = 0;

    GMX_CHECK(tm.begin(tm.H2D));
    if (sources && nsources) GMX_HIP(hipMemcpyAsync(sources_dev.p, sources, sizeof(int32_t) * (size_t) nsources, hipMemcpyHostToDevice, 0));
    GMX_CHECK(tm.end(tm.H2D));
    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(unsigned long long) * (CL_CTL + 1), 0));
    GMX_HIP(hipMemsetAsync(far.p, 0, sizeof(int64_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(reach.p, 0, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(ecc.p, 0, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(harm.p, 0, sizeof(uint64_t) * (size_t) V, 0));
    // the rows a level can list, for the wave kernel's grid (none: it is never launched)
    hipLaunchKernelGGL(close_count_long_kernel, dim3(grid_for(V)), dim3(BFS_THREADS), 0, 0, (const int32_t*) (mode == GMX_CLOSE_IN ? g->r_begin.p : g->begin.p),
                       (const int32_t*) (mode == GMX_CLOSE_BOTH ? g->r_begin.p : nullptr), V, c.long_min, ctl.p + CL_CTL);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_read_back(h_word, (const unsigned long long*) (ctl.p + CL_CTL)));
    c.long_grid = *h_word.p ? grid_for((int64_t) *h_word.p, BFS_THREADS >> 6, 256 * 8) : 0;

    if (B == 1) GMX_CHECK(cl_run_mode<1>(c));
    else if (B == 2) GMX_CHECK(cl_run_mode<2>(c));
    else GMX_CHECK(cl_run_mode<4>(c));
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    if (far_host) GMX_HIP(hipMemcpyAsync(far_host, far.p, sizeof(int64_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    if (reach_host) GMX_HIP(hipMemcpyAsync(reach_host, reach.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    if (ecc_host) GMX_HIP(hipMemcpyAsync(ecc_host, ecc.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    if (harm_host) GMX_HIP(hipMemcpyAsync(harm_host, harm.p, sizeof(uint64_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    GMX_HIP(hipMemcpyAsync(h_word.p, ctl.p, sizeof(unsigned long long) * CL_CTL, hipMemcpyDeviceToHost, 0));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));   // (the downloads have landed)
    const unsigned long long* h = h_word.p;
    stats->iterations = (int32_t) (c.levels > INT32_MAX ? INT32_MAX : c.levels);
    stats->vertices_reached = c.pairs;
    stats->edges_examined = (int64_t) h[CL_SLOTS];
    if (log)
        fprintf(stderr, "gmx close: V %lld E %lld mode %d sources %lld words %d sweeps %lld levels %lld lane %llu wave %llu saturated %llu slots %llu pairs %lld\n",
                (long long) V, (long long) g->E, mode, (long long) n, B, (long long) c.sweeps, (long long) c.levels, h[CL_LANE], h[CL_WAVE], h[CL_SAT], h[CL_SLOTS],
                (long long) c.pairs);
    return GMX_OK;
}

void gmx_touch_close() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) close_count_long_kernel);
}
