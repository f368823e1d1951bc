// gmx_tcd.hip -- triangle_counting_directed for gfx950.
//
// Replaces the body of apps/src/triangle_counting_directed.gm:
//     Foreach(v) Foreach(u: v.Nbrs) Foreach(w: v.Nbrs)(w > u)
//         If (w.HasEdgeFrom(u) || w.HasEdgeTo(u)) T++;
// With adj(u, w) = (u -> w in E or w -> u in E):
//     T = sum over v of #{ ordered slot pairs (i, j) of row v : node_idx[i] < node_idx[j], adj(node_idx[i], node_idx[j]) }
// Repeated slots of row v count multiply, the adjacency test is boolean (set membership, whatever the row order), self
// loops take part literally (gmx.h).  `w > u` only picks every unordered pair of distinct VALUES of a row once, so T does
// not depend on the vertex numbering, and the count runs on a renumbered copy.
//
// Plan (graph preprocessing: built on first use from the forward CSR alone, cached on the graph, outside kernel_ms; the struct is
// in gmx_tcd_plan.h because gmx_clustering, gmx_ktruss, gmx_kclique and gmx_squares share the plan and keep their additions with
// it; they get it through tcd_plan_get, ask tcd_real_slots whether there is an edge at all, scan their groups with
// tcd_group_offsets and sort their lists with tcd_sort_by_key; the symmetric adjacency that gmx_ktruss and gmx_squares walk
// is built here as well, by tcd_plan_adjacency):
//   N      the undirected simple neighbourhood: keys (s,d) and (d,s) of every slot with s != d, sorted, repeats dropped;
//   perm   ascending |N(x)| (stable: ties by id), or the identity with GMX_TCD_NO_ORDER=1;
//   OUT'   the forward rows renumbered and sorted, repeats and self loops kept (E entries);
//   UP'    per vertex x the distinct y > x with adj(x, y), sorted (half of N's entries);
//   groups exclusive scan of the 64-slot groups of the OUT' rows: a row of d >= 2 slots has ceil((d - 1) / 64) of them
//          (its last slot has nothing above it).
// Count: a work item is (v, group of 64 slots of OUT'(v)), claimed from a counter (the loop, the staging and the searches are
// gmx_rowgroup.h's).  The row from the group's first slot on
// is staged in the wave's LDS slice (at most `cap` entries; longer ones are searched in memory).  Lane i owns the slot
// u = A[i]; its tail is A from the first position with a value > u (the run of equal values is skipped), the other side is
// UP'(u).  With the degree order UP'(u) is short for a low-degree u and hubs own almost nothing.  A side of at most
// `alone` entries is walked by the lane itself; the other slots are taken one after the other by the whole wave, which
// streams UP'(u) in coalesced pieces and binary-searches the tail while |UP'(u)| <= ratio * |tail|, and streams the tail
// and searches UP'(u) in memory otherwise.
// Multiplicity: walking UP'(u) (distinct values), every w found adds its RUN LENGTH in the tail; walking the tail, every
// slot adds one.  Both give the number of tail slots whose value is in UP'(u).
// Integer only: exact.  64-bit partials per lane, a shuffle reduction, one atomic add per wave.
#include "gmx_tcd_plan.h"
#include "gmx_rowgroup.h"
#include "gmx_frontier.h"

#include <rocprim/rocprim.hpp>

#define TCD_THREADS 256
#define TCD_WAVES 4
#define TCD_CLAIM 8      // work items per dequeue
#define TCD_PIECES 4     // 256-byte pieces of UP'(u) a wave keeps in flight
// alone, ratio and cap are gmx_tc.hip's TCO_ALONE, TCO_RATIO and TCO_CAP, swept here with tools/tcd_prof.py --sweep on directed
// RMAT-16 and RMAT-20 only; NOT MEASURED: RMAT-22/24, permuted and symmetrised graphs, and TCD_PIECES and
// TCD_CLAIM above, which are taken over unchanged.
#define TCD_ALONE 4      // a lane walks a side of up to this many entries by itself (0 .. 16 flat within the spread; 48: +5 %)
#define TCD_RATIO 4      // stream UP'(u) and search the tail while |UP'(u)| <= TCD_RATIO * |tail| (2 .. 64 flat; 1: +5 %)
#define TCD_CAP 1024     // row entries staged per wave (4 KiB; 4 waves: 16 KiB of LDS per workgroup; 512: +5 %, 256: +10 %)
#define TCD_CAP_MIN 64

enum { TCD_TOTAL, TCD_NEXT, TCD_STAGED, TCD_MEMORY, TCD_SLOT_ALONE, TCD_SLOT_LIST, TCD_SLOT_TAIL, TCD_SLOT_EMPTY, TCD_NCTR };

void gmx_tcd_plan_free(tcd_plan* p) { delete p; }

// ------------------------------------------------------------------ plan kernels
// both orientations of every slot that is no self loop; `none` (row V: sorts last) for the others
__global__ void tcd_pair_keys_kernel(const uint64_t* __restrict__ fwd, int64_t E, uint64_t none, uint64_t* __restrict__ out) {
    int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; e < E; e += stride) {
        const uint64_t k = fwd[e];
        const uint64_t s = k >> 32, d = k & 0xffffffffu;
        out[2 * e] = s == d ? none : k;
        out[2 * e + 1] = s == d ? none : ((d << 32) | s);
    }
}

// begin[r] = first of the n sorted keys whose row is >= r, r <= V; idx[e] = column of key e, e < nidx
__global__ void tcd_extract_kernel(const uint64_t* __restrict__ keys, int64_t V, int64_t n, int64_t nidx,
                                   int32_t* __restrict__ begin, int32_t* __restrict__ idx) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t e = i; e < nidx; e += stride) idx[e] = (int32_t) (uint32_t) (keys[e] & 0xffffffffu);
    for (int64_t r = i; r <= V; r += stride) {
        const uint64_t target = (uint64_t) r << 32;
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < target) lo = mid + 1; else hi = mid;
        }
        begin[r] = (int32_t) lo;
    }
}

// ascending |N(x)|, as tc_degkey_kernel does it on a CSR; deg[] keeps |N(x)| for gmx_clustering (key NULL: only that)
__global__ void tcd_degkey_kernel(const int32_t* __restrict__ nbegin, int64_t V, uint32_t* __restrict__ key, int32_t* __restrict__ deg) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < V; i += stride) {
        const uint32_t d = (uint32_t) nbegin[i + 1] - (uint32_t) nbegin[i];   // (N has up to 2 E < 2^32 entries: the offsets may wrap, the difference does not)
        deg[i] = (int32_t) d;   // (< V <= 2^31 - 1)
        if (key) key[i] = d;
    }
}

// the keys of N, renumbered (perm NULL: as they are): (x, y) with x < y stays, its mirror becomes `none`
__global__ void tcd_up_keys_kernel(const uint64_t* __restrict__ nkeys, int64_t n, const int32_t* __restrict__ perm, uint64_t none,
                                   uint64_t* __restrict__ out) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const uint64_t k = nkeys[i];
        uint64_t x = k >> 32, y = k & 0xffffffffu;
        if (perm) {
            x = (uint32_t) perm[x];
            y = (uint32_t) perm[y];
        }
        out[i] = x < y ? ((x << 32) | y) : none;
    }
}

// groups[v] = 64-slot groups of a row of d = begin[v + 1] - begin[v] slots: ceil((d - 1) / 64) from d = 2 on
static __global__ void tcd_groups_kernel(const int32_t* __restrict__ begin, int64_t V, int64_t* __restrict__ groups) {
    int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; v < V; v += stride) {
        const int32_t d = begin[v + 1] - begin[v];
        groups[v] = d >= 2 ? (d - 1 + 63) / 64 : 0;
    }
}

// forward slots that are no self loop (is there any edge at all: asked before a plan is built)
static __global__ void __launch_bounds__(TCD_THREADS) tcd_real_slots_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V,
                                                                            int64_t E, unsigned long long* __restrict__ out) {
    unsigned long long n = 0;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (int64_t) gridDim.x * blockDim.x)
        n += idx[i] != csr_row_of(begin, V, (uint32_t) i) ? 1 : 0;
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, n);
}

// ---- the symmetric adjacency (tcd_plan_adjacency)
// begin[r] = the first of the n sorted keys that is >= r, r <= V
__global__ void __launch_bounds__(TCD_THREADS) tcd_down_begin_kernel(const uint32_t* __restrict__ key, int64_t n, int64_t V, int32_t* __restrict__ begin) {
    for (int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; r <= V; r += (int64_t) gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t) key[mid] < r) lo = mid + 1; else hi = mid;
        }
        begin[r] = (int32_t) lo;
    }
}
__global__ void __launch_bounds__(TCD_THREADS) tcd_nb_begin_kernel(const int32_t* __restrict__ down_begin, const int32_t* __restrict__ up_begin, int64_t V,
                                                                   int32_t* __restrict__ nb_begin) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v <= V; v += (int64_t) gridDim.x * blockDim.x) nb_begin[v] = down_begin[v] + up_begin[v];
}
// entry j of the sorted (w, position) pairs is the lower slot (x, w) of row w, x = the row of the position in UP'; the
// position itself is the upper slot of row x.  up_src[position] = x.
__global__ void __launch_bounds__(TCD_THREADS) tcd_fill_kernel(const uint32_t* __restrict__ key, const int32_t* __restrict__ pos_of, int64_t U, int64_t V,
                                                               const int32_t* __restrict__ up_begin, const int32_t* __restrict__ up_idx,
                                                               const int32_t* __restrict__ down_begin, const int32_t* __restrict__ nb_begin,
                                                               int32_t* __restrict__ nb_idx, int32_t* __restrict__ nb_eid, int32_t* __restrict__ up_src) {
    for (int64_t j = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; j < U; j += (int64_t) gridDim.x * blockDim.x) {
        const int32_t w = (int32_t) key[j], pos = pos_of[j];
        const int32_t x = csr_row_of(up_begin, V, (uint32_t) pos);
        const int64_t lower = (int64_t) nb_begin[w] + (j - down_begin[w]);
        nb_idx[lower] = x;
        nb_eid[lower] = pos;
        const int64_t upper = (int64_t) nb_begin[x] + (down_begin[x + 1] - down_begin[x]) + (pos - up_begin[x]);
        nb_idx[upper] = w;   // (= up_idx[pos])
        nb_eid[upper] = pos;
        up_src[pos] = x;
    }
}

// ------------------------------------------------------------------ count kernel
struct tcd_tally {   // what GMX_TCD_LOG reports: counted where the decisions are taken
    unsigned long long c = 0;          // per lane
    unsigned int alone = 0, empty = 0; // per lane
    unsigned int list = 0, tail = 0;   // per wave (the same in every lane)
};

// One work item: R[0, da) is OUT'(v) from the group's first slot on (the wave's LDS slice or the row in memory), the
// group's slots are R[0 .. 63], one per lane; slot i pairs with the entries above its value.
template <bool LDS>
__device__ __forceinline__ void tcd_item(const int32_t* R, int32_t da, const int32_t* __restrict__ up_begin,
                                         const int32_t* __restrict__ up_idx, int lane, int alone_max, int ratio, tcd_tally& t) {
    const bool act = lane + 1 < da;
    int32_t bb = 0, be = 0, ts = da;
    if (act) {
        const int32_t u = R[lane];
        ts = rg_lower_bound<LDS>(R, lane + 1, da, u + 1);
        bb = up_begin[u];
        be = up_begin[u + 1];
    }
    const int32_t db = be - bb, ta = da - ts;
    const bool tail_side = ta < db;                     // the side to walk: the shorter one
    const int32_t shorter = db == 0 || ta == 0 ? 0 : (tail_side ? ta : db);
    if (act && shorter == 0) t.empty++;
    if (act && shorter > 0 && shorter <= alone_max) {
        t.alone++;
        if (tail_side) {
            for (int32_t p = ts; p < da; p++) t.c += rg_contains<false>(up_idx, bb, be, R[p]) ? 1 : 0;
        } else {
            for (int32_t p = bb; p < be; p++) t.c += (unsigned long long) rg_run<LDS>(R, ts, da, up_idx[p]);
        }
    }
    unsigned long long m = __ballot(act && shorter > alone_max);
    while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        const int32_t sbb = __shfl(bb, src, 64), sbe = __shfl(be, src, 64), sts = __shfl(ts, src, 64);
        const int32_t sdb = sbe - sbb, sta = da - sts;
        if ((long long) sdb <= (long long) ratio * sta) {    // stream UP'(u), search the tail
            t.list++;
            for (int32_t p = sbb + lane; p < sbe; p += TCD_PIECES * 64) {
                int32_t w[TCD_PIECES];
#pragma unroll
                for (int k = 0; k < TCD_PIECES; k++) w[k] = p + 64 * k < sbe ? up_idx[p + 64 * k] : -1;
#pragma unroll
                for (int k = 0; k < TCD_PIECES; k++) {
                    if (w[k] < 0) continue;
                    t.c += (unsigned long long) rg_run<LDS>(R, sts, da, w[k]);
                }
            }
        } else {                                             // stream the tail, search UP'(u) in memory
            t.tail++;
            for (int32_t p = sts + lane; p < da; p += 64) t.c += rg_contains<false>(up_idx, sbb, sbe, R[p]) ? 1 : 0;
        }
    }
}

__global__ void __launch_bounds__(TCD_WAVES * 64)
tcd_count_kernel(const int32_t* __restrict__ out_begin, const int32_t* __restrict__ out_idx, const int32_t* __restrict__ up_begin,
                 const int32_t* __restrict__ up_idx, const int64_t* __restrict__ grp_off, int64_t V, int part, int nparts,
                 int cap /* <= TCD_CAP */, int alone_max, int ratio, unsigned long long* __restrict__ ctr /* [TCD_NCTR] */) {
    __shared__ int32_t s_row[TCD_WAVES][TCD_CAP];
    const int lane = threadIdx.x & 63;
    int32_t* A = s_row[threadIdx.x >> 6];
    tcd_tally t;
    unsigned int staged = 0, in_memory = 0;
    rg_items<TCD_CLAIM>(
        grp_off, V, part, nparts, &ctr[TCD_NEXT], lane,
        [&](int32_t v, int32_t group) {
            const int32_t ab = out_begin[v] + group * 64, ae = out_begin[v + 1];
            const int32_t da = ae - ab;                 // OUT'(v) from the group's first slot on (>= 2)
            if (da <= cap) {
                rg_stage(A, out_idx + ab, da, lane);
                staged++;
                tcd_item<true>(A, da, up_begin, up_idx, lane, alone_max, ratio, t);
                rg_slice_done();
            } else {
                in_memory++;
                tcd_item<false>(out_idx + ab, da, up_begin, up_idx, lane, alone_max, ratio, t);
            }
        });
    unsigned long long c = t.c, na = t.alone, ne = t.empty;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c += __shfl_down(c, off, 64);
        na += __shfl_down(na, off, 64);
        ne += __shfl_down(ne, off, 64);
    }
    if (lane == 0) {
        if (c) atomicAdd(&ctr[TCD_TOTAL], c);
        if (staged) atomicAdd(&ctr[TCD_STAGED], (unsigned long long) staged);
        if (in_memory) atomicAdd(&ctr[TCD_MEMORY], (unsigned long long) in_memory);
        if (na) atomicAdd(&ctr[TCD_SLOT_ALONE], na);
        if (t.list) atomicAdd(&ctr[TCD_SLOT_LIST], (unsigned long long) t.list);
        if (t.tail) atomicAdd(&ctr[TCD_SLOT_TAIL], (unsigned long long) t.tail);
        if (ne) atomicAdd(&ctr[TCD_SLOT_EMPTY], ne);
    }
}

// ------------------------------------------------------------------ host
// sorts n keys (bits [0, end_bit)) between the two buffers; *sorted = the buffer that holds them, *other = the free one
static int tcd_sort_keys(uint64_t* a, uint64_t* b, int64_t n, unsigned end_bit, hipStream_t s, uint64_t** sorted, uint64_t** other) {
    *sorted = a;
    *other = b;
    if (n < 2) return GMX_OK;
    rocprim::double_buffer<uint64_t> db(a, b);
    size_t tb = 0;
    GMX_HIP(rocprim::radix_sort_keys(nullptr, tb, db, (size_t) n, 0u, end_bit, s));
    wbuf<char> tmp;
    GMX_CHECK(tmp.alloc(tb));
    GMX_HIP(rocprim::radix_sort_keys((void*) tmp.p, tb, db, (size_t) n, 0u, end_bit, s));
    GMX_HIP(hipStreamSynchronize(s));
    *sorted = db.current();
    *other = db.alternate();
    return GMX_OK;
}

int tcd_sort_by_key(const uint32_t* key, uint32_t* key_sorted, int32_t* val_sorted, int64_t n, unsigned end_bit, hipStream_t s, size_t* tmp_bytes) {
    if (tmp_bytes) *tmp_bytes = 0;
    wbuf<int32_t> val;
    wbuf<char> tmp;
    GMX_CHECK(val.alloc((size_t) n));
    hipLaunchKernelGGL(iota_kernel, dim3(grid_for(n)), dim3(TCD_THREADS), 0, s, val.p, n);
    GMX_HIP(hipGetLastError());
    size_t tb = 0;
    GMX_HIP(rocprim::radix_sort_pairs(nullptr, tb, key, key_sorted, val.p, val_sorted, (size_t) n, 0u, end_bit, s));
    if (tmp_bytes) *tmp_bytes = tb;
    GMX_CHECK(tmp.alloc(tb));
    GMX_HIP(rocprim::radix_sort_pairs((void*) tmp.p, tb, key, key_sorted, val.p, val_sorted, (size_t) n, 0u, end_bit, s));
    return GMX_OK;
}

template <template <typename> class Buf>
int tcd_group_offsets(const int32_t* begin, int64_t V, dbuf<int64_t>* grp_off, hipStream_t s) {
    Buf<int64_t> groups;
    Buf<char> tmp;
    GMX_CHECK(groups.alloc((size_t) V + 1));
    GMX_CHECK(grp_off->alloc((size_t) V + 1));
    GMX_HIP(hipMemsetAsync(groups.p + V, 0, sizeof(int64_t), s));
    hipLaunchKernelGGL(tcd_groups_kernel, dim3(grid_for(V, TCD_THREADS, 256 * 16)), dim3(TCD_THREADS), 0, s, begin, V, groups.p);
    GMX_HIP(hipGetLastError());
    size_t tb = 0;
    GMX_HIP(rocprim::exclusive_scan(nullptr, tb, groups.p, grp_off->p, (int64_t) 0, (size_t) V + 1, rocprim::plus<int64_t>(), s));
    GMX_CHECK(tmp.alloc(tb));
    GMX_HIP(rocprim::exclusive_scan((void*) tmp.p, tb, groups.p, grp_off->p, (int64_t) 0, (size_t) V + 1, rocprim::plus<int64_t>(), s));
    GMX_HIP(hipStreamSynchronize(s));
    return GMX_OK;
}
// the two forms the header promises: both are instantiated here, whoever calls them
template int tcd_group_offsets<wbuf>(const int32_t*, int64_t, dbuf<int64_t>*, hipStream_t);   // tcd_build_plan below
template int tcd_group_offsets<dbuf>(const int32_t*, int64_t, dbuf<int64_t>*, hipStream_t);   // gmx_lcc.hip's lcc_prepare

// builds the plan of g; the caller owns *out (gmx_tcd_plan_free)
static int tcd_build_plan(const gmx_graph* g, bool ordered, tcd_plan** out) {
    const int64_t V = g->V, E = g->E;
    hipStream_t s = 0;
    gmx_tick tick("tcd plan");
    const double t0 = gmx_tick::now();
    tcd_plan* p = new tcd_plan();
    struct guard {
        tcd_plan* p;
        ~guard() { delete p; }
    } gd{p};
    p->V = V;
    p->E = E;
    p->ordered = ordered;
    gmx_ws_scope scope;
    // the transient keys: 2 E of 64 bits, double-buffered
    wbuf<uint64_t> ka, kb;
    const size_t key_bytes = 2 * (size_t) (2 * E) * sizeof(uint64_t);
    if (ka.alloc((size_t) (2 * E)) || kb.alloc((size_t) (2 * E))) {
        const std::string why = gmx_last_error();
        gmx_set_error("triangle_counting_directed: the plan's key buffers need %zu bytes (2 x %lld 64-bit keys): %s", key_bytes,
                      (long long) (2 * E), why.c_str());
        return GMX_ERR_NOMEM;
    }
    const uint64_t none = (uint64_t) V << 32;
    const unsigned end_bit = 32 + (unsigned) gmx_bits_for(V + 1);
    // N: both orientations, sorted, repeats dropped
    GMX_CHECK(gmx_keys_from_csr(g->begin.p, g->node_idx.p, V, E, false, nullptr, kb.p, s));
    hipLaunchKernelGGL(tcd_pair_keys_kernel, dim3(grid_for(E, TCD_THREADS, 256 * 16)), dim3(TCD_THREADS), 0, s, (const uint64_t*) kb.p, E, none, ka.p);
    GMX_HIP(hipGetLastError());
    uint64_t *cur = nullptr, *oth = nullptr;
    GMX_CHECK(tcd_sort_keys(ka.p, kb.p, 2 * E, end_bit, s, &cur, &oth));
    int64_t n = 0;
    {
        wbuf<int64_t> count;
        wbuf<char> tmp;
        GMX_CHECK(count.alloc(1));
        size_t ub = 0;
        GMX_HIP(rocprim::unique(nullptr, ub, (const uint64_t*) cur, oth, count.p, (size_t) (2 * E), rocprim::equal_to<uint64_t>(), s));
        GMX_CHECK(tmp.alloc(ub));
        GMX_HIP(rocprim::unique((void*) tmp.p, ub, (const uint64_t*) cur, oth, count.p, (size_t) (2 * E), rocprim::equal_to<uint64_t>(), s));
        GMX_HIP(hipMemcpy(&n, count.p, sizeof(int64_t), hipMemcpyDeviceToHost));
        uint64_t last = 0;   // the self loops' key, if present, is the last one
        if (n > 0) GMX_HIP(hipMemcpy(&last, oth + (n - 1), sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (n > 0 && last == none) n--;
    }
    uint64_t* nkeys = oth;   // n keys of N; `cur` is free
    tick.mark("N");
    // |N(x)| (kept on the plan: gmx_clustering's deg) and perm: ascending |N(x)| (kept: gmx_clustering maps its arrays back through it)
    dbuf<int32_t>& perm = p->perm;
    GMX_CHECK(p->deg.alloc((size_t) V));
    {
        wbuf<int32_t> nbegin, order;
        wbuf<uint32_t> key, key2;
        GMX_CHECK(nbegin.alloc((size_t) V + 1));
        if (ordered) {
            GMX_CHECK(order.alloc((size_t) V));
            GMX_CHECK(key.alloc((size_t) V));
            GMX_CHECK(key2.alloc((size_t) V));
            GMX_CHECK(perm.alloc((size_t) V));
        }
        hipLaunchKernelGGL(tcd_extract_kernel, dim3(grid_for(V + 1, TCD_THREADS, 256 * 16)), dim3(TCD_THREADS), 0, s, (const uint64_t*) nkeys, V, n, (int64_t) 0, nbegin.p,
                           (int32_t*) nullptr);
        hipLaunchKernelGGL(tcd_degkey_kernel, dim3(grid_for(V, TCD_THREADS, 256 * 16)), dim3(TCD_THREADS), 0, s, (const int32_t*) nbegin.p, V, key.p, p->deg.p);
        GMX_HIP(hipGetLastError());
        if (ordered) {
            GMX_CHECK(tcd_sort_by_key(key.p, key2.p, order.p, V, 32u, s));
            hipLaunchKernelGGL(tc_invert_kernel, dim3(grid_for(V, TCD_THREADS, 256 * 16)), dim3(TCD_THREADS), 0, s, (const int32_t*) order.p, V, perm.p);
            GMX_HIP(hipGetLastError());
        }
    }
    tick.mark("perm");
    // UP': the half of N's keys that points upwards in the new numbering
    p->E_up = n / 2;
    GMX_CHECK(p->up_begin.alloc((size_t) V + 1));
    GMX_CHECK(p->up_idx.alloc((size_t) p->E_up));
    if (n > 0) {
        hipLaunchKernelGGL(tcd_up_keys_kernel, dim3(grid_for(n, TCD_THREADS, 256 * 16)), dim3(TCD_THREADS), 0, s, (const uint64_t*) nkeys, n, (const int32_t*) perm.p, none, cur);
        GMX_HIP(hipGetLastError());
    }
    uint64_t *up_sorted = nullptr, *up_free = nullptr;
    GMX_CHECK(tcd_sort_keys(cur, nkeys, n, end_bit, s, &up_sorted, &up_free));
    hipLaunchKernelGGL(tcd_extract_kernel, dim3(grid_for(p->E_up > V ? p->E_up : V + 1, TCD_THREADS, 256 * 16)), dim3(TCD_THREADS), 0, s, (const uint64_t*) up_sorted, V, n,
                       p->E_up, p->up_begin.p, p->up_idx.p);
    GMX_HIP(hipGetLastError());
    GMX_HIP(hipStreamSynchronize(s));
    tick.mark("UP'");
    // OUT': the forward rows renumbered and sorted
    GMX_CHECK(p->out_begin.alloc((size_t) V + 1));
    GMX_CHECK(p->out_idx.alloc((size_t) E));
    GMX_CHECK(gmx_keys_from_csr(g->begin.p, g->node_idx.p, V, E, false, perm.p, ka.p, s));
    GMX_CHECK(gmx_csr_from_keys(ka.p, kb.p, V, E, p->out_begin.p, p->out_idx.p, s));
    tick.mark("OUT'");
    // the work items
    GMX_CHECK(tcd_group_offsets<wbuf>(p->out_begin.p, V, &p->grp_off, s));
    tick.mark("groups");
    p->build_ms = (gmx_tick::now() - t0) * 1e3;
    gd.p = nullptr;
    *out = p;
    return GMX_OK;
}

int tcd_plan_get(gmx_graph* g, bool ordered, tcd_plan** out, bool* built) {
    *built = false;
    if (g->tcd_cache && g->tcd_cache->ordered != ordered) {
        gmx_tcd_plan_free(g->tcd_cache);
        g->tcd_cache = nullptr;
    }
    if (!g->tcd_cache) {
        GMX_CHECK(tcd_build_plan(g, ordered, &g->tcd_cache));
        *built = true;
    }
    *out = g->tcd_cache;
    return GMX_OK;
}

int tcd_real_slots(const gmx_graph* g, int64_t* real) {
    *real = 0;
    if (g->tcd_cache) *real = g->tcd_cache->E_up;
    else if (g->E > 0) {
        dbuf<unsigned long long> cnt;
        GMX_CHECK(cnt.alloc(1));
        GMX_HIP(hipMemset(cnt.p, 0, sizeof(unsigned long long)));
        hipLaunchKernelGGL(tcd_real_slots_kernel, dim3(grid_for(g->E)), dim3(TCD_THREADS), 0, 0, (const int32_t*) g->begin.p, (const int32_t*) g->node_idx.p,
                           g->V, g->E, cnt.p);
        GMX_HIP(hipGetLastError());
        unsigned long long h = 0;
        GMX_HIP(hipMemcpy(&h, cnt.p, sizeof(h), hipMemcpyDeviceToHost));
        *real = (int64_t) h;
    }
    return GMX_OK;
}

// the plan's additions for gmx_ktruss and gmx_squares, once per plan (the error texts name the entry that had them first)
int tcd_plan_adjacency(tcd_plan* p) {
    if (p->kt_ready) return GMX_OK;
    const int64_t V = p->V, U = p->E_up;
    GMX_REQUIRE(2 * U <= INT32_MAX, "ktruss: %lld undirected edges: the symmetric adjacency needs 32-bit offsets", (long long) U);
    const size_t bytes = ((size_t) V + 1 + 5 * (size_t) U) * sizeof(int32_t);
    if (p->nb_begin.alloc((size_t) V + 1) || p->nb_idx.alloc(2 * (size_t) U) || p->nb_eid.alloc(2 * (size_t) U) || p->up_src.alloc((size_t) U)) {
        const std::string why = gmx_last_error();
        p->nb_begin.release();
        p->nb_idx.release();
        p->nb_eid.release();
        p->up_src.release();
        gmx_set_error("ktruss: the symmetric adjacency of %lld edges needs %zu bytes: %s", (long long) U, bytes, why.c_str());
        return GMX_ERR_NOMEM;
    }
    hipStream_t s = 0;
    gmx_ws_scope scope;
    wbuf<uint32_t> key, key2;
    wbuf<int32_t> pos2, down_begin;
    GMX_CHECK(key.alloc((size_t) U));
    GMX_CHECK(key2.alloc((size_t) U));
    GMX_CHECK(pos2.alloc((size_t) U));
    GMX_CHECK(down_begin.alloc((size_t) V + 1));
    if (U > 0) {
        GMX_HIP(hipMemcpyAsync(key.p, p->up_idx.p, (size_t) U * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        GMX_CHECK(tcd_sort_by_key(key.p, key2.p, pos2.p, U, (unsigned) gmx_bits_for(V), s));
    }
    const uint32_t* sorted = key2.p;   // (U == 0: nobody reads it)
    hipLaunchKernelGGL(tcd_down_begin_kernel, dim3(grid_for(V + 1)), dim3(TCD_THREADS), 0, s, sorted, U, V, down_begin.p);
    hipLaunchKernelGGL(tcd_nb_begin_kernel, dim3(grid_for(V + 1)), dim3(TCD_THREADS), 0, s, (const int32_t*) down_begin.p, (const int32_t*) p->up_begin.p, V,
                       p->nb_begin.p);
    if (U > 0)
        hipLaunchKernelGGL(tcd_fill_kernel, dim3(grid_for(U)), dim3(TCD_THREADS), 0, s, sorted, (const int32_t*) pos2.p, U, V, (const int32_t*) p->up_begin.p,
                           (const int32_t*) p->up_idx.p, (const int32_t*) down_begin.p, (const int32_t*) p->nb_begin.p, p->nb_idx.p, p->nb_eid.p, p->up_src.p);
    GMX_HIP(hipGetLastError());
    GMX_HIP(hipStreamSynchronize(s));
    p->kt_ready = true;
    return GMX_OK;
}

static int tcd_count_part(gmx_graph_t* g, int part, int nparts, int64_t* count, gmx_stats_t* stats) {
    GMX_REQUIRE(g && count, "NULL argument");
    GMX_REQUIRE(nparts >= 1 && part >= 0 && part < nparts, "bad part %d / nparts %d", part, nparts);
    if (stats) memset(stats, 0, sizeof(*stats));
    *count = 0;
    if (g->V == 0 || g->E == 0) return GMX_OK;
    // knobs, read at every call; the count does not depend on them
    const bool ordered = !getenv("GMX_TCD_NO_ORDER");
    const int cap = (int) gmx_env_int("GMX_TCD_CAP", TCD_CAP, TCD_CAP_MIN, TCD_CAP);
    const int alone = (int) gmx_env_int("GMX_TCD_ALONE", TCD_ALONE, 0, INT32_MAX);
    const int ratio = (int) gmx_env_int("GMX_TCD_RATIO", TCD_RATIO, 0, INT32_MAX);
    // graph preprocessing (cached on the graph like the reverse CSR; outside the timed region)
    bool built = false;
    tcd_plan* p = nullptr;
    GMX_CHECK(tcd_plan_get(g, ordered, &p, &built));
    dbuf<unsigned long long> ctr;
    GMX_CHECK(ctr.alloc(TCD_NCTR));
    GMX_HIP(hipMemset(ctr.p, 0, TCD_NCTR * sizeof(unsigned long long)));
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.KERNEL));
    hipLaunchKernelGGL(tcd_count_kernel, dim3(256 * 8), dim3(TCD_WAVES * 64), 0, 0, (const int32_t*) p->out_begin.p, (const int32_t*) p->out_idx.p,
                       (const int32_t*) p->up_begin.p, (const int32_t*) p->up_idx.p, (const int64_t*) p->grp_off.p, p->V, part, nparts, cap, alone,
                       ratio, ctr.p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.finish(stats));
    unsigned long long h[TCD_NCTR];
    GMX_HIP(hipMemcpy(h, ctr.p, sizeof(h), hipMemcpyDeviceToHost));
    *count = (int64_t) h[TCD_TOTAL];
    if (stats) stats->iterations = 1;
    if (getenv("GMX_TCD_LOG"))   // one line per call (tools/tcd_prof.py and the tests parse it)
        fprintf(stderr, "gmx triangle_counting_directed: plan V %lld out %lld up %lld order %s built %d build_ms %.3f; part %d/%d cap %d alone %d "
                        "ratio %d; items %llu staged + %llu memory; slots %llu alone + %llu list + %llu tail + %llu empty\n",
                (long long) p->V, (long long) p->E, (long long) p->E_up, p->ordered ? "degree" : "identity", built ? 1 : 0, built ? p->build_ms : 0.0,
                part, nparts, cap, alone, ratio, h[TCD_STAGED], h[TCD_MEMORY], h[TCD_SLOT_ALONE], h[TCD_SLOT_LIST], h[TCD_SLOT_TAIL], h[TCD_SLOT_EMPTY]);
    return GMX_OK;
}

extern "C" int gmx_triangle_counting_directed(gmx_graph_t* g, int64_t* count, gmx_stats_t* stats) {
    return tcd_count_part(g, 0, 1, count, stats);
}

extern "C" int gmx_triangle_counting_directed_part(gmx_graph_t* g, int part, int nparts, int64_t* count, gmx_stats_t* stats) {
    return tcd_count_part(g, part, nparts, count, stats);
}

void gmx_touch_tcd() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) tcd_count_kernel);
}
