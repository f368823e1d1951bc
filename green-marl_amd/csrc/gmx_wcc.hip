// gmx_wcc.hip -- weakly connected components on gfx950: the Afforest scheme (Sutton, Ben-Nun, Barak, IPDPS'18) on a
// directed CSR.  The reference has no such program; the result follows gmx_scc's conventions (gmx.h).
//
// One array parent[V] with parent[x] <= x: a forest whose trees only ever merge, the larger root hooked under the smaller,
// so that in the end every component's root is its smallest vertex.
//   sampling   K rounds (GMX_WCC_SAMPLE_ROUNDS, default 2): round r links every vertex that has an out-slot r with that
//              neighbour, one thread per vertex; compress (between the rounds and after them) makes every parent[v] the
//              root of v.
//   giant      parent[] is probed at WCC_PROBES fixed positions and the most frequent root g* (ties: the smallest) names
//              the tree that the final pass skips.  GMX_WCC_GIANT=<vertex> forces g* = that vertex's root (for tests: the
//              result does not depend on which tree is skipped).
//   live list  the vertices outside g*'s tree, counted and -- those that have a slot -- compacted BEFORE any link of the
//              final pass runs: the live set is the complement of g*'s tree in the sampled forest whatever the order of
//              the links.
//   final      with the reverse CSR (and GMX_WCC_SKIP != 0) the whole out-rows and the whole in-rows of the live vertices
//              are linked slot by slot: an edge with both ends in g*'s tree needs nothing, every other edge has a live end
//              whose out-row or in-row holds it.  Without the reverse CSR (or with GMX_WCC_SKIP=0) every vertex is live
//              and only the out-rows are walked.  The rows go through the merge-path tile (gmx_frontier.h), so a
//              workgroup's work is BFS_ITEMS items however long a live hub's row is.
//   finish     compress, flag the roots, exclusive scan of the flags = the rank of every root, comp[v] = rank[parent[v]],
//              and the largest component from a histogram by root (g*'s tree counted apart, in sharded counters).
// Host round trips: the length of the live list (skipping form only), the slots of its rows, the results.
#include "gmx_frontier.h"

#include <rocprim/rocprim.hpp>

#define WCC_THREADS BFS_THREADS
#define WCC_PROBES 1024
#define WCC_MAX_ROUNDS 8

struct wcc_ctl {
    unsigned long long live;    // live vertices
    unsigned long long listed;  // tail of the list: the live vertices that have a slot
    int32_t gstar;              // root of the skipped tree (in the sampled forest)
    int32_t count;              // components
    unsigned int largest;       // the largest component outside g*'s tree
    unsigned int pad0;
    unsigned long long pad1[12];
    struct {
        unsigned long long sampled;   // slots read by the sampling rounds
        unsigned long long giant;     // vertices of the component that holds g*
        unsigned long long pad[14];
    } shard[BFS_SHARDS];
};

__global__ void __launch_bounds__(WCC_THREADS) wcc_init_kernel(int32_t* __restrict__ parent, int64_t V) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) parent[v] = (int32_t) v;
}

// round r: every vertex with an out-slot r links itself with it (begin[] coalesced, one slot per vertex)
__global__ void __launch_bounds__(WCC_THREADS) wcc_sample_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx, int64_t V, int32_t r,
                                                                 int32_t* __restrict__ parent, wcc_ctl* __restrict__ ctl) {
    unsigned long long slots = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const int32_t b = begin[v], e = begin[v + 1];
        if (e - b > r) {
            const int32_t w = idx[(int64_t) b + r];
            slots++;
            wcc_hook(parent, parent[v], parent[w]);
        }
    }
    slots = wave_sum(slots);
    if ((threadIdx.x & 63) == 0 && slots) {
        const int sh = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (BFS_SHARDS - 1);
        atomicAdd(&ctl->shard[sh].sampled, slots);
    }
}

// parent[v] = the root of v.  Roots stay roots while this runs, so the walk ends at a true root whatever it reads on the
// way; every vertex it passes is pointed at its grandparent (atomicMin: ancestors descend towards the root, so no late
// write undoes a better one), which halves a long chain for everybody behind.  The loads are agent-scope so that this
// shortening is seen across XCDs: the chain of a path graph is V deep.
__global__ void __launch_bounds__(WCC_THREADS) wcc_compress_kernel(int32_t* __restrict__ parent, int64_t V) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        int32_t x = (int32_t) v, p = wcc_load(&parent[x]);
        if (p == x) continue;
        for (;;) {
            const int32_t gp = wcc_load(&parent[p]);
            if (gp == p) break;
            atomicMin(&parent[x], gp);
            x = p;
            p = gp;
        }
        atomicMin(&parent[v], p);
    }
}

// g* = the most frequent root among the probes (ties: the smallest root), or the root of `forced`.  One workgroup.
__global__ void __launch_bounds__(WCC_PROBES) wcc_giant_kernel(const int32_t* __restrict__ parent, int64_t V, int32_t forced, wcc_ctl* __restrict__ ctl) {
    __shared__ int32_t s_root[WCC_PROBES];
    __shared__ unsigned long long s_best;
    const int tid = threadIdx.x;
    const int np = V < WCC_PROBES ? (int) V : WCC_PROBES;
    if (tid == 0) s_best = 0;
    if (tid < np) s_root[tid] = parent[V <= WCC_PROBES ? (int64_t) tid : (int64_t) (((uint32_t) tid * 0x9E3779B1u) % (uint32_t) V)];
    __syncthreads();
    if (tid < np) {
        const int32_t mine = s_root[tid];
        unsigned int c = 0;
        for (int j = 0; j < np; j++) c += s_root[j] == mine ? 1u : 0u;
        atomicMax(&s_best, ((unsigned long long) c << 32) | (unsigned long long) (0xFFFFFFFFu - (uint32_t) mine));
    }
    __syncthreads();
    if (tid == 0) ctl->gstar = forced >= 0 ? parent[forced] : (int32_t) (0xFFFFFFFFu - (uint32_t) s_best);
}

// the live vertices -- outside g*'s tree -- are counted, and those of them that have an out- or an in-slot go to list (all:
// every vertex is live and listed, and the host needs no count): at RMAT-24 7.6 M of the 9.1 M live vertices are isolated,
// and the offsets and the merge path of the final pass are paid per listed row.  A workgroup collects BFS_ITEMS vertices in
// LDS and claims the tail once.
__global__ void __launch_bounds__(WCC_THREADS) wcc_live_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ begin,
                                                               const int32_t* __restrict__ rbegin, int64_t V, int all, wcc_ctl* __restrict__ ctl,
                                                               int32_t* __restrict__ list) {
    __shared__ int32_t s_list[BFS_ITEMS];
    __shared__ unsigned int s_n, s_live;
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const int32_t gs = ctl->gstar;
    for (int64_t t0 = (int64_t) blockIdx.x * BFS_ITEMS; t0 < V; t0 += (int64_t) gridDim.x * BFS_ITEMS) {
        if (tid == 0) s_n = s_live = 0;
        __syncthreads();
        for (int k = 0; k < BFS_ITEMS / WCC_THREADS; k++) {
            const int64_t v = t0 + k * WCC_THREADS + tid;
            const bool on = v < V && (all || parent[v] != gs);
            const bool rows = on && (all || begin[v + 1] > begin[v] || rbegin[v + 1] > rbegin[v]);
            const unsigned long long mk = __ballot(on);
            if ((tid & 63) == 0 && mk) atomicAdd(&s_live, (unsigned int) __popcll(mk));
            wave_append(rows, (int32_t) v, s_list, &s_n, tid & 63);
        }
        __syncthreads();
        frontier_flush(s_list, s_n, &ctl->listed, list, &s_base, [&] { if (s_live) atomicAdd(&ctl->live, (unsigned long long) s_live); });
        __syncthreads();
    }
}

// one merge-path tile of the rows (begin / idx: the forward or the reverse CSR) of list[0, n): every slot is linked with
// its row's vertex.  A thread's slots go through the dependent accesses -- the slot, the two parents, the hook -- together.
__global__ void __launch_bounds__(WCC_THREADS) wcc_final_kernel(const int32_t* __restrict__ begin, const int32_t* __restrict__ idx,
                                                                const int32_t* __restrict__ list, int64_t n, const int64_t* __restrict__ off, int64_t m,
                                                                int32_t* __restrict__ parent) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_v[BFS_ITEMS + 2];
    __shared__ int64_t s_split[2][2];
    const int tid = threadIdx.x;
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, begin, list, n, off, m, s_off, s_row, [&](int i, int32_t v, bool) { s_v[i] = v; });
    constexpr int K = BFS_ITEMS / WCC_THREADS;
    if (t.e1 <= t.e0) return;   // (workgroup-uniform)
    int32_t u[K], w[K], pu[K], pw[K];
    bool valid[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int64_t x = t.e0 + tid + (int64_t) k * WCC_THREADS;
        valid[k] = x < t.e1;
        const int64_t xc = valid[k] ? x : t.e0;   // (loads stay unconditional: a slot that exists)
        const int lo = frontier_slot(s_off, nv, xc);
        u[k] = s_v[lo];
        w[k] = idx[(int64_t) s_row[lo] + (xc - s_off[lo])];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        pu[k] = parent[u[k]];
        pw[k] = parent[w[k]];
    }
#pragma unroll
    for (int k = 0; k < K; k++)
        if (valid[k]) wcc_hook(parent, pu[k], pw[k]);
}

__global__ void __launch_bounds__(WCC_THREADS) wcc_flag_kernel(const int32_t* __restrict__ parent, int64_t V, int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) flag[v] = parent[v] == v ? 1 : 0;
}
// comp[v] = rank of v's root; the component sizes by root in size[] (zeroed), those of the component that holds g* in the
// sharded counters instead: V adds to one word retire at ~90 per microsecond
__global__ void __launch_bounds__(WCC_THREADS) wcc_comp_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ rank,
                                                               const int32_t* __restrict__ flag, int64_t V, int32_t* __restrict__ comp,
                                                               int32_t* __restrict__ size, wcc_ctl* __restrict__ ctl) {
    const int32_t big = parent[ctl->gstar];
    unsigned long long in_big = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        const int32_t r = parent[v];
        comp[v] = rank[r];
        if (r == big) in_big++;
        else atomicAdd(&size[r], 1);
        if (v == V - 1) ctl->count = rank[v] + flag[v];
    }
    in_big = wave_sum(in_big);
    if ((threadIdx.x & 63) == 0 && in_big) {
        const int sh = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (BFS_SHARDS - 1);
        atomicAdd(&ctl->shard[sh].giant, in_big);
    }
}
__global__ void __launch_bounds__(WCC_THREADS) wcc_max_kernel(const int32_t* __restrict__ size, int64_t V, wcc_ctl* __restrict__ ctl) {
    __shared__ int32_t s_mx[WCC_THREADS / 64];
    int32_t mx = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) mx = max(mx, size[v]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < WCC_THREADS / 64; i++) mx = max(mx, s_mx[i]);
        if (mx) atomicMax(&ctl->largest, (unsigned int) mx);
    }
}

// what the forest needs besides parent[]: the knobs (read at every call), the live list, the control block and its mirror
struct wcc_work {
    int K = 0;
    bool skip = false;
    int32_t forced = -1;
    wbuf<int32_t> list;
    wbuf<wcc_ctl> ctl;
    frontier_scan fs[2];
    gmx_pinned<wcc_ctl> h_ctl;
    gmx_pinned<int64_t> h_m;
    int64_t live = 0, final_slots = 0;   // results: live vertices, slots of the final pass
    int alloc(const gmx_graph* g) {
        const int64_t V = g->V;
        K = (int) gmx_env_int("GMX_WCC_SAMPLE_ROUNDS", 2, 0, WCC_MAX_ROUNDS);
        skip = g->has_reverse && gmx_env_int("GMX_WCC_SKIP", 1, -1, 1) != 0;
        forced = (int32_t) gmx_env_int("GMX_WCC_GIANT", -1, -1, V - 1);
        GMX_CHECK(list.alloc(V));
        GMX_CHECK(ctl.alloc(1));
        GMX_CHECK(gmx_frontier_scan_alloc(&fs[0], (size_t) V, 0));
        if (skip) GMX_CHECK(gmx_frontier_scan_alloc(&fs[1], (size_t) V, 0));
        GMX_CHECK(h_ctl.alloc());
        GMX_CHECK(h_m.alloc(2));
        return GMX_OK;
    }
};

// sampling, compress, giant, live list and the final pass on parent[V]: every component is one tree in the end, its root
// its smallest vertex (the trees are not compressed yet).  phase_end(i) marks the end of phase i = 0 .. 3.
template <class PhaseEnd>
static int wcc_forest(gmx_graph* g, wcc_work& W, int32_t* parent, PhaseEnd phase_end) {
    const int64_t V = g->V, E = g->E;
    const int K = W.K;
    const bool skip = W.skip;
    wbuf<int32_t>& list = W.list;
    wbuf<wcc_ctl>& ctl = W.ctl;
    frontier_scan* fs = W.fs;
    gmx_pinned<wcc_ctl>& h_ctl = W.h_ctl;
    gmx_pinned<int64_t>& h_m = W.h_m;
    const int gv = grid_for(V);

    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(wcc_ctl), 0));
    hipLaunchKernelGGL(wcc_init_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, parent, V);
    for (int r = 0; r < K; r++) {
        // (a compress between the rounds as well: a round then starts from roots, and most of its links end at the two loads)
        if (r > 0) hipLaunchKernelGGL(wcc_compress_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, parent, V);
        hipLaunchKernelGGL(wcc_sample_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, (const int32_t*) g->begin.p, (const int32_t*) g->node_idx.p, V, (int32_t) r,
                           parent, ctl.p);
    }
    phase_end(0);
    if (K > 0) hipLaunchKernelGGL(wcc_compress_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, parent, V);
    phase_end(1);
    hipLaunchKernelGGL(wcc_giant_kernel, dim3(1), dim3(WCC_PROBES), 0, 0, (const int32_t*) parent, V, W.forced, ctl.p);
    hipLaunchKernelGGL(wcc_live_kernel, dim3(grid_for(V, BFS_ITEMS)), dim3(WCC_THREADS), 0, 0, (const int32_t*) parent, (const int32_t*) g->begin.p,
                       (const int32_t*) g->r_begin.p, V, skip ? 0 : 1, ctl.p, list.p);
    GMX_HIP(hipGetLastError());
    int64_t n = V, live = V;   // rows listed, live vertices
    if (skip) {
        GMX_CHECK(gmx_read_back(h_ctl, (const wcc_ctl*) ctl.p));
        n = (int64_t) h_ctl.p->listed;
        live = (int64_t) h_ctl.p->live;
    }
    phase_end(2);
    // the rows of the live list: the slots of both CSRs in one read-back
    const int ndir = skip ? 2 : 1;
    const int32_t* begs[2] = {g->begin.p, g->r_begin.p};
    const int32_t* idxs[2] = {g->node_idx.p, g->r_node_idx.p};
    int64_t final_slots = 0;
    if (n > 0 && E > 0) {
        for (int d = 0; d < ndir; d++) {
            GMX_CHECK(gmx_frontier_offsets(begs[d], list.p, n, &fs[d], nullptr, false));
            GMX_HIP(hipMemcpyAsync(&h_m.p[d], fs[d].off.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, 0));
        }
        GMX_HIP(hipStreamSynchronize(0));
        for (int d = 0; d < ndir; d++) {
            const int64_t m = h_m.p[d], nb = frontier_tiles(n, m);
            final_slots += m;
            if (m > 0)
                hipLaunchKernelGGL(wcc_final_kernel, dim3((unsigned) nb), dim3(WCC_THREADS), 0, 0, begs[d], idxs[d], (const int32_t*) list.p, n,
                                   (const int64_t*) fs[d].off.p, m, parent);
        }
        GMX_HIP(hipGetLastError());
    }
    phase_end(3);
    W.live = live;
    W.final_slots = final_slots;
    return GMX_OK;
}

extern "C" int gmx_wcc(gmx_graph_t* g, int32_t* comp_host, int64_t* num_comps, gmx_stats_t* stats_out) {
    GMX_REQUIRE(g && comp_host, "NULL argument");
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    if (num_comps) *num_comps = 0;
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    const bool phase_log = getenv("GMX_WCC_PHASES") != nullptr;   // per-phase times (events) for tools/wcc_prof.py

    gmx_ws_scope scope;
    wbuf<int32_t> parent, flag, rank, comp;
    wbuf<char> scan_tmp;
    wcc_work W;
    GMX_CHECK(parent.alloc(V));
    GMX_CHECK(W.alloc(g));
    GMX_CHECK(flag.alloc(V));
    GMX_CHECK(rank.alloc(V));
    GMX_CHECK(comp.alloc(V));
    wbuf<int32_t>& list = W.list;
    wbuf<wcc_ctl>& ctl = W.ctl;
    gmx_pinned<wcc_ctl>& h_ctl = W.h_ctl;
    const int K = W.K;
    size_t scan_bytes = 0;
    GMX_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag.p, rank.p, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
    GMX_CHECK(scan_tmp.alloc(scan_bytes));
    gmx_spans tm;
    gmx_event pev[5];
    if (phase_log)
        for (gmx_event& e : pev) GMX_CHECK(e.create());
    auto phase_end = [&](int ph) {
        if (phase_log) (void) hipEventRecord(pev[ph], 0);
    };
    const int gv = grid_for(V);

    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_CHECK(wcc_forest(g, W, parent.p, phase_end));
    const int64_t live = W.live, final_slots = W.final_slots;
    // finish: roots, ranks, comp, sizes (the list's memory is free now)
    int32_t* size = list.p;
    hipLaunchKernelGGL(wcc_compress_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, parent.p, V);
    hipLaunchKernelGGL(wcc_flag_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, (const int32_t*) parent.p, V, flag.p);
    GMX_HIP(rocprim::exclusive_scan((void*) scan_tmp.p, scan_bytes, flag.p, rank.p, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
    GMX_HIP(hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t) V, 0));
    hipLaunchKernelGGL(wcc_comp_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, (const int32_t*) parent.p, (const int32_t*) rank.p, (const int32_t*) flag.p, V,
                       comp.p, size, ctl.p);
    hipLaunchKernelGGL(wcc_max_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, (const int32_t*) size, V, ctl.p);
    GMX_HIP(hipGetLastError());
    phase_end(4);
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(gmx_read_back(h_ctl, (const wcc_ctl*) ctl.p));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(comp_host, comp.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    unsigned long long sampled = 0, in_big = 0;
    for (int i = 0; i < BFS_SHARDS; i++) {
        sampled += h_ctl.p->shard[i].sampled;
        in_big += h_ctl.p->shard[i].giant;
    }
    const int64_t largest = std::max((int64_t) in_big, (int64_t) h_ctl.p->largest);
    if (num_comps) *num_comps = h_ctl.p->count;
    stats->iterations = K + 1;
    stats->vertices_reached = largest;
    stats->edges_examined = (int64_t) sampled + final_slots;
    if (phase_log) {
        static const char* const names[5] = {"sampling", "compress", "live", "final", "finish"};
        float t[5];
        for (int i = 0; i < 5; i++) (void) hipEventElapsedTime(&t[i], i ? (hipEvent_t) pev[i - 1] : tm.begin_event(tm.KERNEL), pev[i]);
        fprintf(stderr, "gmx wcc phases:");
        for (int i = 0; i < 5; i++) fprintf(stderr, " %s %.3f ms%s", names[i], t[i], i < 4 ? "," : "\n");
    }
    if (getenv("GMX_WCC_LOG"))
        fprintf(stderr,
                "gmx wcc: V %lld E %lld sample_rounds %d sampled %llu giant %d skipped %lld live %lld reverse %d final_slots %lld comps %d largest %lld\n",
                (long long) V, (long long) E, K, sampled, (int) h_ctl.p->gstar, (long long) (V - live), (long long) live, g->has_reverse ? 1 : 0,
                (long long) final_slots, (int) h_ctl.p->count, (long long) largest);
    return GMX_OK;
}

// ---- the forest and the finish for other units (gmx_internal.h)
int gmx_wcc_forest(gmx_graph* g, int32_t* parent) {
    gmx_ws_scope scope;
    wcc_work W;
    GMX_CHECK(W.alloc(g));
    GMX_CHECK(wcc_forest(g, W, parent, [](int) {}));
    return gmx_wcc_compress(parent, g->V);
}
int gmx_wcc_compress(int32_t* parent, int64_t V) {
    hipLaunchKernelGGL(wcc_compress_kernel, dim3(grid_for(V)), dim3(WCC_THREADS), 0, 0, parent, V);
    GMX_HIP(hipGetLastError());
    return GMX_OK;
}
// comp[v] = rank of v's root, *count = the roots (wcc_comp_kernel without the sizes)
__global__ void __launch_bounds__(WCC_THREADS) wcc_canon_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ rank,
                                                                const int32_t* __restrict__ flag, int64_t V, int32_t* __restrict__ comp,
                                                                int32_t* __restrict__ count) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        comp[v] = rank[parent[v]];
        if (v == V - 1) *count = rank[v] + flag[v];
    }
}
int gmx_wcc_canon(int32_t* parent, int64_t V, int32_t* flag, int32_t* rank, int32_t* comp, int32_t* count) {
    const int gv = grid_for(V);
    size_t scan_bytes = 0;
    GMX_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flag, rank, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
    wbuf<char> scan_tmp;
    GMX_CHECK(scan_tmp.alloc(scan_bytes));   // (the caller's workspace scope)
    GMX_CHECK(gmx_wcc_compress(parent, V));
    hipLaunchKernelGGL(wcc_flag_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, (const int32_t*) parent, V, flag);
    GMX_HIP(rocprim::exclusive_scan((void*) scan_tmp.p, scan_bytes, flag, rank, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
    hipLaunchKernelGGL(wcc_canon_kernel, dim3(gv), dim3(WCC_THREADS), 0, 0, (const int32_t*) parent, (const int32_t*) rank, (const int32_t*) flag, V, comp, count);
    GMX_HIP(hipGetLastError());
    return GMX_OK;
}

void gmx_touch_wcc() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) wcc_init_kernel);
}
