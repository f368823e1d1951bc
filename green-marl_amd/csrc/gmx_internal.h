// gmx_internal.h -- shared internals of libgmx (HIP, gfx950 only).
#ifndef GMX_INTERNAL_H_
#define GMX_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <time.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "gmx.h"

void gmx_set_error(const char* fmt, ...);

#define GMX_HIP(call)                                                                      \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess) {                                                            \
            gmx_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_e)); \
            return GMX_ERR_HIP;                                                            \
        }                                                                                  \
    } while (0)

#define GMX_CHECK(call)                 \
    do {                                \
        int _s = (call);                \
        if (_s != GMX_OK) return _s;    \
    } while (0)

#define GMX_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            gmx_set_error(__VA_ARGS__); \
            return GMX_ERR_ARG;         \
        }                               \
    } while (0)

// Simple owning device buffer.
template <typename T>
struct dbuf {
    T* p = nullptr;
    size_t n = 0;
    dbuf() {}
    dbuf(const dbuf&) = delete;
    dbuf& operator=(const dbuf&) = delete;
    ~dbuf() { release(); }
    int alloc(size_t count) {
        release();
        n = count;
        size_t bytes = (count ? count : 1) * sizeof(T);
        hipError_t e = hipMalloc((void**) &p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            n = 0;
            gmx_set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
            return GMX_ERR_NOMEM;
        }
        return GMX_OK;
    }
    void release() {
        if (p) (void) hipFree(p);
        p = nullptr;
        n = 0;
    }
    T* take() { T* q = p; p = nullptr; n = 0; return q; }
};

// A hipEvent that is released on every return path.
struct gmx_event {
    hipEvent_t e = nullptr;
    gmx_event() {}
    gmx_event(gmx_event&& o) : e(o.e) { o.e = nullptr; }
    gmx_event(const gmx_event&) = delete;
    gmx_event& operator=(const gmx_event&) = delete;
    ~gmx_event() { if (e) (void) hipEventDestroy(e); }
    int create() { GMX_HIP(hipEventCreate(&e)); return GMX_OK; }
    operator hipEvent_t() const { return e; }
};

// The timed spans of gmx_stats_t.  An entry point says where its upload, its kernels and its download begin and end;
// finish() waits for the last end and fills h2d_ms / kernel_ms / d2h_ms.  A span's two events are created at its first
// begin(); a span that is never begun costs nothing and its field keeps the zero of the entry's memset.  A span that is
// begun again adds to its sum (the earlier pair is read first, which waits for its end).  Every failure, that of reading
// a recorded pair's time included, is GMX_ERR_HIP with the error text of GMX_HIP.
struct gmx_spans {
    enum span { H2D, KERNEL, D2H };
    gmx_event ev[3][2];
    double ms[3] = {0, 0, 0};
    bool pending[3] = {false, false, false};   // ended, not yet added to ms
    hipEvent_t last = nullptr;                 // the latest end
    int begin(span s, hipStream_t st = 0) {
        if (!ev[s][0].e) {
            GMX_CHECK(ev[s][0].create());
            GMX_CHECK(ev[s][1].create());
        }
        GMX_CHECK(fold(s));
        GMX_HIP(hipEventRecord(ev[s][0], st));
        return GMX_OK;
    }
    int end(span s, hipStream_t st = 0) {
        GMX_HIP(hipEventRecord(ev[s][1], st));
        pending[s] = true;
        last = ev[s][1];
        return GMX_OK;
    }
    int sync(span s) {   // wait for the span's end
        GMX_HIP(hipEventSynchronize(ev[s][1]));
        return GMX_OK;
    }
    hipEvent_t begin_event(span s) const { return ev[s][0]; }
    int fold(span s) {
        if (!pending[s]) return GMX_OK;
        float t = 0;
        GMX_CHECK(sync(s));
        GMX_HIP(hipEventElapsedTime(&t, ev[s][0], ev[s][1]));
        ms[s] += t;
        pending[s] = false;
        return GMX_OK;
    }
    // waits for the last end whether or not anyone reads the times: the asynchronous downloads of a d2h span have landed
    int finish(gmx_stats_t* stats) {
        if (last) GMX_HIP(hipEventSynchronize(last));
        if (!stats) return GMX_OK;
        for (int s = 0; s < 3; s++) GMX_CHECK(fold((span) s));
        if (ev[H2D][0].e) stats->h2d_ms = ms[H2D];
        if (ev[KERNEL][0].e) stats->kernel_ms = ms[KERNEL];
        if (ev[D2H][0].e) stats->d2h_ms = ms[D2H];
        return GMX_OK;
    }
};

// GMX_*_PHASES: the device time of one phase at a time, added to a slot the caller names.  It synchronises at every
// end(), so it is the profiler's mode only: off, it creates no events and does nothing.  Failures are swallowed.
struct gmx_phase_clock {
    bool on = false;
    gmx_event ev[2];
    int enable(bool want) {
        if (want)
            for (gmx_event& e : ev) GMX_CHECK(e.create());
        on = want;
        return GMX_OK;
    }
    void begin() {
        if (on) (void) hipEventRecord(ev[0], 0);
    }
    float end(float* slot = nullptr) {   // the device time since begin() (0 when off or on failure)
        float t = 0;
        if (on && hipEventRecord(ev[1], 0) == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess &&
            hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess && slot)
            *slot += t;
        return t;
    }
};

// Pinned host words that are released on every return path.
template <typename T>
struct gmx_pinned {
    T* p = nullptr;
    gmx_pinned() {}
    gmx_pinned(const gmx_pinned&) = delete;
    gmx_pinned& operator=(const gmx_pinned&) = delete;
    ~gmx_pinned() { if (p) (void) hipHostFree(p); }
    int alloc(size_t count = 1) {
        if (hipHostMalloc((void**) &p, count * sizeof(T), hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            gmx_set_error("pinned host allocation (%zu bytes) failed", count * sizeof(T));
            return GMX_ERR_HIP;
        }
        return GMX_OK;
    }
};
// a device control block (count words of it) into its pinned mirror on stream 0; synchronises
template <typename T>
static inline int gmx_read_back(gmx_pinned<T>& host, const T* dev, size_t count = 1) {
    GMX_HIP(hipMemcpyAsync(host.p, dev, count * sizeof(T), hipMemcpyDeviceToHost, 0));
    GMX_HIP(hipStreamSynchronize(0));
    return GMX_OK;
}

// an integer knob of the environment: dflt when unset or empty, else clamped to [lo, hi]
static inline int64_t gmx_env_int(const char* name, int64_t dflt, int64_t lo, int64_t hi) {
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    const long long v = atoll(e);
    return v < lo ? lo : (v > hi ? hi : (int64_t) v);
}

// ---- workspace: where the big temporaries of graph construction and plan builds live ----
// Device memory that has just been freed is not free: the driver wipes it before it hands it out again, and a
// hipMalloc that needs such memory waits for the wipe -- measured here as stalls of 1-2.4 s inside an RMAT-26 plan build
// (an 8 GB allocation behind the ~100 GB of temporaries the graph construction had freed), against 0.2 s without them.
// So the multi-gigabyte temporaries are carved from chunks that stay allocated for the life of the process (stack
// discipline: gmx_ws_scope rewinds on exit; a buffer's release() is a no-op) and nothing big is ever freed between a
// graph's construction and its plans.  gmx_workspace_release() (gmx.h) gives the chunks back.
struct gmx_ws_mark { size_t chunk, off; };
void* gmx_ws_alloc(size_t bytes);
gmx_ws_mark gmx_ws_top();
void gmx_ws_rewind(gmx_ws_mark m);
struct gmx_ws_scope {
    gmx_ws_mark m;
    gmx_ws_scope() : m(gmx_ws_top()) {}
    // (nothing may still be running on memory that the next build will hand out again: also on the error paths)
    ~gmx_ws_scope() { (void) hipDeviceSynchronize(); gmx_ws_rewind(m); }
    gmx_ws_scope(const gmx_ws_scope&) = delete;
    gmx_ws_scope& operator=(const gmx_ws_scope&) = delete;
};
// dbuf's interface on workspace memory (valid until the enclosing gmx_ws_scope ends)
template <typename T>
struct wbuf {
    T* p = nullptr;
    size_t n = 0;
    wbuf() {}
    wbuf(const wbuf&) = delete;
    wbuf& operator=(const wbuf&) = delete;
    int alloc(size_t count) {
        n = count;
        p = (T*) gmx_ws_alloc((count ? count : 1) * sizeof(T));
        if (!p) { n = 0; return GMX_ERR_NOMEM; }
        return GMX_OK;
    }
    void release() { p = nullptr; n = 0; }
};

struct gmx_bfs;
struct tcd_plan;
void gmx_tcd_plan_free(tcd_plan* p);   // gmx_tcd.hip
struct vc_plan;
void gmx_vc_plan_free(vc_plan* p);     // gmx_vcover.hip
struct spf_scratch;
void gmx_spf_scratch_free(spf_scratch* s);   // gmx_sssp_f64.hip

struct gmx_graph {
    int64_t V = 0, E = 0;
    bool has_reverse = false;
    // original numbering, rows ascending (semi-sorted)
    dbuf<int32_t> begin, node_idx, r_begin, r_node_idx;
    // gm_graph's e_idx2idx (gm_graph.h:141, do_semi_sort gm_graph.cc:468-503): slot of the uploaded (unsorted) forward
    // CSR that every slot of the sorted rows came from.  Empty: the upload was already in order (identity).
    dbuf<int32_t> e_idx2idx;
    // every row of node_idx (r_node_idx) non-decreasing.  Graphs built on the device are sorted by construction; an upload
    // that keeps the caller's arrays verbatim records what its validation pass found (gmx.h: the sorted-row contract)
    bool rows_sorted = true, r_rows_sorted = true;
    int device = 0;
    // PageRank plans built by the whole-kernel entries (fp32, fp64), kept for the next call on the same
    // graph: the plan is graph preprocessing, like the reverse CSR.  Freed with the graph.
    gmx_pr* pr_cache[4] = {nullptr, nullptr, nullptr, nullptr};   // [2], [3]: the pull-sweep plans used for d outside (0, 1]
    // the same for the multi-GPU form of those entries (gmx_pr_multi.hip): N rank states driven by one host thread
    struct gmx_pr_multi* pr_multi_cache[2] = {nullptr, nullptr};
    bool pr_multi_refused = false;   // the multi-GPU exchange failed its first-contact check on this box: single GPU from then on
    // triangle counting: -1 not examined, 0 general graph, 1 symmetric and simple -> `tc_oriented` holds the
    // forward CSR of the same graph renumbered by ascending degree (its reverse CSR is the same arrays)
    int tc_sym_state = -1;
    gmx_graph* tc_oriented = nullptr;
    // on the oriented copy: the adjacency among its tc_hubs highest vertices (the hubs: ids >= V - tc_hubs) as a bit matrix,
    // row u - (V - tc_hubs), bit w - (V - tc_hubs) (gmx_tc.hip)
    dbuf<uint32_t> tc_hub_bits;
    int64_t tc_hubs = 0;
    // triangle_counting_directed and clustering: the two renumbered CSRs and the work items (gmx_tcd.hip, gmx_tcd_plan.h; the
    // hub matrix of gmx_lcc.hip), built on first use by either; the plan records the order it was built with
    tcd_plan* tcd_cache = nullptr;
    // v_cover: Deg0, the incident lists sorted by (Deg0 of the other end descending, uploaded slot ascending), their offsets
    // and the lowest incident slot per vertex (gmx_vcover.hip), built on first use
    vc_plan* vc_cache = nullptr;
    // sssp_path_f64: the per-vertex words, lists and the cost copies of a call (gmx_sssp_f64.hip), allocated on first use
    spf_scratch* spf_cache = nullptr;
    // hop_dist: the single-rank traversal state (queues, bitmaps, dist[]) of the whole-kernel entry, kept for the
    // next call on the same graph instead of nine allocations per call
    gmx_bfs* bfs_cache = nullptr;
    // bottom-up BFS: per vertex the in-neighbour to try first (the one with most out-edges among the first of its
    // in-row; -1: no in-edges).  Graph preprocessing like the reverse CSR, built with the first traversal object.
    dbuf<int32_t> bfs_hint;
    // ... and the BFS_HUBS vertices with most out-edges ("hubs"; all vertices if there are fewer): a hint that is a hub is
    // stored as its slot in this list, and a bottom-up level probes the hubs' frontier bits in LDS (gmx_bfs.hip)
    dbuf<int32_t> bfs_hub_id;     // [bfs_hubs]; empty when every vertex is a hub (slot = id)
    int64_t bfs_hubs = 0;
    bool bfs_hint_plain = false;  // V > 2^30: the hints are plain vertex ids (no room for the flag bits)
    // scc: the transposed view (g's four CSR arrays with the roles swapped, its own traversal object and hints) that the
    // backward traversal runs on; it borrows the arrays and is freed with g (gmx_scc.hip)
    gmx_graph* scc_transpose = nullptr;
};

// root's whole traversal on g's single-rank traversal object (created on first use, as gmx_hop_dist does): *dist = its
// device dist[] (INT_MAX = unreached, valid until the next traversal on g), *edges = edge slots inspected (gmx_bfs.hip)
int gmx_bfs_reach(gmx_graph* g, int32_t root, const int32_t** dist, int64_t* edges);
// comp_BC's per-seed loop on a device BC[V] (zero_bc: G.BC = 0 first; tm: begins its kernel span, or NULL); *reached = vertices reached, summed over the seeds.
// The caller has checked g, the reverse CSR and the seeds (gmx_bfs.hip; gmx_bc and gmx_bc_batch's per-seed batches)
int gmx_bc_seeds(gmx_graph* g, const gmx_node_t* seeds, int32_t nseeds, int skip_root, float* bc_dev, bool zero_bc, gmx_spans* tm, int64_t* reached);

// ---- graph construction helpers (gmx_graph.hip) ----
// keys are (row << 32 | col).  Sorts keys in place (double buffer), then writes
// begin[V+1] and idx[E].
int gmx_csr_from_keys(uint64_t* keys, uint64_t* keys_alt, int64_t V, int64_t E,
                      int32_t* begin, int32_t* idx, hipStream_t stream, int32_t* slots = nullptr);   // slots: [E] key order -> input position
// keys[e] = (row(e) << 32 | col(e)) from a CSR; if transpose, (col << 32 | row).
// perm (optional): map both endpoints through perm[] first.
int gmx_keys_from_csr(const int32_t* begin, const int32_t* idx, int64_t V, int64_t E,
                      bool transpose, const int32_t* perm, uint64_t* keys, hipStream_t stream);
int gmx_keys_from_edges(const int32_t* src, const int32_t* dst, int64_t E, bool transpose,
                        const int32_t* perm, uint64_t* keys, hipStream_t stream);
// a[i] = i: the values a sort of keys carries along.  Defined in gmx_graph.hip and launched from gmx_route.hip as well: without
// relocatable device code that works through the defining unit's host stub, so the kernel must stay non-static there.
__global__ void iota_kernel(int32_t* __restrict__ a, int64_t n);
// perm[order[j]] = j: the renumbering a sort by degree gives.  Defined in gmx_tc.hip and launched from gmx_tcd.hip as well, the same way.
__global__ void tc_invert_kernel(const int32_t* __restrict__ order, int64_t V, int32_t* __restrict__ perm);

// ---- cold-source part of the PageRank sweep (gmx_pr_cold.hip) ----
// Sources whose id inside their rank range [r * slice, (r + 1) * slice) is >= T are "cold": their edges are not
// gathered by the pull sweep but pushed through plan-time-ordered bins (see gmx_pr_cold.hip).
struct pr_cold;
struct pr_cold_params {
    int elem;        // 4 (float) or 8 (double)
    int nranks;
    int64_t slice;   // ids per rank range of the contribution replica
    int64_t T;       // hot ids per rank range
    int64_t row_lo;  // first owned row (internal numbering)
    int64_t nactive; // owned rows with in-edges
    const int32_t* index_of_row;   // [rows] local row -> position in the active-row list (device)
    const int32_t* deg_by_id;      // [nranks * slice] out-degree by internal id (device; padding ids < 0), or NULL
};
// keys[Ec]: (row << 32 | source) of the cold in-edges of the owned rows, any order (device).
int pr_cold_create(const uint64_t* keys, int64_t Ec, const pr_cold_params& prm, hipStream_t s, pr_cold** out);
void pr_cold_free(pr_cold* c);
// what the fused finish needs to apply the PageRank update of active row i itself (see pr_combine_kernel)
struct pr_cold_fuse {
    const int32_t* active;     // [nactive] local row of active row i
    const int32_t* outdeg_c;   // [nactive]
    void* rk_c;                // [nactive] x elem: ranks, updated in place
    void* next_owned;          // owned range of the replica being produced, indexed by local row
    double base, d;
};
// enqueue phases 1-3: reads the contribution replica; fuse == NULL leaves the row sums in pr_cold_partial(),
// otherwise the rows are finished in place and pr_cold_diff_partials() holds the |val - rank| partials
int pr_cold_launch(pr_cold* c, const void* contrib, const pr_cold_fuse* fuse, hipStream_t s);
// the same in pieces (see pr_cold_set_parts in gmx_pr_cold.hip): phase 1 per tile class, phases 2-3 per row part
int pr_cold_set_parts(pr_cold* c, int nparts, const int64_t* act_bound, int64_t hub, int64_t live);
int pr_cold_parts(const pr_cold* c);
int64_t pr_cold_class_items(const pr_cold* c, int cls);   // phase-1 work items of a tile class
int pr_cold_gather(pr_cold* c, const void* contrib, int cls, hipStream_t s);
int pr_cold_accumulate(pr_cold* c, const pr_cold_fuse* fuse, int part, hipStream_t s);
const double* pr_cold_diff_partials(const pr_cold* c, int64_t* n);
bool pr_cold_covers_all_rows(const pr_cold* c);
// fp32 plans keep ONE 2^-62 fixed-point limb: true if that provably holds the 1e-6 bar for damping d on a graph of N
// vertices (see pr_cold_limb_guard in gmx_pr_cold.hip); fp64 plans (two limbs): always true
bool pr_cold_limb_guard(const pr_cold* c, double d, double N);
const void* pr_cold_partial(const pr_cold* c);   // [nactive] x elem, indexed like the per-slice partial sums
int64_t pr_cold_edges(const pr_cold* c);
int64_t pr_cold_items(const pr_cold* c);
void pr_cold_shape(const pr_cold* c, gmx_pr_cold_shape_t* out);   // everything but `fused` (NULL plan: zeros)

// ---- whole-kernel PageRank over several GPUs from one host thread (gmx_pr_multi.hip) ----
struct gmx_pr_multi;
int gmx_pr_multi_ranks(const gmx_graph* g);    // ranks the entry uses for this graph (GMX_DEVICES, GMX_PR_RANKS); 1 = single GPU
int gmx_pr_multi_create(gmx_graph* g, int elem, int nranks, gmx_pr_multi** out);
int gmx_pr_multi_run(gmx_pr_multi* m, double e, double d, int32_t max_iter, void* rank_host, gmx_stats_t* stats);
void gmx_pr_multi_free(gmx_pr_multi* m);
bool gmx_pr_multi_verified(const gmx_pr_multi* m);   // false: the first exchange has not passed its check

// ---- gmx_wcc's forest for the units that build on it (gmx_wcc.hip; gmx_bicc.hip)
#ifdef __HIPCC__
__device__ __forceinline__ int32_t wcc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// link(u, v), from a = an ancestor of u (or u), b = one of v: while they differ, the larger is hooked under the smaller
// if it still is a root.  THE MEMORY RULE: a plain load of parent[] may be served from a stale line in this CU's L1 or
// this XCD's L2 while a wave on another XCD hooks.  A stale value is an older, still valid ancestor relation (trees only
// merge, and equal ancestors mean "already one tree"), so the FIRST reads -- a and b, by the caller -- may be plain.  Every
// retry must make progress from what the atomic returned (or from wcc_load, a relaxed agent-scope atomic load): a loop that
// re-reads parent[] with plain loads can spin on a stale line for ever.  Here a step reads parent[hi] with wcc_load; a
// root is hooked by the CAS, and where it is none (or the CAS lost) the pair becomes (parent[hi] < hi, lo): its maximum
// falls with every step.  The climb is loads, not atomics: with a CAS at every step and no compress between the rounds, the
// 5.4 M links of the second sampling round at RMAT-24 took 9.3 ms against 0.3 ms for the first round's 7.6 M (DESIGN.md
// 4.2l) -- every climb through a big tree ends in atomics on the few vertices below its root.
__device__ __forceinline__ void wcc_hook(int32_t* __restrict__ parent, int32_t a, int32_t b) {
    while (a != b) {
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        int32_t p = wcc_load(&parent[hi]);
        if (p == hi) {
            p = atomicCAS(&parent[hi], hi, lo);
            if (p == hi) break;
        }
        a = p;
        b = lo;
    }
}
#endif
// gmx_wcc's device part up to its last compress, on stream 0 and with gmx_wcc's knobs: parent[V] (device, the caller's)
// ends as parent[v] = the smallest vertex of v's weak component.  V > 0; temporaries come from the workspace and go back.
int gmx_wcc_forest(gmx_graph* g, int32_t* parent);
// parent[v] = the root of v, for a forest hooked by wcc_hook (enqueued on stream 0)
int gmx_wcc_compress(int32_t* parent, int64_t V);
// gmx_wcc's finish on such a forest: compress, then comp[v] (device) = the rank of v's root among the roots in id order
// and *count (device) = the roots.  flag, rank: V words of scratch each.  Enqueued on stream 0.
int gmx_wcc_canon(int32_t* parent, int64_t V, int32_t* flag, int32_t* rank, int32_t* comp, int32_t* count);

// GMX_PLAN_TIMING=1: where a plan build spends its time (synchronises at every mark)
struct gmx_tick {
    bool on;
    double t0;
    const char* who;
    static double now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
    explicit gmx_tick(const char* w) : on(getenv("GMX_PLAN_TIMING") != nullptr), t0(0), who(w) { if (on) { (void) hipDeviceSynchronize(); t0 = now(); } }
    void mark(const char* what) {
        if (!on) return;
        (void) hipDeviceSynchronize();
        const double t = now();
        fprintf(stderr, "gmx timing %s: %-28s %8.2f ms\n", who, what, (t - t0) * 1e3);
        t0 = t;
    }
};

void gmx_touch_pagerank();
void gmx_touch_pr_cold();
void gmx_touch_bfs();
void gmx_touch_sssp();
void gmx_touch_nbrcount();
void gmx_touch_scc();
void gmx_touch_comm();
void gmx_touch_pf();
void gmx_touch_bc_batch();
void gmx_touch_tcd();
void gmx_touch_vcover();
void gmx_touch_match();
void gmx_touch_spf();
void gmx_touch_route();
void gmx_touch_walk();
void gmx_touch_wcc();
void gmx_touch_kcore();
void gmx_touch_msf();
void gmx_touch_color();
void gmx_touch_close();
void gmx_touch_lcc();
void gmx_touch_bicc();
void gmx_touch_ktruss();
void gmx_touch_kclique();
void gmx_touch_squares();
void gmx_touch_graphlets();
void gmx_touch_louvain();
void gmx_warm_modules();   // once per process: load every translation unit's code object (see gmx_touch_*)

static inline int gmx_bits_for(int64_t v) {  // bits needed to represent values in [0, v)
    int b = 1;
    while ((1LL << b) < v && b < 32) b++;
    return b;
}

#endif
