// gmx_classcount.h -- what the entries share that count something per vertex on the plan of gmx_tcd.hip, by size class over a
// sorted vertex list: gmx_kclique.hip (gmx_kclique) and gmx_squares.hip (gmx_squares).
//
// Such an entry sorts the plan's vertices by a size once per plan (tcd_sort_by_key), gives every class of sizes a kernel of
// its own over a range of that list -- the classes whose tables fit in LDS one launch each, the rest ("global") in batches of
// workspace memory -- counts in 64-bit words by plan id and sends the per-vertex counts back through perm.  Here are the word
// and the credit modes, the run-time mode as a template argument (cc_with_mode), the batches of the global class
// (cc_plan_batches), the finishing kernel and the frame of the entry: the early zero answer, the call's scratch and the end
// of the timed region with the checksum and the statistics.  What is counted and how -- the walks, the tables, the matrices,
// the credits -- is the entry's own and stays in its unit.
#ifndef GMX_CLASSCOUNT_H_
#define GMX_CLASSCOUNT_H_

#include "gmx_tcd_plan.h"
#include "gmx_rowgroup.h"
#include "gmx_frontier.h"

#include <algorithm>
#include <type_traits>

#define CC_THREADS 256

typedef unsigned long long cc_word;

// MODE: where the per-vertex credits go: nowhere (count_host == NULL), through counters close to the workgroup that are
// flushed once per vertex, or every one by a global atomic (GMX_*_PLAIN)
enum { CC_NONE = 0, CC_LOCAL = 1, CC_PLAIN = 2 };
static inline const char* cc_mode_word(int mode) { return mode == CC_NONE ? "none" : mode == CC_PLAIN ? "global" : "lds"; }   // the log lines' `counts`

// f(std::integral_constant<int, i>()) for the i in 0 .. 2 that is known at run time only: a mode (or one of three steps) as a
// template argument, so that a launch is written once
template <class F>
static inline int cc_with_mode(int i, F f) {
    if (i == 0) return f(std::integral_constant<int, 0>());
    if (i == 1) return f(std::integral_constant<int, 1>());
    return f(std::integral_constant<int, 2>());
}

// the wave's sum, the same in every lane
__device__ __forceinline__ cc_word cc_wave_total(cc_word x) { return rg_first_lane(wave_sum(x)); }

// ------------------------------------------------------------------ finishing kernel
// one thread per caller's id x: the count a + b / 2 (b NULL: a) back through perm; the vertices with a count and the sum of
// the counts.  static: every unit that launches it has its own (no relocatable device code)
static __global__ void __launch_bounds__(CC_THREADS) cc_finish_kernel(const cc_word* __restrict__ a, const cc_word* __restrict__ b,
                                                                      const int32_t* __restrict__ perm /* NULL: identity */, int64_t V, int64_t* __restrict__ cnt_out,
                                                                      cc_word* __restrict__ nonzero, cc_word* __restrict__ total) {
    cc_word nz = 0, sum = 0;
    for (int64_t x = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; x < V; x += (int64_t) gridDim.x * blockDim.x) {
        const int64_t p = perm ? perm[x] : x;
        const cc_word cv = a[p] + (b ? b[p] >> 1 : 0);
        cnt_out[x] = (int64_t) cv;
        nz += cv ? 1 : 0;
        sum += cv;
    }
    nz = wave_sum(nz);
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) {
        if (nz) atomicAdd(nonzero, nz);
        if (sum) atomicAdd(total, sum);
    }
}

// ------------------------------------------------------------------ host
// The global class's batches: entries [lo, hi) of the list, every one in a slot of `stride` words, the widest any of them
// needs (stride_of(i), i = the position in the list).  A batch is grown while its entries x stride stay within the budget;
// an entry that alone exceeds it is a batch by itself.  Returns the words of the largest batch.
struct cc_batch { int64_t lo, hi, stride; };
template <class Stride>
static inline int64_t cc_plan_batches(int64_t lo, int64_t hi, Stride stride_of, int64_t budget_words, std::vector<cc_batch>* batches) {
    int64_t most = 0;
    for (int64_t a = lo; a < hi;) {
        int64_t b = a + 1, stride = stride_of(a);
        while (b < hi && (b + 1 - a) * std::max(stride, stride_of(b)) <= budget_words) {
            stride = std::max(stride, stride_of(b));
            b++;
        }
        batches->push_back({a, b, stride});
        most = std::max(most, (b - a) * stride);
        a = b;
    }
    return most;
}

// rc, with the text of a GMX_ERR_NOMEM from the sort of the list's keys (the caller's buffers and tcd_sort_by_key) in the
// entry's words: ws_bytes of workspace or, once the sort has asked for them (tmp_bytes != 0), its temporary storage
static inline int cc_sort_nomem(int rc, const char* who, const char* by, int64_t V, size_t ws_bytes, size_t tmp_bytes) {
    if (rc == GMX_ERR_NOMEM) {
        const std::string why = gmx_last_error();
        gmx_set_error("%s: the sort of %lld vertices by %s needs %zu bytes of %s: %s", who, (long long) V, by, tmp_bytes ? tmp_bytes : ws_bytes,
                      tmp_bytes ? "temporary storage" : "workspace", why.c_str());
    }
    return rc;
}

// E = 0 or self loops only (*empty): zeros, answered without a plan
static inline int cc_answer_empty(const gmx_graph* g, int64_t* count_host, gmx_stats_t* stats, bool* empty) {
    int64_t real = 0;
    GMX_CHECK(tcd_real_slots(g, &real));
    *empty = real == 0;
    if (*empty) {
        if (count_host) memset(count_host, 0, (size_t) g->V * sizeof(int64_t));
        if (stats) stats->iterations = 1;
    }
    return GMX_OK;
}

struct cc_scratch {   // a call's scratch
    gmx_ws_scope scope;
    dbuf<cc_word> out;       // [nctr]: the sums, zero
    dbuf<cc_word> acc;       // [nacc x V]: the accumulators in the plan's numbering     } with count_host only
    dbuf<int64_t> cnt_out;   // [V]: the array asked for                                 }
    wbuf<char> ws;           // [ws_bytes]: the global class's workspace, if any
    // nomem_fmt: the text of GMX_ERR_NOMEM, with %zu for the bytes of it all and %s for the reason
    int alloc(int nctr, bool counts, int nacc, int64_t V, size_t ws_bytes, const char* nomem_fmt) {
        const size_t bytes = (counts ? (size_t) (nacc + 1) * (size_t) V * sizeof(int64_t) : 0) + (size_t) nctr * sizeof(cc_word) + ws_bytes;
        if (out.alloc((size_t) nctr) || (counts && (acc.alloc((size_t) nacc * (size_t) V) || cnt_out.alloc((size_t) V))) || (ws_bytes && ws.alloc(ws_bytes))) {
            const std::string why = gmx_last_error();
            gmx_set_error(nomem_fmt, bytes, why.c_str());
            return GMX_ERR_NOMEM;
        }
        GMX_HIP(hipMemset(out.p, 0, (size_t) nctr * sizeof(cc_word)));
        return GMX_OK;
    }
};

// the end of the timed region: the kernel span ends, the download span reads the sums into h[nctr] and the counts into
// count_host, the times go to stats
static inline int cc_read_back(gmx_spans& tm, const cc_scratch& S, cc_word* h, int nctr, int64_t V, int64_t* count_host, gmx_stats_t* stats) {
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(h, S.out.p, (size_t) nctr * sizeof(cc_word), hipMemcpyDeviceToHost));
    if (count_host) GMX_HIP(hipMemcpy(count_host, S.cnt_out.p, (size_t) V * sizeof(int64_t), hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));
    return GMX_OK;
}

// the checksum of the per-vertex counts -- every one of the `total` things found has m vertices -- and the statistics
static inline int cc_check(const char* who, bool counts, cc_word sum, int m, cc_word total, cc_word nonzero, int64_t examined, gmx_stats_t* stats) {
    if (counts && sum != (cc_word) m * total) {
        gmx_set_error("%s: the counts sum to %llu, not to %d x %llu", who, sum, m, total);
        return GMX_ERR_HIP;
    }
    if (stats) {
        stats->iterations = 1;
        stats->edges_examined = examined;
        stats->vertices_reached = counts ? (int64_t) nonzero : 0;
    }
    return GMX_OK;
}

// ------------------------------------------------------------------ the counts of one entry for another (gmx_graphlets.hip)
// The walks of gmx_squares and gmx_kclique at their default thresholds on a plan the caller holds, the per-vertex words left
// on the device in PLAN ids; mode as above (CC_NONE: the totals only, the word arrays may be NULL).  The callers zero their
// words; the launches are enqueued on stream 0 and have run on return.  *classes_built: the entry's additions to the plan were
// built by this call.
// gmx_squares.hip: squares through v = mid[v] + end2[v] / 2; squares = total2[0] + total2[1] / 2.  The adjacency is there.
int sq_count_into(tcd_plan* p, int mode, cc_word* mid, cc_word* end2, cc_word* total2, bool* classes_built);
// gmx_kclique.hip: the k-cliques through v = cnt[v]; *total = their number
int kc_count_into(tcd_plan* p, int k, int mode, cc_word* cnt, cc_word* total, bool* classes_built);

#endif
