// gmx_route.hip -- point-to-point route queries with Int edge weights for gfx950: bidir_dijkstra.gm (a search from src
// over out-edges and one from dst over in-edges, stopped when the two meet) and, with the reverse side never expanded,
// sssp_dijkstra.gm (one-sided search with early exit).  The weights and everything a query needs stay on the device in a
// route object, so a query uploads a few scalars only.  gmx.h has the contract, DESIGN.md 4.2b''' the design and the
// argument for the stop rule; in short:
//   - labels: per side one 64-bit word per vertex, (distance << 32) | slot of the edge it came over in that side's CSR
//     (forward slot for F, reverse slot for R), lowered as in gmx_sssp_path: a positive-weight edge by atomicMin, a
//     zero-weight edge only when it lowers the distance strictly (compare-and-swap), so predecessor chains have no cycle;
//   - the meeting word mu = (cost << 32) | vertex under atomicMin: a relaxation that lowers v's distance on one side and
//     finds v's label on the other side finite offers the sum, AT THE RELAXATION;
//   - a round expands ONE side (the one whose queue holds fewer row slots): the other side's labels do not move during it;
//   - a side's queue holds the vertices with a row whose distance dropped in that side's last round; L = the lowest
//     distance that put a vertex there bounds every label the side may still produce (weights are >= 0);
//   - an offer c is dropped when c >= cost(mu), or when the other side has not reached v and c + L_other > cost(mu);
//   - stop when a queue is empty or L_F + L_R >= cost(mu);
//   - while the side to expand holds few slots one workgroup runs the rounds of both sides in one launch (rt_tail_kernel);
//   - one wave extracts the route on the device (rt_extract_kernel), cutting a zero-weight loop between the two chains.
#include "gmx_frontier.h"

#include <limits.h>
#include <rocprim/rocprim.hpp>

#define RT_THREADS 256           // = BFS_THREADS (frontier_flush copies with that stride)
static_assert(RT_THREADS == BFS_THREADS, "frontier_flush and first_bad_slot_kernel are built for BFS_THREADS");
#define RT_TAIL_THREADS 1024
#define RT_TAIL 4096             // GMX_ROUTE_TAIL: the tail launch takes over while the side to expand holds at most this many slots
#define RT_TAIL_LANE 8           // the tail reads a row of at most this many slots with one lane, a longer one with a wave
#define RT_TAIL_MAX_ROUNDS 65536 // rounds a tail launch runs before it hands back whatever the queues hold
#define RT_INF 0x7FFFFFFFu       // the distance of a vertex a side has not reached (INT_MAX: path sums stay below it)
#define RT_NIL 0xFFFFFFFFu
#define RT_WORD(d, e) (((rt_word) (uint32_t) (d) << 32) | (rt_word) (uint32_t) (e))

typedef unsigned long long rt_word;

// what the kernels leave for the host (one read-back per grid round or tail launch)
struct rt_ctl {
    rt_word mu;              // (cost << 32) | meeting vertex; RT_WORD(RT_INF, RT_NIL): none yet
    rt_word nnext;           // a grid round: tail of the next queue, the slots of its rows, max of 2^32 - distance over its entries
    rt_word mnext;
    rt_word linv;
    rt_word seed_deg[2];     // init: slots of src's out-row and of dst's in-row
    rt_word tail_n[2];       // a tail launch: both queues as it leaves them,
    rt_word tail_m[2];
    rt_word tail_L[2];
    rt_word tail_rounds[2];  // and what it ran
    rt_word tail_slots[2];
    rt_word tail_queued;
    rt_word hops;            // extract: edges of the route
    rt_word bad;             // weight check: E - (first slot whose weight is negative), 0: none; extract: 1 when a chain did not end (never)
    rt_word pad[3];
};

// one side's view of the graph: side 0 walks the forward CSR from src, side 1 the reverse CSR from dst
struct rt_side {
    const int32_t* begin;
    const int32_t* idx;
    const int32_t* w;        // by this CSR's slots
    rt_word* label;          // [V]
    int32_t* stamp;          // [V] tag of the round that last queued the vertex
};

struct rt_dev {
    rt_side side[2];
    rt_ctl* ctl;
    int64_t V;
};

// labels and mu are read and written through device-scope accesses everywhere: in the tail launch they pass between the
// waves of one workgroup behind a barrier only
__device__ __forceinline__ rt_word rt_load(const rt_word* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// slot e = n -> v of a queued n at distance d on side s (other: the side that rests; L_other: its bound).  Returns whether
// v enters the next queue; *deg = the slots of its row then.  *low = the distance when it dropped and v has a row.
__device__ __forceinline__ bool rt_relax(const rt_side& S, const rt_side& O, rt_ctl* ctl, bool on, uint32_t d, int32_t e, rt_word L_other,
                                         int32_t tag, int32_t* v_out, int32_t* deg, uint32_t* low) {
    if (!on) return false;
    const int32_t l = S.w[e];
    const rt_word c = (rt_word) d + (rt_word) (uint32_t) l;
    const rt_word muc = rt_load(&ctl->mu) >> 32;
    if (c >= muc) return false;                       // cannot be part of a better route
    const int32_t v = S.idx[e];
    const uint32_t nd = (uint32_t) c;
    const rt_word cand = RT_WORD(nd, e);
    rt_word cur = rt_load(&S.label[v]);
    if (l > 0 ? cand >= cur : (uint32_t) (cur >> 32) <= nd) return false;
    const uint32_t od = (uint32_t) (rt_load(&O.label[v]) >> 32);
    if (od == RT_INF && c + L_other > muc) return false;   // the other side is not there, and will not get there below L_other
    bool dropped = false;
    if (l > 0) {
        dropped = (uint32_t) (atomicMin(&S.label[v], cand) >> 32) > nd;   // equal distance: a smaller slot, no new work
    } else {
        while ((uint32_t) (cur >> 32) > nd) {         // zero weight: only a strictly lower distance
            const rt_word seen = atomicCAS(&S.label[v], cur, cand);
            if (seen == cur) {
                dropped = true;
                break;
            }
            cur = seen;
        }
    }
    if (!dropped) return false;
    if (od != RT_INF) atomicMin(&ctl->mu, RT_WORD(nd + od, v));   // the two searches meet at v
    const int32_t dg = S.begin[v + 1] - S.begin[v];
    if (dg <= 0) return false;
    if (nd < *low) *low = nd;
    if (atomicExch(&S.stamp[v], tag) == tag) return false;       // queued in this round already
    *v_out = v;
    *deg = dg;
    return true;
}

// ------------------------------------------------------------------ grid kernels
__global__ void __launch_bounds__(RT_THREADS) rt_init_kernel(rt_dev D, int32_t src, int32_t dst, int32_t* __restrict__ pos, int32_t* __restrict__ qf,
                                                              int32_t* __restrict__ qr) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    if (i == 0) {
        const int32_t df = D.side[0].begin[src + 1] - D.side[0].begin[src];
        const int32_t dr = D.side[1].begin ? D.side[1].begin[dst + 1] - D.side[1].begin[dst] : 0;
        qf[0] = src;
        qr[0] = dst;
        D.ctl->mu = RT_WORD(RT_INF, RT_NIL);
        D.ctl->seed_deg[0] = (rt_word) df;
        D.ctl->seed_deg[1] = (rt_word) dr;
    }
    for (; i < D.V; i += stride) {
        D.side[0].label[i] = RT_WORD(i == src ? 0 : RT_INF, RT_NIL);
        D.side[1].label[i] = RT_WORD(i == dst ? 0 : RT_INF, RT_NIL);
        D.side[0].stamp[i] = -1;
        D.side[1].stamp[i] = -1;
        pos[i] = -1;
    }
}

// the k-th reverse slot and the k-th forward slot in the order of their (dst, src) keys are the same edge
__global__ void rt_pair_kernel(const int32_t* __restrict__ rslot, const int32_t* __restrict__ fslot, int64_t n, int32_t* __restrict__ rev2fwd) {
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < n; i += stride) rev2fwd[rslot[i]] = fslot[i];
}

// one round of side s over the grid: the rows of its queue q[0 .. n), m slots in all, cut into merge-path tiles
__global__ void __launch_bounds__(BFS_THREADS) rt_round_kernel(rt_dev D, int s, const int32_t* __restrict__ q, int64_t n, const int64_t* __restrict__ off,
                                                               int64_t m, rt_word L_other, int32_t tag, int32_t* __restrict__ next) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ uint32_t s_d[BFS_ITEMS + 2];
    __shared__ int64_t s_split[2][2];
    __shared__ int32_t s_win[BFS_ITEMS];
    __shared__ unsigned int s_nwin, s_low;
    __shared__ rt_word s_deg, s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    const rt_side& S = D.side[s];
    const rt_side& O = D.side[1 - s];
    if (tid == 0) {
        s_nwin = 0;
        s_low = RT_NIL;
        s_deg = 0;
    }
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.begin, q, n, off, m, s_off, s_row, [&](int i, int32_t v, bool in) {
        s_d[i] = in ? (uint32_t) (rt_load(&S.label[v]) >> 32) : 0u;   // the current distance (a later drop queues v again)
    });
    rt_word degs = 0;
    uint32_t low = RT_NIL;
    for (int64_t base = t.e0; base < t.e1; base += BFS_THREADS) {   // (workgroup-uniform trip count)
        const int64_t x = base + tid;
        const bool on = x < t.e1;
        uint32_t d = 0;
        int32_t e = 0;
        if (on) {
            const int lo = frontier_slot(s_off, nv, x);
            d = s_d[lo];
            e = (int32_t) ((int64_t) s_row[lo] + (x - s_off[lo]));
        }
        int32_t v = 0, dg = 0;
        const bool won = rt_relax(S, O, D.ctl, on, d, e, L_other, tag, &v, &dg, &low);
        degs += (rt_word) dg;
        wave_append(won, v, s_win, &s_nwin, lane);
    }
    degs = wave_sum(degs);
    low = wave_min(low);
    if (lane == 0) {
        if (degs) atomicAdd(&s_deg, degs);
        if (low != RT_NIL) atomicMin(&s_low, low);
    }
    __syncthreads();
    frontier_flush(s_win, s_nwin, &D.ctl->nnext, next, &s_base, [&] {
        if (s_deg) atomicAdd(&D.ctl->mnext, s_deg);
        if (s_low != RT_NIL) atomicMax(&D.ctl->linv, 0x100000000ull - (rt_word) s_low);
    });
}

// ------------------------------------------------------------------ the tail: one workgroup runs rounds of both sides in one launch
struct rt_tail_args {
    int32_t* q[2][2];        // [side][0]: the side's queue, [side][1]: its other buffer
    int64_t n[2], m[2];
    rt_word L[2];
    int64_t tail_from;
    int32_t tag;
    int32_t both;            // 0: the reverse side is never expanded
};

// Runs rounds until a queue is empty, L_F + L_R >= cost(mu), or the side to expand holds more than tail_from slots (the
// grid takes over).  A queue is plain stores of this workgroup, visible to its waves behind the barrier; its rows are
// walked by tail_rows (gmx_frontier.h).  Every round but a side's last lowers a label, and each is a bounded loop: no waiting on anybody.
__global__ void __launch_bounds__(RT_TAIL_THREADS) rt_tail_kernel(rt_dev D, rt_tail_args A) {
    __shared__ unsigned int s_nnext, s_low;
    __shared__ rt_word s_mnext;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = blockDim.x >> 6;
    if (tid == 0) {
        s_nnext = 0;
        s_low = RT_NIL;
        s_mnext = 0;
    }
    __syncthreads();
    rt_word slots[2] = {0, 0}, queued = 0;
    int32_t rounds[2] = {0, 0};
    int32_t tag = A.tag;
    for (int32_t it = 0; it < RT_TAIL_MAX_ROUNDS; it++) {   // (everything the loop branches on is workgroup-uniform)
        const rt_word muc = rt_load(&D.ctl->mu) >> 32;
        if (A.n[0] == 0 || (A.both && A.n[1] == 0)) break;
        if (A.L[0] + (A.both ? A.L[1] : 0ull) >= muc) break;
        const int s = A.both && A.m[1] < A.m[0] ? 1 : 0;
        if (A.m[s] > A.tail_from) break;
        const rt_side S = D.side[s];   // (a copy: through a reference into the arguments every slot step reloaded S.label)
        const rt_side& O = D.side[1 - s];
        const rt_word L_other = A.both ? A.L[1 - s] : 0ull;
        const int32_t* la = A.q[s][0];
        int32_t* lb = A.q[s][1];
        const int64_t n = A.n[s];
        rt_word degs = 0;
        uint32_t low = RT_NIL;
        const auto slot = [&](bool on, uint32_t d, int32_t e) {
            int32_t v = 0, dg = 0;
            const bool won = rt_relax(S, O, D.ctl, on, d, e, L_other, tag, &v, &dg, &low);
            degs += (rt_word) dg;
            wave_append(won, v, lb, &s_nnext, lane);
        };
        const auto load = [&](bool have, int32_t v, int32_t) { return have ? (uint32_t) (rt_load(&S.label[v]) >> 32) : 0u; };
        tail_rows<RT_TAIL_LANE>(la, n, S.begin, lane, wave, nwaves, load, slot);
        degs = wave_sum(degs);
        low = wave_min(low);
        if (lane == 0) {
            if (degs) atomicAdd(&s_mnext, degs);
            if (low != RT_NIL) atomicMin(&s_low, low);
        }
        __syncthreads();
        slots[s] += (rt_word) A.m[s];
        rounds[s]++;
        A.n[s] = (int64_t) s_nnext;
        A.m[s] = (int64_t) s_mnext;
        A.L[s] = s_low == RT_NIL ? (rt_word) RT_INF : (rt_word) s_low;
        queued += (rt_word) s_nnext;
        A.q[s][0] = lb;
        A.q[s][1] = (int32_t*) la;
        tag++;
        __syncthreads();
        if (tid == 0) {
            s_nnext = 0;
            s_low = RT_NIL;
            s_mnext = 0;
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int s = 0; s < 2; s++) {
            D.ctl->tail_n[s] = (rt_word) A.n[s];
            D.ctl->tail_m[s] = (rt_word) A.m[s];
            D.ctl->tail_L[s] = A.L[s];
            D.ctl->tail_rounds[s] = (rt_word) rounds[s];
            D.ctl->tail_slots[s] = slots[s];
        }
        D.ctl->tail_queued = queued;
    }
}

// ------------------------------------------------------------------ the route, by one wave
// the row that holds slot e: the last one that starts at or before it (the empty rows before it start there too); a
// 64-way search, one probe per lane
__device__ __forceinline__ int32_t rt_row_of(const int32_t* __restrict__ begin, int64_t V, uint32_t e, int lane) {
    int64_t lo = 0, hi = V;   // the row lies in [lo, hi)
    while (hi - lo > 1) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t at = lo + (int64_t) lane * step;
        const bool le = at < hi && (uint32_t) begin[at] <= e;
        const int cnt = __popcll(__ballot(le));   // (begin never decreases: the lanes that say yes are the first cnt; lane 0 does)
        lo += (int64_t) (cnt > 0 ? cnt - 1 : 0) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return (int32_t) lo;
}

// From mu's vertex m: R's slots on to dst (rn / re: vertex and uploaded forward slot per edge, pos[v] = edges from m), then F's
// slots back to src (tn / te).  Where the backward walk meets a vertex of the forward one again (a zero-weight loop between
// the two chains) the route changes over at the one nearest src.  out_n / out_e [V]: the route from src; ctl->hops.
__global__ void __launch_bounds__(64) rt_extract_kernel(rt_dev D, const int32_t* __restrict__ order /* device forward slot -> uploaded, NULL: same */,
                                                        const int32_t* __restrict__ r2u /* reverse slot -> uploaded forward slot */,
                                                        int32_t* __restrict__ pos, int32_t* __restrict__ rn, int32_t* __restrict__ re,
                                                        int32_t* __restrict__ tn, int32_t* __restrict__ te, int32_t* __restrict__ out_n,
                                                        int32_t* __restrict__ out_e) {
    const int lane = threadIdx.x;
    const rt_word mu = D.ctl->mu;
    const int32_t m = (int32_t) (uint32_t) mu;
    int64_t hr = 0, k = 0, kstart = 0;
    int32_t v = m, xstar = m;
    bool bad = false;
    if (lane == 0) pos[m] = 0;
    for (;;) {
        const uint32_t e = (uint32_t) D.side[1].label[v];
        if (e == RT_NIL) break;
        if (hr >= D.V) { bad = true; break; }
        v = rt_row_of(D.side[1].begin, D.V, e, lane);
        if (lane == 0) {
            rn[hr] = v;
            re[hr] = r2u[e];
            pos[v] = (int32_t) (hr + 1);
        }
        hr++;
    }
    __threadfence();   // (one wave: pos[] below is read by lane 0, which wrote it)
    v = m;
    for (;;) {
        const uint32_t e = (uint32_t) D.side[0].label[v];
        if (e == RT_NIL) break;
        if (k >= D.V) { bad = true; break; }
        if (lane == 0) {
            tn[k] = v;
            te[k] = order ? order[e] : (int32_t) e;
        }
        k++;
        v = rt_row_of(D.side[0].begin, D.V, e, lane);
        const int32_t p = __shfl(lane == 0 ? pos[v] : 0, 0, 64);
        if (p >= 0) {
            xstar = v;
            kstart = k;
        }
    }
    const int64_t hf = k - kstart;
    const int64_t p0 = __shfl(lane == 0 ? (int64_t) pos[xstar] : 0ll, 0, 64);
    for (int64_t j = lane; j < hf; j += 64) {
        out_n[j] = tn[k - 1 - j];
        out_e[j] = te[k - 1 - j];
    }
    if (hf + (hr - p0) > D.V) bad = true;   // (a route is simple: never)
    for (int64_t j = p0 + lane; j < hr && !bad; j += 64) {
        out_n[hf + (j - p0)] = rn[j];
        out_e[hf + (j - p0)] = re[j];
    }
    if (lane == 0) {
        D.ctl->hops = (rt_word) (hf + (hr - p0));
        D.ctl->bad = bad ? 1ull : 0ull;
    }
}

// ------------------------------------------------------------------ host
struct gmx_route {
    gmx_graph* g = nullptr;
    bool has_reverse = false;
    dbuf<int32_t> w_up, w_f, w_r, r2u;           // weights by uploaded slot (only while they differ from w_f), by forward and by reverse slot
    dbuf<rt_word> label[2];
    dbuf<int32_t> stamp[2], pos, q[2][2], out_n, out_e;
    dbuf<rt_ctl> ctl;
    frontier_scan fs;
    gmx_pinned<rt_ctl> h_ctl;
    double h2d_ms = 0;
};

// rev2fwd[j] = the device forward slot that reverse slot j stands for: both CSRs' slots sorted (stably) by (dst << 32 | src)
// pair up in order, whatever order the rows are stored in; a reverse CSR with sorted rows is in that order already
static int rt_reverse_map(const gmx_graph* g, int32_t* rev2fwd) {
    gmx_ws_scope ws;
    const size_t E = (size_t) g->E;
    const unsigned end_bit = 32 + (unsigned) gmx_bits_for(g->V);
    wbuf<uint64_t> keys, keys2;
    wbuf<int32_t> val, fslot, rslot;
    wbuf<char> tmp;
    GMX_CHECK(keys.alloc(E));
    GMX_CHECK(keys2.alloc(E));
    GMX_CHECK(val.alloc(E));
    GMX_CHECK(fslot.alloc(E));
    GMX_CHECK(rslot.alloc(E));
    size_t tb = 0;
    GMX_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys.p, keys2.p, val.p, fslot.p, E, 0u, end_bit, 0));
    GMX_CHECK(tmp.alloc(tb));
    hipLaunchKernelGGL(iota_kernel, dim3(grid_for(g->E)), dim3(RT_THREADS), 0, 0, val.p, g->E);
    GMX_CHECK(gmx_keys_from_csr(g->begin.p, g->node_idx.p, g->V, g->E, true, nullptr, keys.p, 0));
    GMX_HIP(rocprim::radix_sort_pairs((void*) tmp.p, tb, keys.p, keys2.p, val.p, fslot.p, E, 0u, end_bit, 0));
    if (g->r_rows_sorted) {
        hipLaunchKernelGGL(iota_kernel, dim3(grid_for(g->E)), dim3(RT_THREADS), 0, 0, rslot.p, g->E);
    } else {
        GMX_CHECK(gmx_keys_from_csr(g->r_begin.p, g->r_node_idx.p, g->V, g->E, false, nullptr, keys.p, 0));
        GMX_HIP(rocprim::radix_sort_pairs((void*) tmp.p, tb, keys.p, keys2.p, val.p, rslot.p, E, 0u, end_bit, 0));
    }
    hipLaunchKernelGGL(rt_pair_kernel, dim3(grid_for(g->E)), dim3(RT_THREADS), 0, 0, (const int32_t*) rslot.p, (const int32_t*) fslot.p, g->E, rev2fwd);
    GMX_HIP(hipGetLastError());
    return GMX_OK;
}

static int rt_create(gmx_route* r, gmx_graph* g, const int32_t* weight_host) {
    const size_t V = (size_t) g->V, E = (size_t) g->E;
    r->g = g;
    r->has_reverse = g->has_reverse;
    GMX_CHECK(r->ctl.alloc(1));
    GMX_CHECK(r->h_ctl.alloc(1));
    if (V == 0) return GMX_OK;   // no vertex to ask for: every query is refused
    GMX_CHECK(r->w_f.alloc(E));
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.H2D));
    GMX_HIP(hipMemsetAsync(r->ctl.p, 0, sizeof(rt_ctl), 0));
    if (E) {
        // the weights: copied in, checked on the device copy, brought into the order of the sorted rows when the upload sorted them
        int32_t* up = r->w_f.p;
        if (g->e_idx2idx.p) {
            GMX_CHECK(r->w_up.alloc(E));
            up = r->w_up.p;
        }
        GMX_HIP(hipMemcpyAsync(up, weight_host, sizeof(int32_t) * E, hipMemcpyHostToDevice, 0));
        hipLaunchKernelGGL((first_bad_slot_kernel<int32_t, rt_ctl>), dim3(grid_for(g->E, RT_THREADS)), dim3(RT_THREADS), 0, 0, (const int32_t*) up, g->E, r->ctl.p);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(r->h_ctl, r->ctl.p));
        if (r->h_ctl.p->bad) {
            const int64_t at = g->E - (int64_t) r->h_ctl.p->bad;
            gmx_set_error("route: weight[%lld] = %d is negative: every weight must be >= 0", (long long) at, (int) weight_host[at]);
            return GMX_ERR_ARG;
        }
        if (g->e_idx2idx.p) {
            hipLaunchKernelGGL(gather_by_order_kernel<int32_t>, dim3(grid_for(g->E, RT_THREADS)), dim3(RT_THREADS), 0, 0, (const int32_t*) up, (const int32_t*) g->e_idx2idx.p,
                               g->E, r->w_f.p);
            GMX_HIP(hipGetLastError());
            GMX_HIP(hipStreamSynchronize(0));
            r->w_up.release();
        }
        if (r->has_reverse) {
            // the reverse side: its weights, and per reverse slot the uploaded forward slot (r2u first holds the device forward slot)
            GMX_CHECK(r->w_r.alloc(E));
            GMX_CHECK(r->r2u.alloc(E));
            GMX_CHECK(rt_reverse_map(g, r->r2u.p));
            hipLaunchKernelGGL(gather_by_order_kernel<int32_t>, dim3(grid_for(g->E, RT_THREADS)), dim3(RT_THREADS), 0, 0, (const int32_t*) r->w_f.p, (const int32_t*) r->r2u.p,
                               g->E, r->w_r.p);
            if (g->e_idx2idx.p) {
                dbuf<int32_t> dev_slot;
                GMX_CHECK(dev_slot.alloc(E));
                GMX_HIP(hipMemcpyAsync(dev_slot.p, r->r2u.p, sizeof(int32_t) * E, hipMemcpyDeviceToDevice, 0));
                hipLaunchKernelGGL(gather_by_order_kernel<int32_t>, dim3(grid_for(g->E, RT_THREADS)), dim3(RT_THREADS), 0, 0, (const int32_t*) g->e_idx2idx.p,
                                   (const int32_t*) dev_slot.p, g->E, r->r2u.p);
                GMX_HIP(hipGetLastError());
                GMX_HIP(hipStreamSynchronize(0));
            }
            GMX_HIP(hipGetLastError());
        }
    }
    GMX_CHECK(tm.end(tm.H2D));
    for (int s = 0; s < 2; s++) {
        GMX_CHECK(r->label[s].alloc(V));
        GMX_CHECK(r->stamp[s].alloc(V));
        GMX_CHECK(r->q[s][0].alloc(V));
        GMX_CHECK(r->q[s][1].alloc(V));
    }
    GMX_CHECK(r->pos.alloc(V));
    GMX_CHECK(r->out_n.alloc(V));
    GMX_CHECK(r->out_e.alloc(V));
    GMX_CHECK(gmx_frontier_scan_alloc(&r->fs, V, 0));
    gmx_stats_t up{};
    GMX_CHECK(tm.finish(&up));
    r->h2d_ms = up.h2d_ms;
    return GMX_OK;
}

extern "C" int gmx_route_create(gmx_graph_t* g, const int32_t* weight_host, gmx_route_t** out) {
    GMX_REQUIRE(g && out, "NULL argument");
    *out = nullptr;
    GMX_REQUIRE(weight_host || g->E == 0, "route: weight is NULL");
    gmx_route* r = new gmx_route;
    const int rc = rt_create(r, g, weight_host);
    if (rc != GMX_OK) {
        delete r;
        return rc;
    }
    *out = r;
    return GMX_OK;
}

extern "C" int gmx_route_free(gmx_route_t* r) {
    delete r;
    return GMX_OK;
}

extern "C" int gmx_route_query(gmx_route_t* r, gmx_node_t src, gmx_node_t dst, int32_t* found, int64_t* cost, gmx_node_t* path_node,
                               gmx_edge_t* path_edge, int64_t cap, int64_t* hops, gmx_stats_t* stats) {
    GMX_REQUIRE(r && found && cost && hops, "NULL argument");
    GMX_REQUIRE(cap >= 0, "route: cap = %lld is negative", (long long) cap);
    const gmx_graph* g = r->g;
    const int64_t V = g->V, E = g->E;
    GMX_REQUIRE(src >= 0 && src < V, "route: src = %d is not a vertex of [0, %lld)", (int) src, (long long) V);
    GMX_REQUIRE(dst >= 0 && dst < V, "route: dst = %d is not a vertex of [0, %lld)", (int) dst, (long long) V);
    if (stats) memset(stats, 0, sizeof(*stats));
    const int64_t tail_from = gmx_env_int("GMX_ROUTE_TAIL", RT_TAIL, 0, INT32_MAX);   // the knobs are read at every call; flag and cost do not depend on them
    const int64_t log = gmx_env_int("GMX_ROUTE_LOG", 0, 0, INT32_MAX);
    const char* sides = getenv("GMX_ROUTE_SIDES");
    const bool both = r->has_reverse && !(sides && !strcmp(sides, "forward"));
    const double t_start = gmx_tick::now();
    if (src == dst) {   // the empty route (bidir_dijkstra.gm looks for a cycle here: gmx.h)
        *found = 1;
        *cost = 0;
        *hops = 0;
        if (log >= 1)
            fprintf(stderr, "gmx route: V %lld E %lld src %d dst %d sides %s; tail %lld; rounds F 0 grid + 0 tail, R 0 grid + 0 tail in 0 launches; "
                            "slots F 0 R 0; queued 0; found 1 cost 0 meet %d hops 0; ms %.3f\n",
                    (long long) V, (long long) E, (int) src, (int) dst, both ? "both" : "forward", (long long) tail_from, (int) src,
                    (gmx_tick::now() - t_start) * 1e3);
        return GMX_OK;
    }
    gmx_spans tm;

    rt_dev D;
    D.side[0] = rt_side{g->begin.p, g->node_idx.p, r->w_f.p, r->label[0].p, r->stamp[0].p};
    D.side[1] = rt_side{r->has_reverse ? g->r_begin.p : nullptr, r->has_reverse ? g->r_node_idx.p : nullptr, r->w_r.p, r->label[1].p, r->stamp[1].p};
    D.ctl = r->ctl.p;
    D.V = V;
    const rt_ctl* h = r->h_ctl.p;

    GMX_CHECK(tm.begin(tm.KERNEL));
    hipLaunchKernelGGL(rt_init_kernel, dim3(grid_for(V, RT_THREADS)), dim3(RT_THREADS), 0, 0, D, (int32_t) src, (int32_t) dst, r->pos.p, r->q[0][0].p, r->q[1][0].p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_read_back(r->h_ctl, r->ctl.p));
    int32_t* q[2][2] = {{r->q[0][0].p, r->q[0][1].p}, {r->q[1][0].p, r->q[1][1].p}};   // [side][0]: the side's queue
    int64_t m[2] = {(int64_t) h->seed_deg[0], (int64_t) h->seed_deg[1]};
    int64_t n[2] = {m[0] > 0 ? 1 : 0, m[1] > 0 ? 1 : 0};
    rt_word L[2] = {0, 0};
    int64_t slots[2] = {0, 0}, queued = n[0] + (both ? n[1] : 0);
    int32_t grid_rounds[2] = {0, 0}, tail_rounds[2] = {0, 0}, tail_launches = 0, tag = 0;
    rt_word mu = h->mu;
    for (;;) {
        if (n[0] == 0 || (both && n[1] == 0)) break;
        if (L[0] + (both ? L[1] : 0ull) >= (mu >> 32)) break;
        const int s = both && m[1] < m[0] ? 1 : 0;   // the side whose queue holds fewer slots
        if (tail_from > 0 && m[s] <= tail_from) {    // one workgroup, until a queue outgrows it
            rt_tail_args A;
            for (int x = 0; x < 2; x++) {
                A.q[x][0] = q[x][0];
                A.q[x][1] = q[x][1];
                A.n[x] = n[x];
                A.m[x] = m[x];
                A.L[x] = L[x];
            }
            A.tail_from = tail_from;
            A.tag = tag;
            A.both = both ? 1 : 0;
            hipLaunchKernelGGL(rt_tail_kernel, dim3(1), dim3(RT_TAIL_THREADS), 0, 0, D, A);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(r->h_ctl, r->ctl.p));
            tail_launches++;
            for (int x = 0; x < 2; x++) {
                const int32_t ran = (int32_t) h->tail_rounds[x];
                n[x] = (int64_t) h->tail_n[x];
                m[x] = (int64_t) h->tail_m[x];
                L[x] = h->tail_L[x];
                tail_rounds[x] += ran;
                slots[x] += (int64_t) h->tail_slots[x];
                tag += ran;
                if (ran & 1) { int32_t* t = q[x][0]; q[x][0] = q[x][1]; q[x][1] = t; }
            }
            queued += (int64_t) h->tail_queued;
            GMX_REQUIRE(h->tail_rounds[0] + h->tail_rounds[1] > 0 || h->mu != mu, "route: the tail launch ran no round");
        } else {
            GMX_HIP(hipMemsetAsync(&r->ctl.p->nnext, 0, 3 * sizeof(rt_word), 0));   // nnext, mnext, linv
            GMX_CHECK(gmx_frontier_offsets(D.side[s].begin, q[s][0], n[s], &r->fs, nullptr, false));
            const int64_t nb = frontier_tiles(n[s], m[s]);
            hipLaunchKernelGGL(rt_round_kernel, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, D, s, (const int32_t*) q[s][0], n[s],
                               (const int64_t*) r->fs.off.p, m[s], both ? L[1 - s] : 0ull, tag, q[s][1]);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(r->h_ctl, r->ctl.p));
            grid_rounds[s]++;
            slots[s] += m[s];
            tag++;
            n[s] = (int64_t) h->nnext;
            m[s] = (int64_t) h->mnext;
            L[s] = h->linv ? 0x100000000ull - h->linv : (rt_word) RT_INF;
            queued += n[s];
            { int32_t* t = q[s][0]; q[s][0] = q[s][1]; q[s][1] = t; }
        }
        mu = h->mu;
    }
    const bool hit = (uint32_t) (mu >> 32) != RT_INF;
    int64_t nhops = 0;
    if (hit) {
        hipLaunchKernelGGL(rt_extract_kernel, dim3(1), dim3(64), 0, 0, D, (const int32_t*) g->e_idx2idx.p, (const int32_t*) r->r2u.p, r->pos.p, q[1][0], q[1][1],
                           q[0][0], q[0][1], r->out_n.p, r->out_e.p);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(r->h_ctl, r->ctl.p));
        GMX_REQUIRE(h->bad == 0, "route: a predecessor chain did not end");
        nhops = (int64_t) h->hops;
    }
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.begin(tm.D2H));
    const int64_t ncopy = nhops < cap ? nhops : cap;
    if (ncopy > 0 && path_node) GMX_HIP(hipMemcpyAsync(path_node, r->out_n.p, sizeof(int32_t) * (size_t) ncopy, hipMemcpyDeviceToHost, 0));
    if (ncopy > 0 && path_edge) GMX_HIP(hipMemcpyAsync(path_edge, r->out_e.p, sizeof(int32_t) * (size_t) ncopy, hipMemcpyDeviceToHost, 0));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));   // (the path has landed)
    *found = hit ? 1 : 0;
    if (hit) *cost = (int64_t) (mu >> 32);
    *hops = nhops;
    if (stats) {
        stats->iterations = grid_rounds[0] + grid_rounds[1] + tail_rounds[0] + tail_rounds[1];
        stats->edges_examined = slots[0] + slots[1];
        stats->vertices_reached = queued;
    }
    if (log >= 1)   // one line per query (tools/route_prof.py and the tests parse it)
        fprintf(stderr, "gmx route: V %lld E %lld src %d dst %d sides %s; tail %lld; rounds F %d grid + %d tail, R %d grid + %d tail in %d launches; "
                        "slots F %lld R %lld; queued %lld; found %d cost %lld meet %d hops %lld; ms %.3f\n",
                (long long) V, (long long) E, (int) src, (int) dst, both ? "both" : "forward", (long long) tail_from, grid_rounds[0], tail_rounds[0],
                grid_rounds[1], tail_rounds[1], tail_launches, (long long) slots[0], (long long) slots[1], (long long) queued, hit ? 1 : 0,
                hit ? (long long) (mu >> 32) : -1ll, hit ? (int) (uint32_t) mu : -1, (long long) nhops, (gmx_tick::now() - t_start) * 1e3);
    return GMX_OK;
}

extern "C" int gmx_bidir_dijkstra(gmx_graph_t* g, const int32_t* weight_host, gmx_node_t src, gmx_node_t dst, gmx_node_t* parent_host,
                                  gmx_edge_t* parent_edge_host, int32_t* found, gmx_stats_t* stats) {
    GMX_REQUIRE(g && parent_host && found, "NULL argument");
    GMX_REQUIRE(weight_host || g->E == 0, "route: weight is NULL");
    if (stats) memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V;
    if (V == 0) {
        *found = 0;
        return GMX_OK;
    }
    GMX_REQUIRE(src >= 0 && src < V, "route: src = %d is not a vertex of [0, %lld)", (int) src, (long long) V);
    GMX_REQUIRE(dst >= 0 && dst < V, "route: dst = %d is not a vertex of [0, %lld)", (int) dst, (long long) V);
    gmx_route* r = nullptr;
    GMX_CHECK(gmx_route_create(g, weight_host, &r));
    std::vector<gmx_node_t> pn((size_t) V);
    std::vector<gmx_edge_t> pe((size_t) V);
    int32_t hit = 0;
    int64_t cost = 0, hops = 0;
    gmx_stats_t st;
    const int rc = gmx_route_query(r, src, dst, &hit, &cost, pn.data(), pe.data(), V, &hops, &st);
    const double h2d_ms = r->h2d_ms;
    gmx_route_free(r);
    GMX_CHECK(rc);
    for (int64_t v = 0; v < V; v++) parent_host[v] = -1;
    if (parent_edge_host)
        for (int64_t v = 0; v < V; v++) parent_edge_host[v] = -1;
    gmx_node_t from = src;
    for (int64_t k = 0; k < hops; k++) {   // the route is simple: every vertex gets one predecessor
        parent_host[pn[(size_t) k]] = from;
        if (parent_edge_host) parent_edge_host[pn[(size_t) k]] = pe[(size_t) k];
        from = pn[(size_t) k];
    }
    *found = hit;
    if (stats) {
        *stats = st;
        stats->h2d_ms = h2d_ms;
    }
    return GMX_OK;
}

void gmx_touch_route() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) rt_tail_kernel);
}
