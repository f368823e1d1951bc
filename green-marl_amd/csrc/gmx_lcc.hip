// gmx_lcc.hip -- per-vertex triangle counts and local clustering coefficients for gfx950: gmx_clustering.
//
// The stored slots are read as an undirected simple graph: N(v) = { u != v : v -> u or u -> v is stored }, deg = |N|,
//     tri[v] = #{ unordered {u, w} in N(v) : w in N(u) },   lcc[v] = 2 tri[v] / (deg[v] (deg[v] - 1)).
// Plan: gmx_tcd.hip's (tcd_plan_get, cached on the graph and shared with gmx_triangle_counting_directed): perm, the
// ascending-|N| renumbering, and UP', per vertex the distinct neighbours above it in that numbering, sorted.  Every
// triangle is then found exactly once, as v < u < w with u, w in UP'(v) and w in UP'(u).  On top of the plan, on the first
// call: the 64-slot groups of the UP' rows and UP' among the H highest ids as an H x H bit matrix (every upper neighbour of
// one of them is one of them; with the degree order they are the hubs, as in gmx_tc.hip).
//
// Count: tc_oriented_kernel's walk (gmx_tc.hip) on UP', on the work loop and the searches of gmx_rowgroup.h.  A work item is (v, group of 64 slots of UP'(v)), claimed from a
// counter; UP'(v) from the group's first slot on is staged in the wave's LDS slice (at most `cap` entries; longer ones are
// searched in memory).  Lane i owns the slot u = A[i]; its sides are the tail A(i, da) and UP'(u).  A side of at most `alone`
// entries is walked by the lane itself; the other slots are taken one after the other by the whole wave, which probes the
// hub matrix once per tail entry (u a hub), streams UP'(u) in coalesced pieces and searches the tail (|UP'(u)| <= ratio *
// |tail|), or streams the tail and searches UP'(u) in memory.
//
// Credits: where the counting kernels add one to a total, every match (v, u, w) here goes to its three corners, without
// three scattered global atomics per triangle:
//   u   the slot's count: a register of the lane that owns the slot (a slot the wave takes counts with ballots, and the
//       owner takes the sum); at most one 64-bit atomic per slot, at the item's end;
//   v   the sum of the item's slot counts: one wave reduction and one atomic per work item;
//   w   in every regime w is found as a POSITION p of the tail (the list search's result, the tail walk's index, the bit
//       probe's tail entry), so the credit goes to a per-position counter in LDS and the item flushes the non-zero ones,
//       one atomic each (u's credit rides on the flush of its own position).  UP'(u) holds distinct values, so a position gets at most one credit per slot of the group: a
//       counter holds at most 64 and four of them share a 32-bit word (a byte each, which never carries).  That is 1 KiB
//       per wave next to the 4 KiB list: 20 KiB per workgroup, 8 workgroups and 32 waves per CU in the 160 KiB of LDS (with
//       a word per position it would be 20 waves per CU, which doubled tc_oriented_kernel's time: gmx_tc.hip).
//       Items searched in memory credit tri[w] with a global atomic per match.
// Integers only: tri, deg, lcc (one IEEE division of two exact integers per vertex), triangles and wedges are exact and the
// same bytes from run to run and under every knob.
#include "gmx_tcd_plan.h"
#include "gmx_rowgroup.h"
#include "gmx_frontier.h"

#define LCC_THREADS 256
#define LCC_WAVES 4
#define LCC_CLAIM 8      // work items per dequeue
#define LCC_PIECES 4     // 256-byte pieces of UP'(u) a wave keeps in flight
// Taken over from gmx_tc.hip's TCO_* (the same walk) and swept with tools/lcc_prof.py --sweep on directed RMAT-20 only
// (DESIGN.md 4.2q): no default moved.  NOT MEASURED: RMAT-22, permuted and symmetrised graphs, and LCC_CLAIM and LCC_PIECES above.
#define LCC_ALONE 4      // a lane walks a side of up to this many entries by itself (0 .. 8 flat; 16: +2 %, 48: +6 %)
#define LCC_RATIO 4      // stream UP'(u) and search the tail while |UP'(u)| <= LCC_RATIO * |tail| (1 .. 64 flat)
#define LCC_HUB_TAIL 4   // against a hub u the tail is the side to walk while it is at most this many times |UP'(u)| (2 .. 64 flat; 1: +22 %)
#define LCC_CAP 1024     // list entries staged per wave (4 KiB), and positions counted per wave (1 KiB) (512: +19 %, 256: 5 x)
#define LCC_CAP_MIN 64
#define LCC_HUB_MAX 131072   // gmx_tc.hip's TCO_HUB_MAX: hubs of the bit matrix (half of that up to 2^24 vertices)

enum {
    LCC_NEXT, LCC_STAGED, LCC_MEMORY, LCC_SLOT_ALONE, LCC_SLOT_LIST, LCC_SLOT_TAIL, LCC_SLOT_HUB, LCC_SLOT_EMPTY, LCC_CREDIT_LDS,
    LCC_CREDIT_GLOBAL, LCC_SUM_TRI, LCC_WEDGES, LCC_NONZERO, LCC_NCTR
};

// ------------------------------------------------------------------ the hubs' bit matrix
// One wave per hub row u = base + row: every w of UP'(u) is > u >= base, so it has a bit in the row.
__global__ void lcc_hub_bits_kernel(const int32_t* __restrict__ up_begin, const int32_t* __restrict__ up_idx, int64_t base, int64_t H,
                                    uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= H) return;
    const int64_t u = base + row;
    uint32_t* dst = bits + row * (H >> 5);
    for (int32_t p = up_begin[u] + lane; p < up_begin[u + 1]; p += 64) {
        const int64_t w = up_idx[p] - base;   // in (row, H)
        atomicOr(&dst[w >> 5], 1u << (w & 31));
    }
}

// ------------------------------------------------------------------ count kernel
struct lcc_tally {   // what GMX_LCC_LOG reports: counted where the decisions are taken, per wave (the same in every lane)
    unsigned int alone = 0, empty = 0, list = 0, tail = 0, hub = 0;
};

// the credit of w, found at position p of R.  COUNTERS: the byte of position p among the wave's packed LDS counters, byte
// p / 256 of word p % 256: the lanes of a tail walk hold consecutive positions, which are then consecutive words (with four
// neighbours in a word their atomics hit one address: RMAT-22 45.5 -> 22.5 ms)
static_assert(LCC_CAP == 1024, "the position counters are four bytes of 256 words");
template <bool COUNTERS>
__device__ __forceinline__ void lcc_credit_w(uint32_t* cnt, unsigned long long* __restrict__ tri, int32_t p, int32_t w) {
    if (COUNTERS) atomicAdd(&cnt[p & 255], 1u << (8 * (p >> 8)));
    else atomicAdd(&tri[w], 1ull);
}

// One work item: R[0, da) is UP'(v) from the group's first slot on (LDS: the wave's slice; otherwise the row in memory), the
// group's slots are R[0 .. 63], one per lane.  COUNTERS (only with LDS): the w credits go to cnt[], which is all zero on
// entry and on return.  Returns the item's matches (the same in every lane).
template <bool LDS, bool COUNTERS>
__device__ __forceinline__ unsigned long long lcc_item(const int32_t* R, uint32_t* cnt, int32_t da, int32_t v, const int32_t* __restrict__ up_begin,
                                                       const int32_t* __restrict__ up_idx, unsigned long long* __restrict__ tri,
                                                       const uint32_t* __restrict__ hub_bits, int32_t hub_base /* V: no hubs */, int hub_words,
                                                       int hub_tail, int lane, int alone_max, int ratio, lcc_tally& t) {
    const bool act = lane + 1 < da;
    int32_t bb = 0, be = 0, u = 0;
    if (act) {
        u = R[lane];
        bb = up_begin[u];
        be = up_begin[u + 1];
    }
    const int32_t db = be - bb, ta = act ? da - (lane + 1) : 0;
    // the side to walk: the tail of UP'(v) above u, or UP'(u).  Against a hub u a tail entry costs one bit probe, so the tail
    // is the side unless it is far the longer one
    const bool hubu = act && u >= hub_base;
    const bool tail_side = hubu ? (long long) ta <= (long long) hub_tail * db : ta < db;
    const int32_t shorter = db == 0 || ta == 0 ? 0 : (tail_side ? ta : db);
    unsigned int cu = 0;   // the slot's matches: u's credit
    t.empty += (unsigned int) __popcll(__ballot(act && shorter == 0));
    t.alone += (unsigned int) __popcll(__ballot(act && shorter > 0 && shorter <= alone_max));
    if (act && shorter > 0 && shorter <= alone_max) {
        if (tail_side && hubu) {
            const uint32_t* hrow = hub_bits + (int64_t) (u - hub_base) * hub_words;
#pragma unroll 1   // (at most alone_max short steps: unrolled by four with a remainder, as the compiler does it inside rg_items' flat loop, GMX_LCC_PLAIN=1 was 0.4 % slower)
            for (int32_t p = lane + 1; p < da; p++) {
                const int32_t w = R[p], wh = w - hub_base;   // w > u >= hub_base
                if ((hrow[wh >> 5] >> (wh & 31)) & 1u) {
                    cu++;
                    lcc_credit_w<COUNTERS>(cnt, tri, p, w);
                }
            }
        } else if (!tail_side) {
#pragma unroll 1   // (as above: by two with a remainder otherwise)
            for (int32_t p = bb; p < be; p++) {
                const int32_t w = up_idx[p];
                const int32_t f = rg_lower_bound<LDS>(R, lane + 1, da, w);
                if (f < da && R[f] == w) {
                    cu++;
                    lcc_credit_w<COUNTERS>(cnt, tri, f, w);
                }
            }
        } else {
            for (int32_t p = lane + 1; p < da; p++) {
                const int32_t w = R[p];
                if (rg_contains<false>(up_idx, bb, be, w)) {
                    cu++;
                    lcc_credit_w<COUNTERS>(cnt, tri, p, w);
                }
            }
        }
    }
    // the other slots, one after the other by the whole wave.  Every loop below has the same trip count in all lanes, so the
    // ballots see the whole wave and `sc`, the slot's matches, is the same in every lane
    unsigned long long m = __ballot(act && shorter > alone_max);
    while (m) {
        const int src = __builtin_ctzll(m);
        m &= m - 1;
        const int32_t sbb = __builtin_amdgcn_readlane(bb, src), sbe = __builtin_amdgcn_readlane(be, src), su = __builtin_amdgcn_readlane(u, src);
        const int32_t sdb = sbe - sbb, sta = da - (src + 1);
        unsigned int sc = 0;
        if (su >= hub_base && (long long) sta <= (long long) hub_tail * sdb) {   // a hub: one bit probe per tail entry
            t.hub++;
            const uint32_t* srow = hub_bits + (int64_t) (su - hub_base) * hub_words;
            for (int32_t p0 = src + 1; p0 < da; p0 += 64) {
                const int32_t p = p0 + lane;
                bool hit = false;
                if (p < da) {
                    const int32_t w = R[p], wh = w - hub_base;
                    hit = (srow[wh >> 5] >> (wh & 31)) & 1u;
                    if (hit) lcc_credit_w<COUNTERS>(cnt, tri, p, w);
                }
                sc += (unsigned int) __popcll(__ballot(hit));
            }
        } else if ((long long) sdb <= (long long) ratio * sta) {                 // stream UP'(u), search the tail
            t.list++;
            for (int32_t p0 = sbb; p0 < sbe; p0 += LCC_PIECES * 64) {
                int32_t w[LCC_PIECES];
#pragma unroll
                for (int k = 0; k < LCC_PIECES; k++) {
                    const int32_t q = p0 + 64 * k + lane;
                    w[k] = q < sbe ? up_idx[q] : -1;
                }
#pragma unroll
                for (int k = 0; k < LCC_PIECES; k++) {
                    if (p0 + 64 * k >= sbe) break;   // (the same in every lane)
                    bool hit = false;
                    if (w[k] >= 0) {
                        const int32_t f = rg_lower_bound<LDS>(R, src + 1, da, w[k]);
                        hit = f < da && R[f] == w[k];
                        if (hit) lcc_credit_w<COUNTERS>(cnt, tri, f, w[k]);
                    }
                    sc += (unsigned int) __popcll(__ballot(hit));
                }
            }
        } else {                                                                 // stream the tail, search UP'(u) in memory
            t.tail++;
            for (int32_t p0 = src + 1; p0 < da; p0 += 64) {
                const int32_t p = p0 + lane;
                bool hit = false;
                if (p < da) {
                    const int32_t w = R[p];
                    hit = rg_contains<false>(up_idx, sbb, sbe, w);
                    if (hit) lcc_credit_w<COUNTERS>(cnt, tri, p, w);
                }
                sc += (unsigned int) __popcll(__ballot(hit));
            }
        }
        if (lane == src) cu = sc;
    }
    unsigned long long tot = cu;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_down(tot, off, 64);
    tot = rg_first_lane(tot);
    if (lane == 0 && tot) atomicAdd(&tri[v], tot);
    if (COUNTERS) {
        // flush the positions' counters and leave them zero.  Lane i's first word holds position i, its own slot: u's credit
        // rides on that position's atomic
        rg_lds_landed();
        if (tot) {
            unsigned int own = cu;              // (cu != 0: lane + 1 < da, so the loop below runs for k = lane)
            for (int32_t k = lane; k < da && k < LCC_CAP / 4; k += 64) {
                const uint32_t word = cnt[k];
                if (word) cnt[k] = 0;
                const unsigned int c0 = (word & 255u) + own;
                own = 0;
                if (c0) atomicAdd(&tri[R[k]], (unsigned long long) c0);
#pragma unroll
                for (int j = 1; j < 4; j++) {
                    const uint32_t c = (word >> (8 * j)) & 255u;
                    if (c) atomicAdd(&tri[R[k + 256 * j]], (unsigned long long) c);   // (a non-zero byte is a position < da)
                }
            }
        }
    } else if (cu) {
        atomicAdd(&tri[u], (unsigned long long) cu);
    }
    return tot;
}

// COUNTERS: the packed LDS counters for the w credits of staged items; false: a global atomic per match everywhere (the plain
// form they are measured against, GMX_LCC_PLAIN=1: 30 x slower on RMAT-20 and RMAT-22)
template <bool COUNTERS>
__global__ void __launch_bounds__(LCC_WAVES * 64)
lcc_count_kernel(const int32_t* __restrict__ up_begin, const int32_t* __restrict__ up_idx, const int64_t* __restrict__ grp_off, int64_t V,
                 int cap /* <= LCC_CAP */, int alone_max, int ratio, const uint32_t* __restrict__ hub_bits, int32_t hub_base, int hub_words, int hub_tail,
                 unsigned long long* __restrict__ tri /* [V], zero */, unsigned long long* __restrict__ ctr /* [LCC_NCTR] */) {
    __shared__ int32_t s_up[LCC_WAVES][LCC_CAP];
    __shared__ uint32_t s_cnt[LCC_WAVES][COUNTERS ? LCC_CAP / 4 : 1];
    const int lane = threadIdx.x & 63;
    int32_t* A = s_up[threadIdx.x >> 6];
    uint32_t* cnt = s_cnt[threadIdx.x >> 6];
    if (COUNTERS) {
        for (int k = lane; k < LCC_CAP / 4; k += 64) cnt[k] = 0;
        __builtin_amdgcn_wave_barrier();
    }
    lcc_tally t;
    unsigned int staged = 0, in_memory = 0;
    unsigned long long credit_lds = 0, credit_global = 0;
    rg_items<LCC_CLAIM>(
        grp_off, V, 0, 1, &ctr[LCC_NEXT], lane,
        [&](int32_t v, int32_t group) {
            const int32_t ab = up_begin[v] + group * 64, ae = up_begin[v + 1];
            const int32_t da = ae - ab;                 // UP'(v) from the group's first slot on (>= 2)
            if (da <= cap) {
                rg_stage(A, up_idx + ab, da, lane);
                staged++;
                const unsigned long long n = lcc_item<true, COUNTERS>(A, cnt, da, v, up_begin, up_idx, tri, hub_bits, hub_base, hub_words,
                                                                      hub_tail, lane, alone_max, ratio, t);
                if (COUNTERS) credit_lds += n; else credit_global += n;
                rg_slice_done();
            } else {
                in_memory++;
                credit_global += lcc_item<false, false>(up_idx + ab, cnt, da, v, up_begin, up_idx, tri, hub_bits, hub_base, hub_words, hub_tail,
                                                        lane, alone_max, ratio, t);
            }
        });
    if (lane == 0) {
        if (staged) atomicAdd(&ctr[LCC_STAGED], (unsigned long long) staged);
        if (in_memory) atomicAdd(&ctr[LCC_MEMORY], (unsigned long long) in_memory);
        if (t.alone) atomicAdd(&ctr[LCC_SLOT_ALONE], (unsigned long long) t.alone);
        if (t.list) atomicAdd(&ctr[LCC_SLOT_LIST], (unsigned long long) t.list);
        if (t.tail) atomicAdd(&ctr[LCC_SLOT_TAIL], (unsigned long long) t.tail);
        if (t.hub) atomicAdd(&ctr[LCC_SLOT_HUB], (unsigned long long) t.hub);
        if (t.empty) atomicAdd(&ctr[LCC_SLOT_EMPTY], (unsigned long long) t.empty);
        if (credit_lds) atomicAdd(&ctr[LCC_CREDIT_LDS], credit_lds);
        if (credit_global) atomicAdd(&ctr[LCC_CREDIT_GLOBAL], credit_global);
    }
}

// ------------------------------------------------------------------ finishing kernel
// One thread per caller's id x: tri back through perm, deg, lcc; the three sums.  Only the arrays asked for are written.
__global__ void lcc_finish_kernel(const unsigned long long* __restrict__ tri, const int32_t* __restrict__ perm /* NULL: identity */,
                                  const int32_t* __restrict__ deg, int64_t V, int64_t* __restrict__ tri_out, int32_t* __restrict__ deg_out,
                                  double* __restrict__ lcc_out, unsigned long long* __restrict__ ctr) {
    int64_t x = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    unsigned long long st = 0, sw = 0, nz = 0;
    for (; x < V; x += stride) {
        const unsigned long long tr = tri[perm ? perm[x] : x];
        const int64_t d = deg[x];
        const int64_t pairs = d * (d - 1);   // (d < 2^31: no overflow)
        if (tri_out) tri_out[x] = (int64_t) tr;
        if (deg_out) deg_out[x] = (int32_t) d;
        if (lcc_out) lcc_out[x] = d >= 2 ? (double) (int64_t) (2 * tr) / (double) pairs : 0.0;
        st += tr;
        sw += (unsigned long long) (pairs / 2);
        nz += tr ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        st += __shfl_down(st, off, 64);
        sw += __shfl_down(sw, off, 64);
        nz += __shfl_down(nz, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (st) atomicAdd(&ctr[LCC_SUM_TRI], st);
        if (sw) atomicAdd(&ctr[LCC_WEDGES], sw);
        if (nz) atomicAdd(&ctr[LCC_NONZERO], nz);
    }
}

// ------------------------------------------------------------------ host
// the plan's additions: the work items of the UP' rows (once) and the bit matrix of the H highest ids (again when H changes)
int lcc_plan_groups(tcd_plan* p) {
    if (!p->lcc_ready) {
        GMX_CHECK(tcd_group_offsets<dbuf>(p->up_begin.p, p->V, &p->up_grp_off, 0));
        p->hubs = 0;
        p->lcc_ready = true;
    }
    return GMX_OK;
}

static int lcc_prepare(tcd_plan* p, int64_t H, bool* hub_built) {
    hipStream_t s = 0;
    const int64_t V = p->V;
    GMX_CHECK(lcc_plan_groups(p));
    if (p->hubs != H) {
        const double t0 = gmx_tick::now();
        p->hub_bits.release();
        p->hubs = 0;
        p->hub_ms = 0;
        if (H > 0) {
            const size_t words = (size_t) H * (size_t) (H >> 5);
            if (p->hub_bits.alloc(words)) {
                const std::string why = gmx_last_error();
                gmx_set_error("clustering: the hub matrix of %lld hubs needs %zu bytes: %s", (long long) H, words * sizeof(uint32_t), why.c_str());
                return GMX_ERR_NOMEM;
            }
            GMX_HIP(hipMemsetAsync(p->hub_bits.p, 0, words * sizeof(uint32_t), s));
            hipLaunchKernelGGL(lcc_hub_bits_kernel, dim3((unsigned) ((H + 3) / 4)), dim3(256), 0, s, (const int32_t*) p->up_begin.p,
                               (const int32_t*) p->up_idx.p, V - H, H, p->hub_bits.p);
            GMX_HIP(hipGetLastError());
            GMX_HIP(hipStreamSynchronize(s));
            *hub_built = true;
            p->hubs = H;
            p->hub_ms = (gmx_tick::now() - t0) * 1e3;
        }
    }
    return GMX_OK;
}

template <typename T>
static int lcc_download(T* host, const dbuf<T>& dev, int64_t V) {
    if (host) GMX_HIP(hipMemcpy(host, dev.p, (size_t) V * sizeof(T), hipMemcpyDeviceToHost));
    return GMX_OK;
}

extern "C" int gmx_clustering(gmx_graph_t* g, int64_t* tri_host, int32_t* deg_host, double* lcc_host, int64_t* triangles, int64_t* wedges,
                              gmx_stats_t* stats) {
    GMX_REQUIRE(triangles, "NULL triangles");
    GMX_REQUIRE(g, "NULL graph");
    if (stats) memset(stats, 0, sizeof(*stats));
    const int64_t V = g->V;
    if (V == 0) return GMX_OK;
    *triangles = 0;
    if (wedges) *wedges = 0;
    if (g->E == 0) {
        if (tri_host) memset(tri_host, 0, (size_t) V * sizeof(int64_t));
        if (deg_host) memset(deg_host, 0, (size_t) V * sizeof(int32_t));
        if (lcc_host) memset(lcc_host, 0, (size_t) V * sizeof(double));
        if (stats) stats->iterations = 1;
        return GMX_OK;
    }
    // knobs, read at every call; the results do not depend on them
    const bool ordered = !getenv("GMX_LCC_NO_ORDER");
    const int cap = (int) gmx_env_int("GMX_LCC_CAP", LCC_CAP, LCC_CAP_MIN, LCC_CAP);
    const int alone = (int) gmx_env_int("GMX_LCC_ALONE", LCC_ALONE, 0, INT32_MAX);
    const int ratio = (int) gmx_env_int("GMX_LCC_RATIO", LCC_RATIO, 0, INT32_MAX);
    const int hub_tail = (int) gmx_env_int("GMX_LCC_HUB_TAIL", LCC_HUB_TAIL, 0, INT32_MAX);
    const bool plain = getenv("GMX_LCC_PLAIN") != nullptr;
    // gmx_tc.hip's rule for the number of hubs.  Without the degree order the highest ids are no hubs: no matrix
    int64_t H = gmx_env_int("GMX_LCC_HUBS", V > (1LL << 24) ? LCC_HUB_MAX : LCC_HUB_MAX / 2, 0, LCC_HUB_MAX);
    if (H > V) H = V;
    H &= ~(int64_t) 63;
    if (!ordered) H = 0;
    // graph preprocessing (cached on the graph, shared with gmx_triangle_counting_directed; outside the timed region)
    bool built = false;
    tcd_plan* p = nullptr;
    GMX_CHECK(tcd_plan_get(g, ordered, &p, &built));
    bool hub_built = false;
    GMX_CHECK(lcc_prepare(p, H, &hub_built));
    // the call's scratch: tri in the plan's numbering, the counters, the arrays asked for
    dbuf<unsigned long long> tri, ctr;
    dbuf<int64_t> tri_out;
    dbuf<int32_t> deg_out;
    dbuf<double> lcc_out;
    const size_t scratch = (size_t) V * (8 + (tri_host ? 8 : 0) + (deg_host ? 4 : 0) + (lcc_host ? 8 : 0));
    if (tri.alloc((size_t) V) || ctr.alloc(LCC_NCTR) || (tri_host && tri_out.alloc((size_t) V)) || (deg_host && deg_out.alloc((size_t) V)) ||
        (lcc_host && lcc_out.alloc((size_t) V))) {
        const std::string why = gmx_last_error();
        gmx_set_error("clustering: the per-vertex scratch needs %zu bytes: %s", scratch, why.c_str());
        return GMX_ERR_NOMEM;
    }
    GMX_HIP(hipMemset(ctr.p, 0, LCC_NCTR * sizeof(unsigned long long)));
    gmx_spans tm;
    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_HIP(hipMemsetAsync(tri.p, 0, (size_t) V * sizeof(unsigned long long), 0));
    const uint32_t* bits = p->hubs ? (const uint32_t*) p->hub_bits.p : nullptr;
    const int32_t hub_base = (int32_t) (V - p->hubs);
    const int hub_words = (int) (p->hubs >> 5);
    if (plain)
        hipLaunchKernelGGL(lcc_count_kernel<false>, dim3(256 * 8), dim3(LCC_WAVES * 64), 0, 0, (const int32_t*) p->up_begin.p, (const int32_t*) p->up_idx.p,
                           (const int64_t*) p->up_grp_off.p, V, cap, alone, ratio, bits, hub_base, hub_words, hub_tail, tri.p, ctr.p);
    else
        hipLaunchKernelGGL(lcc_count_kernel<true>, dim3(256 * 8), dim3(LCC_WAVES * 64), 0, 0, (const int32_t*) p->up_begin.p, (const int32_t*) p->up_idx.p,
                           (const int64_t*) p->up_grp_off.p, V, cap, alone, ratio, bits, hub_base, hub_words, hub_tail, tri.p, ctr.p);
    GMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(lcc_finish_kernel, dim3(grid_for(V, LCC_THREADS, 256 * 16)), dim3(LCC_THREADS), 0, 0, (const unsigned long long*) tri.p, (const int32_t*) p->perm.p,
                       (const int32_t*) p->deg.p, V, tri_out.p, deg_out.p, lcc_out.p, ctr.p);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(tm.finish(stats));
    const double t0 = gmx_tick::now();
    unsigned long long h[LCC_NCTR];
    GMX_HIP(hipMemcpy(h, ctr.p, sizeof(h), hipMemcpyDeviceToHost));
    GMX_CHECK(lcc_download(tri_host, tri_out, V));
    GMX_CHECK(lcc_download(deg_host, deg_out, V));
    GMX_CHECK(lcc_download(lcc_host, lcc_out, V));
    const double cms = (gmx_tick::now() - t0) * 1e3;
    *triangles = (int64_t) (h[LCC_SUM_TRI] / 3);
    if (wedges) *wedges = (int64_t) h[LCC_WEDGES];
    if (stats) {
        stats->iterations = 1;
        stats->d2h_ms = cms;   // (the host's clock around the blocking downloads, not a span of tm)
        stats->edges_examined = p->E_up;
        stats->vertices_reached = (int64_t) h[LCC_NONZERO];
    }
    if (getenv("GMX_LCC_LOG"))   // one line per call (tools/lcc_prof.py and the tests parse it)
        fprintf(stderr, "gmx clustering: plan V %lld E %lld up %lld order %s built %d build_ms %.3f hubs %lld hub_ms %.3f; cap %d alone %d ratio %d "
                        "hub_tail %d w %s; items %llu staged + %llu memory; slots %llu alone + %llu list + %llu tail + %llu hub + %llu empty; "
                        "credits %llu lds + %llu global\n",
                (long long) p->V, (long long) p->E, (long long) p->E_up, p->ordered ? "degree" : "identity", built ? 1 : 0, built ? p->build_ms : 0.0,
                (long long) p->hubs, hub_built ? p->hub_ms : 0.0, cap, alone, ratio, hub_tail, plain ? "global" : "lds", h[LCC_STAGED], h[LCC_MEMORY], h[LCC_SLOT_ALONE],
                h[LCC_SLOT_LIST], h[LCC_SLOT_TAIL], h[LCC_SLOT_HUB], h[LCC_SLOT_EMPTY], h[LCC_CREDIT_LDS], h[LCC_CREDIT_GLOBAL]);
    return GMX_OK;
}

void gmx_touch_lcc() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) lcc_count_kernel<true>);
}
