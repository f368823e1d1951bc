// gmx_match.hip -- random_bipartite_matching (maximal bipartite matching by rounds of proposals) for gfx950.
//
// Replaces the body of apps/src/random_bipartite_matching.gm:
//     G.Match = NIL;  G.Suitor = NIL;
//     While (!finished) { finished = True;
//         Foreach (n: G.Nodes)(n.isLeft && n.Match == NIL) Foreach (t: n.Nbrs)(t.Match == NIL) { t.Suitor = n; finished &= False; }
//         Foreach (t: G.Nodes)(!t.isLeft && t.Match == NIL) If (t.Suitor != NIL) { n = t.Suitor; n.Suitor = t; t.Suitor = NIL; }
//         Foreach (n: G.Nodes)(n.isLeft && n.Match == NIL) If (n.Suitor != NIL) { t = n.Suitor; n.Match = t; t.Match = n; count++; } }
//     Return count;
// as ONE thread runs it: the last writer of t.Suitor is the LARGEST unmatched left with an edge to t, the last writer of
// n.Suitor the LARGEST right that chose n (gmx.h).  Both are atomic maxima here:
//   - a round is three launches over lists, none over V or E: propose (the rows of the live lefts, merge-path tiles of
//     gmx_frontier.h), reply (the rights touched in this round) and commit (the live lefts: match, or stay live);
//   - Suitor words carry their round, (round << 32) | id under a 64-bit max: an older round's word loses by itself, nothing
//     is cleared between rounds, and the proposal that replaces an older round's word is the one that puts its right on
//     the touched list;
//   - a left stays live while it is unmatched and proposed in the round before: matches are permanent, so a left whose
//     unmatched neighbours ran out never proposes again.  No row is read twice in a round;
//   - every max is tried only after a load says it would change the word (the max only grows within a round, so skipping
//     is exact even on an old value), and the lanes of a wave that propose to the first proposing lane's right send their
//     largest only: a right that everybody proposes to costs a few atomics per wave that is early, none per wave after;
//   - the first proposal pass reads isLeft[t] instead of Match[t] (nothing is matched yet) and reports a left -> left edge;
//   - once the live rows hold few slots one workgroup runs the rounds to the end (rbm_tail_kernel).
// Integer only: exact.
#include "gmx_frontier.h"

#define RBM_THREADS 256
#define RBM_CHUNK 2048           // list entries a workgroup of the init and commit kernels compacts in LDS
#define RBM_TAIL_THREADS 1024
#define RBM_TAIL 4096            // GMX_RBM_TAIL: the tail launch takes over once the live rows hold at most this many slots
#define RBM_TAIL_LANE 8          // the tail reads a row of at most this many slots with one lane, a longer one with a wave
#define RBM_SHARDS 64

typedef unsigned long long rbm_word;

// Totals that every workgroup adds to are spread over RBM_SHARDS lines (gmx_frontier.h: ~90 atomics per microsecond on one
// line); the list tails are claimed once per workgroup.
struct rbm_counters {
    rbm_word nlive;          // tail of the next live list
    rbm_word mlive;          // its rows' slots
    rbm_word ntouch;         // tail of the touched list
    rbm_word bad;            // 1 + (n << 32 | t) of the largest left -> left edge seen, 0: none
    rbm_word tail_rounds;    // rounds with a proposal the tail launch ran
    rbm_word pad0[11];
    struct {
        rbm_word proposals, matched, lefts, tail_slots;
        rbm_word pad[12];
    } shard[RBM_SHARDS];
};

struct rbm_state {
    const int32_t* begin;
    const int32_t* node_idx;
    const uint8_t* is_left;
    int32_t* match;          // [V] partner, -1: none
    rbm_word* suitor;        // [V] rights: (round << 32) | largest proposing left
    rbm_word* reply;         // [V] lefts:  (round << 32) | largest right that chose it
    int32_t* prop_round;     // [V] lefts:  last round it proposed in
    int32_t* touched;        // [V] rights that got their first proposal of the round
    rbm_counters* ctr;
    int64_t V;
};

__device__ __forceinline__ rbm_word rbm_load(const rbm_word* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rbm_max(rbm_word* p, rbm_word key) {
    if (rbm_load(p) < key) atomicMax(p, key);
}

// ------------------------------------------------------------------ round pieces (shared by the grid kernels and the tail)
// Slot (n, t) of a live left, whole wave here; on: the lane has one.  Returns whether it is a proposal.
template <bool FIRST, class Match>
__device__ __forceinline__ bool rbm_is_proposal(const rbm_state& S, bool on, int32_t n, int32_t t, Match match_of) {
    if (!on) return false;
    if (FIRST) {   // nothing is matched yet; the program's precondition is checked instead
        if (S.is_left[t] == 0) return true;
        rbm_max(&S.ctr->bad, (((rbm_word) (uint32_t) n << 32) | (uint32_t) t) + 1);
        return false;
    }
    return match_of(t) < 0;
}

// prop: the lane's slot (n, t) is a proposal of round r.  list / count: the touched list and its tail.
template <class Count>
__device__ __forceinline__ void rbm_propose(const rbm_state& S, bool prop, int32_t n, int32_t t, int32_t r, int lane, int32_t* list, Count* count) {
    const unsigned long long pm = __ballot(prop);
    if (!pm) return;   // (wave-uniform)
    const int32_t before = __shfl_up(prop ? n : -1, 1, 64);
    if (prop && (lane == 0 || before != n)) S.prop_round[n] = r;   // (one store per run of a row's lanes)
    // the lanes that propose to the first proposing lane's right send their largest left only
    bool act = prop;
    const int32_t t0 = __shfl(t, __builtin_ctzll(pm), 64);
    const bool same = prop && t == t0;
    if (__popcll(__ballot(same)) > 1) {   // (wave-uniform)
        int32_t mx = same ? n : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int32_t y = __shfl_xor(mx, o, 64);
            mx = y > mx ? y : mx;
        }
        if (same && n != mx) act = false;
    }
    bool touch = false;
    if (act) {
        const rbm_word key = ((rbm_word) (uint32_t) r << 32) | (uint32_t) n;
        if (rbm_load(&S.suitor[t]) < key) touch = (int32_t) (atomicMax(&S.suitor[t], key) >> 32) < r;   // replaced an older round's word
    }
    wave_append(touch, t, list, count, lane);
}

// touched right t replies to its suitor
__device__ __forceinline__ void rbm_reply(const rbm_state& S, int32_t t, int32_t r) {
    const int32_t n = (int32_t) (uint32_t) rbm_load(&S.suitor[t]);
    rbm_max(&S.reply[n], ((rbm_word) (uint32_t) r << 32) | (uint32_t) t);
}

// live left n after the replies of round r: 1 matched, 2 stays live, 0 leaves
__device__ __forceinline__ int rbm_commit(const rbm_state& S, int32_t n, int32_t r) {
    const rbm_word w = rbm_load(&S.reply[n]);
    if ((int32_t) (w >> 32) == r) {
        const int32_t t = (int32_t) (uint32_t) w;
        S.match[n] = t;
        S.match[t] = n;
        return 1;
    }
    return S.prop_round[n] == r ? 2 : 0;
}

// ------------------------------------------------------------------ grid kernels
// Round 1's live list: the lefts with a non-empty row, high ids first (a workgroup takes RBM_CHUNK vertices from the top,
// and workgroups start in launch order): a right's proposals then arrive largest first, as far as the schedule keeps it.
__global__ void __launch_bounds__(RBM_THREADS) rbm_init_kernel(rbm_state S, int32_t* __restrict__ live) {
    __shared__ int32_t s_win[RBM_CHUNK];
    __shared__ unsigned int s_nwin;
    __shared__ rbm_word s_deg, s_lefts, s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_nwin = 0;
        s_deg = 0;
        s_lefts = 0;
    }
    __syncthreads();
    rbm_word deg = 0, lefts = 0;
    for (int k = 0; k < RBM_CHUNK / RBM_THREADS; k++) {
        const int64_t i = (int64_t) blockIdx.x * RBM_CHUNK + k * RBM_THREADS + tid;
        const int64_t v = S.V - 1 - i;
        bool keep = false;
        if (v >= 0 && S.is_left[v]) {
            const int32_t d = S.begin[v + 1] - S.begin[v];
            lefts++;
            keep = d > 0;
            deg += (rbm_word) d;
        }
        wave_append(keep, (int32_t) v, s_win, &s_nwin, lane);
    }
    deg = wave_sum(deg);
    lefts = wave_sum(lefts);
    if (lane == 0) {
        if (deg) atomicAdd(&s_deg, deg);
        if (lefts) atomicAdd(&s_lefts, lefts);
    }
    __syncthreads();
    frontier_flush(s_win, s_nwin, &S.ctr->nlive, live, &s_base, [&] {
        if (s_deg) atomicAdd(&S.ctr->mlive, s_deg);
        if (s_lefts) atomicAdd(&S.ctr->shard[blockIdx.x & (RBM_SHARDS - 1)].lefts, s_lefts);
    });
}

// the rows of the live lefts live[0 .. n), m slots in all, cut into merge-path tiles
template <bool FIRST>
__global__ void __launch_bounds__(BFS_THREADS) rbm_propose_kernel(rbm_state S, const int32_t* __restrict__ live, int64_t n,
                                                                  const int64_t* __restrict__ off, int64_t m, int32_t r) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_left[BFS_ITEMS + 2];
    __shared__ int64_t s_split[2][2];
    __shared__ int32_t s_win[BFS_ITEMS];
    __shared__ unsigned int s_nwin;
    __shared__ rbm_word s_prop, s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_nwin = 0;
        s_prop = 0;
    }
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.begin, live, n, off, m, s_off, s_row, [&](int i, int32_t v, bool) { s_left[i] = v; });
    rbm_word props = 0;
    for (int64_t base = t.e0; base < t.e1; base += BFS_THREADS) {   // (workgroup-uniform trip count)
        const int64_t x = base + tid;
        const bool on = x < t.e1;
        int32_t nn = 0, tt = 0;
        if (on) {
            const int lo = frontier_slot(s_off, nv, x);
            nn = s_left[lo];
            tt = S.node_idx[(int64_t) s_row[lo] + (x - s_off[lo])];
        }
        const bool prop = rbm_is_proposal<FIRST>(S, on, nn, tt, [&](int32_t v) { return S.match[v]; });
        props += prop ? 1 : 0;
        rbm_propose(S, prop, nn, tt, r, lane, s_win, &s_nwin);
    }
    props = wave_sum(props);
    if (lane == 0 && props) atomicAdd(&s_prop, props);
    __syncthreads();
    frontier_flush(s_win, s_nwin, &S.ctr->ntouch, S.touched, &s_base, [&] {
        if (s_prop) atomicAdd(&S.ctr->shard[blockIdx.x & (RBM_SHARDS - 1)].proposals, s_prop);
    });
}

// touched[0 .. ctr->ntouch); launched for an upper bound of the count
__global__ void __launch_bounds__(RBM_THREADS) rbm_reply_kernel(rbm_state S, int32_t r) {
    const int64_t n = (int64_t) S.ctr->ntouch;
    int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (; i < n; i += stride) rbm_reply(S, S.touched[i], r);
}

// live[0 .. n): a workgroup per RBM_CHUNK entries, in order, so that the next list keeps the high-ids-first order roughly
__global__ void __launch_bounds__(RBM_THREADS) rbm_commit_kernel(rbm_state S, const int32_t* __restrict__ live, int64_t n, int32_t r,
                                                                 int32_t* __restrict__ next) {
    __shared__ int32_t s_win[RBM_CHUNK];
    __shared__ unsigned int s_nwin;
    __shared__ rbm_word s_deg, s_match, s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        s_nwin = 0;
        s_deg = 0;
        s_match = 0;
    }
    __syncthreads();
    rbm_word deg = 0, matched = 0;
    for (int k = 0; k < RBM_CHUNK / RBM_THREADS; k++) {
        const int64_t i = (int64_t) blockIdx.x * RBM_CHUNK + k * RBM_THREADS + tid;
        int32_t v = 0;
        int what = 0;
        if (i < n) {
            v = live[i];
            what = rbm_commit(S, v, r);
        }
        if (what == 1) matched++;
        if (what == 2) deg += (rbm_word) (S.begin[v + 1] - S.begin[v]);
        wave_append(what == 2, v, s_win, &s_nwin, lane);
    }
    deg = wave_sum(deg);
    matched = wave_sum(matched);
    if (lane == 0) {
        if (deg) atomicAdd(&s_deg, deg);
        if (matched) atomicAdd(&s_match, matched);
    }
    __syncthreads();
    frontier_flush(s_win, s_nwin, &S.ctr->nlive, next, &s_base, [&] {
        if (s_deg) atomicAdd(&S.ctr->mlive, s_deg);
        if (s_match) atomicAdd(&S.ctr->shard[blockIdx.x & (RBM_SHARDS - 1)].matched, s_match);
    });
}

// ------------------------------------------------------------------ the tail: one workgroup runs the rounds to the end
// la[0 .. n): the live lefts of round r (first: no round has run).  Words that atomics
// write (suitor, reply) are read back with device-scope loads behind the workgroup's barrier; Match, the proposal stamps
// and the lists are plain stores of this workgroup, visible to its waves behind the same barrier, as in gmx_vcover.hip.
// The rows are walked by tail_rows (gmx_frontier.h).
// At most V rounds (every round but the last matches a pair), each a bounded loop: no waiting on anybody.
__global__ void __launch_bounds__(RBM_TAIL_THREADS) rbm_tail_kernel(rbm_state S, int32_t* la, int32_t* lb, int64_t n, int first, int32_t r) {
    __shared__ unsigned int s_ntouch, s_nnext;
    __shared__ rbm_word s_prop;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = blockDim.x >> 6;
    if (tid == 0) {
        s_ntouch = 0;
        s_nnext = 0;
        s_prop = 0;
    }
    __syncthreads();
    rbm_word slots = 0, matched = 0, prev = 0;
    int32_t rounds = 0;
    while (n > 0) {
        rbm_word props = 0;
        const auto match_of = [&](int32_t u) { return S.match[u]; };
        const auto slot = [&](bool on, int32_t v, int32_t idx) {
            const int32_t tt = on ? S.node_idx[idx] : 0;
            const bool prop = first ? rbm_is_proposal<true>(S, on, v, tt, match_of) : rbm_is_proposal<false>(S, on, v, tt, match_of);
            props += prop ? 1 : 0;
            rbm_propose(S, prop, v, tt, r, lane, S.touched, &s_ntouch);
        };
        const auto load = [&](bool, int32_t v, int32_t deg) {
            slots += (rbm_word) deg;
            return v;
        };
        tail_rows<RBM_TAIL_LANE>(la, n, S.begin, lane, wave, nwaves, load, slot);
        props = wave_sum(props);
        if (lane == 0 && props) atomicAdd(&s_prop, props);
        __syncthreads();
        const rbm_word total = s_prop;
        const int64_t ntouch = (int64_t) s_ntouch;
        if (total == prev) break;   // the round made no proposal: it does not count (workgroup-uniform)
        prev = total;
        rounds++;
        first = 0;
        for (int64_t i = tid; i < ntouch; i += blockDim.x) rbm_reply(S, S.touched[i], r);
        __syncthreads();
        for (int64_t base = tid - lane; base < n; base += blockDim.x) {
            const int64_t i = base + lane;
            int32_t v = 0;
            int what = 0;
            if (i < n) {
                v = la[i];
                what = rbm_commit(S, v, r);
            }
            if (what == 1) matched++;
            wave_append(what == 2, v, lb, &s_nnext, lane);
        }
        __syncthreads();
        n = (int64_t) s_nnext;
        __syncthreads();
        if (tid == 0) {
            s_ntouch = 0;
            s_nnext = 0;
        }
        int32_t* x = la; la = lb; lb = x;
        r++;
        __syncthreads();
    }
    slots = wave_sum(slots);
    matched = wave_sum(matched);
    if (lane == 0) {
        const int sh = (int) wave & (RBM_SHARDS - 1);
        if (slots) atomicAdd(&S.ctr->shard[sh].tail_slots, slots);
        if (matched) atomicAdd(&S.ctr->shard[sh].matched, matched);
    }
    if (tid == 0) {
        if (prev) atomicAdd(&S.ctr->shard[0].proposals, prev);
        S.ctr->tail_rounds = (rbm_word) rounds;
    }
}

// ------------------------------------------------------------------ host
struct rbm_totals {
    rbm_word proposals = 0, matched = 0, lefts = 0, tail_slots = 0;
};
static rbm_totals rbm_sum(const rbm_counters& h) {
    rbm_totals t;
    for (int i = 0; i < RBM_SHARDS; i++) {
        t.proposals += h.shard[i].proposals;
        t.matched += h.shard[i].matched;
        t.lefts += h.shard[i].lefts;
        t.tail_slots += h.shard[i].tail_slots;
    }
    return t;
}

extern "C" int gmx_random_bipartite_matching(gmx_graph_t* g, const uint8_t* is_left_host, gmx_node_t* match_host, int32_t* count, gmx_stats_t* stats) {
    GMX_REQUIRE(g && count, "NULL argument");
    GMX_REQUIRE((is_left_host && match_host) || g->V == 0, "random_bipartite_matching: is_left or match is NULL");
    if (stats) memset(stats, 0, sizeof(*stats));
    *count = 0;
    const int64_t V = g->V, E = g->E;
    if (V == 0) return GMX_OK;
    const int64_t tail_from = gmx_env_int("GMX_RBM_TAIL", RBM_TAIL, 0, INT32_MAX);   // read at every call; the result does not depend on it
    const int64_t log = gmx_env_int("GMX_RBM_LOG", 0, 0, INT32_MAX);                 // 1: one line per call; 2: a line per grid round before it

    dbuf<uint8_t> is_left;
    dbuf<int32_t> match, prop_round, touched, l0, l1;
    dbuf<rbm_word> suitor, reply;
    dbuf<rbm_counters> ctr;
    frontier_scan fs;
    gmx_pinned<rbm_counters> h_ctr;
    GMX_CHECK(is_left.alloc((size_t) V));
    GMX_CHECK(match.alloc((size_t) V));
    GMX_CHECK(prop_round.alloc((size_t) V));
    GMX_CHECK(touched.alloc((size_t) V));
    GMX_CHECK(l0.alloc((size_t) V));
    GMX_CHECK(l1.alloc((size_t) V));
    GMX_CHECK(suitor.alloc((size_t) V));
    GMX_CHECK(reply.alloc((size_t) V));
    GMX_CHECK(ctr.alloc(1));
    GMX_CHECK(gmx_frontier_scan_alloc(&fs, (size_t) V, 0));
    GMX_CHECK(h_ctr.alloc(1));
    gmx_spans tm;

    rbm_state S;
    S.begin = g->begin.p;
    S.node_idx = g->node_idx.p;
    S.is_left = is_left.p;
    S.match = match.p;
    S.suitor = suitor.p;
    S.reply = reply.p;
    S.prop_round = prop_round.p;
    S.touched = touched.p;
    S.ctr = ctr.p;
    S.V = V;
    rbm_counters* h = h_ctr.p;

    GMX_CHECK(tm.begin(tm.H2D));
    GMX_HIP(hipMemcpyAsync(is_left.p, is_left_host, (size_t) V, hipMemcpyHostToDevice, 0));
    GMX_CHECK(tm.end(tm.H2D));
    GMX_CHECK(tm.begin(tm.KERNEL));
    const double t_start = gmx_tick::now();
    GMX_HIP(hipMemsetAsync(ctr.p, 0, sizeof(rbm_counters), 0));
    GMX_HIP(hipMemsetAsync(match.p, 0xff, sizeof(int32_t) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(suitor.p, 0, sizeof(rbm_word) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(reply.p, 0, sizeof(rbm_word) * (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(prop_round.p, 0, sizeof(int32_t) * (size_t) V, 0));
    int32_t* la = l0.p;   // the live lefts of the next round
    int32_t* lb = l1.p;
    hipLaunchKernelGGL(rbm_init_kernel, dim3((unsigned) ((V + RBM_CHUNK - 1) / RBM_CHUNK)), dim3(RBM_THREADS), 0, 0, S, la);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_read_back(h_ctr, ctr.p));
    int64_t n = (int64_t) h->nlive, m = (int64_t) h->mlive;
    const int64_t lefts = (int64_t) rbm_sum(*h).lefts;
    int32_t round = 0, tail_rounds = 0;
    int64_t grid_slots = 0;
    rbm_word proposals = 0;
    double tail_ms = 0;
    while (n > 0) {
        if (tail_from > 0 && m <= tail_from) {   // the rest in one workgroup
            const double t_tail0 = gmx_tick::now();
            hipLaunchKernelGGL(rbm_tail_kernel, dim3(1), dim3(RBM_TAIL_THREADS), 0, 0, S, la, lb, n, round == 0 ? 1 : 0, round + 1);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctr, ctr.p));
            tail_rounds = (int32_t) h->tail_rounds;
            tail_ms = (gmx_tick::now() - t_tail0) * 1e3;
            break;
        }
        const double t_round0 = gmx_tick::now();
        GMX_HIP(hipMemsetAsync(&ctr.p->nlive, 0, 3 * sizeof(rbm_word), 0));   // nlive, mlive, ntouch
        GMX_CHECK(gmx_frontier_offsets(g->begin.p, la, n, &fs, nullptr, false));
        const int64_t nb = frontier_tiles(n, m);
        if (round == 0)
            hipLaunchKernelGGL(rbm_propose_kernel<true>, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, S, (const int32_t*) la, n, (const int64_t*) fs.off.p, m, round + 1);
        else
            hipLaunchKernelGGL(rbm_propose_kernel<false>, dim3((unsigned) nb), dim3(BFS_THREADS), 0, 0, S, (const int32_t*) la, n, (const int64_t*) fs.off.p, m, round + 1);
        hipLaunchKernelGGL(rbm_reply_kernel, dim3(grid_for(m < V ? m : V, RBM_THREADS)), dim3(RBM_THREADS), 0, 0, S, round + 1);   // a slot touches at most one right
        hipLaunchKernelGGL(rbm_commit_kernel, dim3((unsigned) ((n + RBM_CHUNK - 1) / RBM_CHUNK)), dim3(RBM_THREADS), 0, 0, S, (const int32_t*) la, n, round + 1, lb);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctr, ctr.p));
        grid_slots += m;
        const rbm_word p = rbm_sum(*h).proposals;
        if (log >= 2)
            fprintf(stderr, "gmx random_bipartite_matching round %d: live %lld slots %lld proposals %llu touched %llu ms %.3f\n", round + 1, (long long) n,
                    (long long) m, p - proposals, h->ntouch, (gmx_tick::now() - t_round0) * 1e3);
        if (p == proposals) break;   // the round made no proposal: it does not count, and nobody stayed live
        proposals = p;
        round++;
        n = (int64_t) h->nlive;
        m = (int64_t) h->mlive;
        int32_t* x = la; la = lb; lb = x;
    }
    GMX_CHECK(tm.end(tm.KERNEL));
    const double t_end = gmx_tick::now();
    const rbm_totals tot = rbm_sum(*h);
    if (h->bad) {
        const rbm_word w = h->bad - 1;
        gmx_set_error("random_bipartite_matching: edge %u -> %u joins two left vertices; every edge must lead from a left to a right vertex",
                      (unsigned) (w >> 32), (unsigned) (w & 0xffffffffu));
        return GMX_ERR_ARG;
    }
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpyAsync(match_host, match.p, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost, 0));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));   // (the download has landed)
    *count = (int32_t) tot.matched;
    if (stats) {
        stats->iterations = round + tail_rounds;
        stats->edges_examined = grid_slots + (int64_t) tot.tail_slots;
        stats->edges_reached = (int64_t) tot.proposals;
        stats->vertices_reached = (int64_t) tot.matched;
    }
    if (log >= 1)   // one line per call (tools/match_prof.py and the tests parse it)
        fprintf(stderr, "gmx random_bipartite_matching: V %lld E %lld lefts %lld; tail %lld; rounds %d grid + %d tail; matched %llu; proposals %llu "
                        "slots %lld; ms %.3f grid + %.3f tail\n",
                (long long) V, (long long) E, (long long) lefts, (long long) tail_from, round, tail_rounds, tot.matched, tot.proposals,
                (long long) (grid_slots + (int64_t) tot.tail_slots), (t_end - t_start) * 1e3 - tail_ms, tail_ms);
    return GMX_OK;
}

void gmx_touch_match() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) rbm_tail_kernel);
}
