// gmx_msf.hip -- minimum spanning forests on gfx950: Boruvka's algorithm in synchronous rounds on the directed CSR read as
// an undirected multigraph.  The reference has no such program; the graph read, the order (weight, uploaded slot) that
// makes the forest unique, the schedule and the statistics are the contract at gmx_msf in gmx.h.
//
// parent[V] is a forest of the trees found so far (a root has parent[x] == x; unlike gmx_wcc's, a parent may be the larger
// id) and best[V] one 64-bit word per vertex, used at the roots: the smallest key = (weight biased to unsigned) << 32 |
// uploaded slot among the cross slots that touch the tree, under atomicMin.
//   find      the rows of the list go through the merge-path tile (gmx_frontier.h).  At a round's start every listed u and
//             every head w has its root in parent[] (the compress of the round before), so a slot is cross when parent[u] !=
//             parent[w].  A tile's offers for the tail's side are reduced per staged row in LDS and leave as one atomic per
//             row; those for the head's side are reduced over the lanes of a wave that share the first lane's tree (in
//             RMAT's later rounds: the giant tree) and leave as one atomic for them.  Every atomic is tried only after a
//             load says it would lower the word: best only falls, so a stale load costs an atomic and never loses an offer.
//             A row with a cross slot sets flag[u] for the next list.
//   hook      every root with a best selects its slot: the slot's device position through the inverse of e_idx2idx (built
//             per call, only where the rows were sorted on upload), its tail by csr_row_of, its head from node_idx.  The
//             root takes the other end's tree as its parent, except that of a mutual pair -- both chose the same slot -- the
//             smaller id stays root and marks the slot alone.  With a strict order these are the only cycles.
//   next      compress (every parent[v] = the root of v), best[v] reset, and the flagged vertices compacted into the next
//             list together with the slots of their rows: one pass over the vertices, one read-back per round.
//   tail      once the list's rows hold at most GMX_MSF_TAIL slots one workgroup runs all remaining rounds behind barriers:
//             roots by climbing (nothing compresses the other vertices any more), the trees that received an offer in a
//             list of their own, so that a round costs what its list costs and nothing per vertex.  The list's slots never
//             grow -- a row is listed only if it was listed before -- so the tail never hands back.
//   finish    with comp: compress, the smallest vertex of every tree, wcc's scan of those flags, the sizes by root.
// Host round trips: one per grid round (the next list's length, its slots, the slots selected so far), one for the tail.
#include "gmx_frontier.h"

#include <rocprim/rocprim.hpp>

#define MSF_THREADS BFS_THREADS
#define MSF_TAIL_THREADS 1024
#define MSF_TAIL 4096       // GMX_MSF_TAIL: the tail launch takes over once the list's rows hold at most this many slots
#define MSF_TAIL_LANE 8     // the tail reads a row of at most this many slots with one lane, a longer one with a wave
#define MSF_BIG_GROUP 8     // msf_trees_kernel: a wave carries a group of equal roots along from this many lanes on
#define MSF_NONE 0xFFFFFFFFFFFFFFFFull   // no offer: above every key (a slot is below 2^31)

typedef unsigned long long msf_word;

struct msf_ctl {
    msf_word listed;       // tail of the list that msf_next_kernel writes
    msf_word next_slots;   // slots of its rows
    // what the tail hands back
    msf_word t_rounds, t_merging, t_slots;
    unsigned int maxatom, pad0;
    msf_word pad1[10];
    struct {
        msf_word count;    // slots selected so far
        long long weight;  // their sum
        msf_word pad[14];
    } shard[BFS_SHARDS];
    int32_t comps;
    unsigned int largest;
};

struct msf_state {
    const int32_t* begin;
    const int32_t* idx;
    const int32_t* weight;   // by device slot, or NULL: all 0
    const int32_t* order;    // e_idx2idx: uploaded slot of a device slot, or NULL: the same
    const int32_t* inv;      // its inverse, or NULL
    int32_t* parent;
    msf_word* best;
    uint8_t* flag;           // [V] the vertex had a cross out-slot in this round
    uint8_t* in_forest;      // [E] by uploaded slot
    unsigned int* atoms;     // [V] atomics tried on best[v] in this round (GMX_MSF_PHASES), or NULL
    msf_ctl* ctl;
    int64_t V;
};

__device__ __forceinline__ int32_t msf_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ msf_word msf_load(const msf_word* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint8_t msf_load(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T>
__device__ __forceinline__ void msf_store(T* p, T x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int msf_shard() { return (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (BFS_SHARDS - 1); }

__device__ __forceinline__ msf_word msf_key(int32_t weight, uint32_t slot) { return ((msf_word) ((uint32_t) weight ^ 0x80000000u) << 32) | slot; }
__device__ __forceinline__ int32_t msf_key_weight(msf_word key) { return (int32_t) ((uint32_t) (key >> 32) ^ 0x80000000u); }

// The root of v.  While this runs no root is hooked, so the climb ends at v's true root whatever it reads on the way.  Every
// vertex it passes is pointed at its grandparent by a CAS that expects the parent it read: a word only ever moves towards
// its root and a late CAS fails instead of undoing a better one (gmx_wcc's compress gets the same from atomicMin, which
// needs parent[x] <= x; here a tree hooks under the tree it chose, whichever id that has).  The loads are agent-scope
// atomic loads (THE MEMORY RULE at wcc_hook): the words come from atomics, and the chain of a path graph is V - 1 deep.
__device__ __forceinline__ int32_t msf_root(int32_t* __restrict__ parent, int32_t v) {
    int32_t x = v, p = msf_load(&parent[x]);
    while (p != x) {
        const int32_t gp = msf_load(&parent[p]);
        if (gp == p) break;
        atomicCAS(&parent[x], p, gp);
        x = p;
        p = gp;
    }
    return p;
}

// key is offered to best[t]; the caller's load said it would lower the word.  Returns what the word held.
__device__ __forceinline__ msf_word msf_offer(const msf_state& S, int32_t t, msf_word key) {
    if (S.atoms) atomicAdd(&S.atoms[t], 1u);
    return atomicMin(&S.best[t], key);
}

// inv[order[e]] = e
__global__ void __launch_bounds__(MSF_THREADS) msf_inverse_kernel(const int32_t* __restrict__ order, int64_t E, int32_t* __restrict__ inv) {
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t) gridDim.x * blockDim.x) inv[order[e]] = (int32_t) e;
}

// ---- find: one merge-path tile of the rows of list[0, n)
__global__ void __launch_bounds__(MSF_THREADS) msf_find_kernel(msf_state S, const int32_t* __restrict__ list, int64_t n, const int64_t* __restrict__ off, int64_t m) {
    __shared__ int64_t s_off[BFS_ITEMS + 2];
    __shared__ int32_t s_row[BFS_ITEMS + 2];
    __shared__ int32_t s_tu[BFS_ITEMS + 2];
    __shared__ msf_word s_best[BFS_ITEMS + 2];
    __shared__ int64_t s_split[2][2];
    const int tid = threadIdx.x;
    const frontier_tile t = frontier_tile_search(off, n, m, s_split);
    const int nv = frontier_stage(t, S.begin, list, n, off, m, s_off, s_row, [&](int i, int32_t v, bool in_range) {
        s_tu[i] = in_range ? S.parent[v] : 0;
        s_best[i] = MSF_NONE;
    });
    if (t.e1 <= t.e0) return;   // (workgroup-uniform)
    constexpr int K = BFS_ITEMS / MSF_THREADS;
    int32_t w[K], tw[K], wt[K], lo[K];
    uint32_t up[K];
    bool valid[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int64_t x = t.e0 + tid + (int64_t) k * MSF_THREADS;
        valid[k] = x < t.e1;
        const int64_t xc = valid[k] ? x : t.e0;   // (loads stay unconditional: a slot that exists)
        lo[k] = frontier_slot(s_off, nv, xc);
        const int64_t e = (int64_t) s_row[lo[k]] + (xc - s_off[lo[k]]);
        w[k] = S.idx[e];
        wt[k] = S.weight ? S.weight[e] : 0;
        up[k] = S.order ? (uint32_t) S.order[e] : (uint32_t) e;
    }
#pragma unroll
    for (int k = 0; k < K; k++) tw[k] = S.parent[w[k]];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const bool cross = valid[k] && tw[k] != s_tu[lo[k]];
        const msf_word key = cross ? msf_key(wt[k], up[k]) : MSF_NONE;
        if (cross) atomicMin(&s_best[lo[k]], key);
        // the head's side: the lanes whose tree is the first offering lane's leave as one atomic
        const bool on = cross && key < S.best[tw[k]];
        const unsigned long long mk = __ballot(on);
        if (mk) {   // (wave-uniform)
            const int32_t lt = __shfl(tw[k], __ffsll((long long) mk) - 1, 64);
            const bool same = on && tw[k] == lt;
            const msf_word mn = wave_min(same ? key : MSF_NONE);
            if ((tid & 63) == 0) msf_offer(S, lt, mn);
            if (on && !same) msf_offer(S, tw[k], key);
        }
    }
    __syncthreads();
    // the tail's side: one atomic per staged row that had a cross slot, and the row's vertex goes to the next list (read
    // again: a fifth array would put the tile's LDS at 57 KB, two workgroups a CU)
    for (int i = tid; i < nv; i += MSF_THREADS) {
        const msf_word key = s_best[i];
        if (key != MSF_NONE) {   // (a staged row that has a slot is one of the list's)
            S.flag[list[t.v0 + i]] = 1;
            if (key < S.best[s_tu[i]]) msf_offer(S, s_tu[i], key);
        }
    }
}

// what selecting its best slot means for the root t: *other = the tree at the slot's other end (tree_of(x): the root of x
// as the round began), *stay = t is the smaller root of a mutual pair and stays a root; returns whether t marks the slot
template <class TreeOf, class BestOf>
__device__ __forceinline__ bool msf_choose(const msf_state& S, int32_t t, msf_word key, TreeOf tree_of, BestOf best_of, int32_t* other, bool* stay) {
    const uint32_t s = (uint32_t) key;
    const uint32_t e = S.inv ? (uint32_t) S.inv[s] : s;
    const int32_t u = csr_row_of(S.begin, S.V, e), w = S.idx[e];
    const int32_t tu = tree_of(u);
    const int32_t o = tu == t ? tree_of(w) : tu;
    const bool mutual = best_of(o) == key;
    *other = o;
    *stay = mutual && t < o;
    return !mutual || *stay;
}

// ---- hook on the grid: every root with a best.  parent[] is written at hooking roots only, and those are exactly the
// vertices x with best[x] != MSF_NONE, which this kernel does not write: so the tree of x as the round began is x itself
// where best[x] is set and the (compressed, unwritten) parent[x] elsewhere, whatever the other threads have hooked already.
__global__ void __launch_bounds__(MSF_THREADS) msf_hook_kernel(msf_state S) {
    msf_word count = 0;
    long long weight = 0;
    const auto tree_of = [&](int32_t x) { return S.best[x] != MSF_NONE ? x : S.parent[x]; };
    const auto best_of = [&](int32_t x) { return S.best[x]; };
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < S.V; v += (int64_t) gridDim.x * blockDim.x) {
        const msf_word key = S.best[v];
        if (key == MSF_NONE) continue;
        int32_t other;
        bool stay;
        if (msf_choose(S, (int32_t) v, key, tree_of, best_of, &other, &stay)) {
            S.in_forest[(uint32_t) key] = 1;
            count++;
            weight += msf_key_weight(key);
        }
        if (!stay) S.parent[v] = other;
    }
    count = wave_sum(count);
    weight = wave_sum(weight);
    if ((threadIdx.x & 63) == 0 && count) {
        atomicAdd(&S.ctl->shard[msf_shard()].count, count);
        atomicAdd((msf_word*) &S.ctl->shard[msf_shard()].weight, (msf_word) weight);
    }
}

// ---- next: first: parent[v] = v and the vertices that have an out-slot are listed; else parent[v] = the root of v and
// the flagged vertices are.  best[v] is reset, the list's slots are summed.  A workgroup collects BFS_ITEMS vertices in LDS
// and claims the tail once.
__global__ void __launch_bounds__(MSF_THREADS) msf_next_kernel(msf_state S, int first, int32_t* __restrict__ list) {
    __shared__ int32_t s_list[BFS_ITEMS];
    __shared__ unsigned int s_n;
    __shared__ msf_word s_m, s_base;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t t0 = (int64_t) blockIdx.x * BFS_ITEMS; t0 < S.V; t0 += (int64_t) gridDim.x * BFS_ITEMS) {
        if (tid == 0) {
            s_n = 0;
            s_m = 0;
        }
        __syncthreads();
        for (int k = 0; k < BFS_ITEMS / MSF_THREADS; k++) {
            const int64_t v = t0 + k * MSF_THREADS + tid;
            bool on = false;
            msf_word deg = 0;
            if (v < S.V) {
                deg = (msf_word) (S.begin[v + 1] - S.begin[v]);
                if (first) {
                    S.parent[v] = (int32_t) v;
                    on = deg > 0;
                } else {
                    const int32_t r = msf_root(S.parent, (int32_t) v);
                    msf_store(&S.parent[v], r);   // (after it no CAS on this word succeeds: each expects a value that is not the root)
                    on = S.flag[v] != 0;
                    if (on) S.flag[v] = 0;
                }
                S.best[v] = MSF_NONE;
            }
            const msf_word d = wave_sum(on ? deg : 0);
            if (lane == 0 && d) atomicAdd(&s_m, d);
            wave_append(on, (int32_t) v, s_list, &s_n, lane);
        }
        __syncthreads();
        frontier_flush(s_list, s_n, &S.ctl->listed, list, &s_base, [&] { if (s_m) atomicAdd(&S.ctl->next_slots, s_m); });
        __syncthreads();
    }
}

// ---- the tail: one workgroup runs every remaining round on la[0, n).  parent[], best[] and flag[] are read with agent-scope
// atomic loads and written with atomics or atomic stores; the lists, roots[] and to[] are plain stores of this workgroup,
// read behind its barrier.  roots[]: the trees that received their first offer in this round (the atomicMin that returns
// MSF_NONE appends), to[i]: what roots[i] hooks under, -1: it stays a root.
__global__ void __launch_bounds__(MSF_TAIL_THREADS) msf_tail_kernel(msf_state S, int32_t* la, int32_t* lb, int64_t n, int32_t* __restrict__ roots,
                                                                     int32_t* __restrict__ to) {
    __shared__ unsigned int s_nnext, s_nroots;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t wave = tid >> 6, nwaves = blockDim.x >> 6;
    if (tid == 0) s_nnext = s_nroots = 0;
    __syncthreads();
    msf_word slots = 0, count = 0, rounds = 0, merging = 0;
    long long weight = 0;
    const auto offer = [&](bool on, int32_t t, msf_word key) {   // (the whole wave)
        bool firstoffer = false;
        if (on && key < msf_load(&S.best[t])) firstoffer = msf_offer(S, t, key) == MSF_NONE;
        wave_append(firstoffer, t, roots, &s_nroots, lane);
    };
    const auto tree_of = [&](int32_t x) { return msf_root(S.parent, x); };
    const auto best_of = [&](int32_t x) { return msf_load(&S.best[x]); };
    while (n > 0) {
        // find: the trees of both ends by climbing; nothing hooks before the barrier
        const auto load = [&](bool have, int32_t v, int32_t deg) {
            slots += (msf_word) deg;
            return ((msf_word) (uint32_t) v << 32) | (msf_word) (uint32_t) (have ? msf_root(S.parent, v) : 0);
        };
        const auto slot = [&](bool on, msf_word p, int32_t e) {
            const int32_t u = (int32_t) (p >> 32), tu = (int32_t) (uint32_t) p;
            const int32_t w = on ? S.idx[e] : u;
            const int32_t tw = w != u ? msf_root(S.parent, w) : tu;
            const bool cross = tw != tu;
            msf_word key = MSF_NONE;
            if (cross) {
                key = msf_key(S.weight ? S.weight[e] : 0, S.order ? (uint32_t) S.order[e] : (uint32_t) e);
                msf_store(&S.flag[u], (uint8_t) 1);
            }
            offer(cross, tu, key);
            offer(cross, tw, key);
        };
        tail_rows<MSF_TAIL_LANE>(la, n, S.begin, lane, wave, nwaves, load, slot);
        __syncthreads();
        rounds++;
        const int64_t nroots = (int64_t) s_nroots;
        if (nroots == 0) break;   // no cross slot: the last round (workgroup-uniform)
        merging++;
        // hook, first half: what every offered tree does, from the forest as the round began
        for (int64_t i = tid; i < nroots; i += MSF_TAIL_THREADS) {
            const int32_t t = roots[i];
            const msf_word key = msf_load(&S.best[t]);
            int32_t other;
            bool stay;
            if (msf_choose(S, t, key, tree_of, best_of, &other, &stay)) {
                S.in_forest[(uint32_t) key] = 1;
                count++;
                weight += msf_key_weight(key);
            }
            to[i] = stay ? -1 : other;
        }
        // ... and the next list: the rows that had a cross slot
        for (int64_t base = tid - lane; base < n; base += MSF_TAIL_THREADS) {
            const int64_t i = base + lane;
            const int32_t v = i < n ? la[i] : 0;
            const bool on = i < n && msf_load(&S.flag[v]) != 0;
            if (on) msf_store(&S.flag[v], (uint8_t) 0);
            wave_append(on, v, lb, &s_nnext, lane);
        }
        __syncthreads();
        // second half: the hooks, and best reset
        for (int64_t i = tid; i < nroots; i += MSF_TAIL_THREADS) {
            const int32_t t = roots[i];
            if (to[i] >= 0) msf_store(&S.parent[t], to[i]);
            msf_store(&S.best[t], (msf_word) MSF_NONE);
        }
        n = (int64_t) s_nnext;
        int32_t* x = la; la = lb; lb = x;
        __syncthreads();
        if (tid == 0) s_nnext = s_nroots = 0;
        __syncthreads();
    }
    slots = wave_sum(slots);
    count = wave_sum(count);
    weight = wave_sum(weight);
    if (lane == 0) {
        if (slots) atomicAdd(&S.ctl->t_slots, slots);
        if (count) {
            atomicAdd(&S.ctl->shard[msf_shard()].count, count);
            atomicAdd((msf_word*) &S.ctl->shard[msf_shard()].weight, (msf_word) weight);
        }
    }
    if (tid == 0) {
        S.ctl->t_rounds = rounds;
        S.ctl->t_merging = merging;
    }
}

// the largest number of atomics one word received in the round, and the counts reset (GMX_MSF_PHASES)
__global__ void __launch_bounds__(MSF_THREADS) msf_maxatom_kernel(unsigned int* __restrict__ atoms, int64_t V, msf_ctl* __restrict__ ctl) {
    unsigned int mx = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        mx = max(mx, atoms[v]);
        atoms[v] = 0;
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctl->maxatom, mx);
}

// ---- finish (with comp): the components are the trees, numbered as gmx_wcc numbers them
__global__ void __launch_bounds__(MSF_THREADS) msf_compress_kernel(int32_t* __restrict__ parent, int64_t V, int32_t* __restrict__ minv, int32_t* __restrict__ size) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        msf_store(&parent[v], msf_root(parent, (int32_t) v));
        minv[v] = INT32_MAX;
        size[v] = 0;
    }
}
// minv[r] = the smallest vertex of the tree of root r, size[r] = its vertices.  The lanes of a wave that share a root
// leave as one atomic each; a group of at least MSF_BIG_GROUP lanes is carried along by the wave while later groups have
// the same root and leaves once: V adds to the giant tree's word would retire at ~90 per microsecond, and on a permuted
// RMAT its vertices sit in every wave between isolated ones.
__global__ void __launch_bounds__(MSF_THREADS) msf_trees_kernel(const int32_t* __restrict__ parent, int64_t V, int32_t* __restrict__ minv, int32_t* __restrict__ size) {
    const int lane = threadIdx.x & 63;
    int32_t acc_root = -1, acc_n = 0, acc_min = INT32_MAX;   // (wave-uniform)
    const auto leave = [&](int32_t r, int32_t cnt, int32_t mn) {
        atomicAdd(&size[r], cnt);
        atomicMin(&minv[r], mn);
    };
    const int64_t stride = (int64_t) gridDim.x * blockDim.x;
    for (int64_t base = (int64_t) blockIdx.x * blockDim.x + threadIdx.x - lane; base < V; base += stride) {
        const int64_t v = base + lane;
        const int32_t r = v < V ? parent[v] : -1;
        unsigned long long rem = __ballot(v < V);
        while (rem) {   // (wave-uniform) one group of equal roots a step
            const int32_t gr = __shfl(r, __ffsll((long long) rem) - 1, 64);
            const unsigned long long same = __ballot(r == gr) & rem;
            const int32_t cnt = (int32_t) __popcll(same), mn = (int32_t) (base + __ffsll((long long) same) - 1);
            rem &= ~same;
            if (gr == acc_root) {
                acc_n += cnt;
                acc_min = min(acc_min, mn);
            } else if (cnt >= MSF_BIG_GROUP) {
                if (lane == 0 && acc_root >= 0) leave(acc_root, acc_n, acc_min);
                acc_root = gr;
                acc_n = cnt;
                acc_min = mn;
            } else if (lane == 0) {
                leave(gr, cnt, mn);
            }
        }
    }
    if (lane == 0 && acc_root >= 0) leave(acc_root, acc_n, acc_min);
}
__global__ void __launch_bounds__(MSF_THREADS) msf_flag_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ minv, int64_t V, int32_t* __restrict__ flag) {
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) flag[v] = minv[parent[v]] == v ? 1 : 0;
}
// comp[v] = rank of the smallest vertex of v's tree; the count and the largest tree
__global__ void __launch_bounds__(MSF_THREADS) msf_comp_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ minv, const int32_t* __restrict__ rank,
                                                               const int32_t* __restrict__ flag, const int32_t* __restrict__ size, int64_t V,
                                                               int32_t* __restrict__ comp, msf_ctl* __restrict__ ctl) {
    int32_t mx = 0;
    for (int64_t v = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t) gridDim.x * blockDim.x) {
        comp[v] = rank[minv[parent[v]]];
        mx = max(mx, size[v]);
        if (v == V - 1) ctl->comps = rank[v] + flag[v];
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&ctl->largest, (unsigned int) mx);
}

// ------------------------------------------------------------------ host
extern "C" int gmx_msf(gmx_graph_t* g, const int32_t* weight_host, uint8_t* in_forest_host, int64_t* num_edges, int64_t* total_weight, int32_t* comp_host,
                       int64_t* num_comps, gmx_stats_t* stats_out) {
    GMX_REQUIRE(g, "NULL argument");
    GMX_REQUIRE(in_forest_host || g->E == 0, "msf: in_forest is NULL");
    gmx_stats_t local_stats;
    gmx_stats_t* stats = stats_out ? stats_out : &local_stats;
    memset(stats, 0, sizeof(*stats));
    if (num_edges) *num_edges = 0;
    if (total_weight) *total_weight = 0;
    const int64_t V = g->V, E = g->E;
    if (num_comps) *num_comps = V;
    if (V == 0) return GMX_OK;
    if (E == 0) {   // every vertex is its own tree
        if (comp_host)
            for (int64_t v = 0; v < V; v++) comp_host[v] = (int32_t) v;
        if (comp_host) stats->vertices_reached = 1;
        return GMX_OK;
    }
    const int64_t tail_from = gmx_env_int("GMX_MSF_TAIL", MSF_TAIL, 0, INT64_MAX);   // read at every call; the result does not depend on it
    const bool phase_log = getenv("GMX_MSF_PHASES") != nullptr;                       // per-round device times for tools/msf_prof.py

    gmx_ws_scope scope;
    wbuf<int32_t> parent, l0, l1, weight, weight_sorted, inv, roots, to;
    wbuf<msf_word> best;
    wbuf<uint8_t> flag, in_forest;
    wbuf<unsigned int> atoms;
    wbuf<msf_ctl> ctl;
    GMX_CHECK(parent.alloc(V));
    GMX_CHECK(l0.alloc(V));
    GMX_CHECK(l1.alloc(V));
    GMX_CHECK(best.alloc(V));
    GMX_CHECK(flag.alloc(V));
    GMX_CHECK(in_forest.alloc(E));
    GMX_CHECK(roots.alloc(V));
    GMX_CHECK(to.alloc(V));
    GMX_CHECK(ctl.alloc(1));
    if (weight_host) GMX_CHECK(weight.alloc(E));
    if (weight_host && g->e_idx2idx.p) GMX_CHECK(weight_sorted.alloc(E));
    if (g->e_idx2idx.p) GMX_CHECK(inv.alloc(E));
    if (phase_log) GMX_CHECK(atoms.alloc(V));
    frontier_scan fs;
    GMX_CHECK(gmx_frontier_scan_alloc(&fs, (size_t) V, 0));
    gmx_pinned<msf_ctl> h_ctl;
    GMX_CHECK(h_ctl.alloc());
    const msf_ctl* h = h_ctl.p;
    gmx_spans tm;
    gmx_phase_clock phase;   // GMX_MSF_PHASES (synchronises: the profiler's mode only)
    GMX_CHECK(phase.enable(phase_log));
    const int gv = grid_for(V);

    // ---- the weights: uploaded by the caller's slots, brought into the order of the device's
    GMX_CHECK(tm.begin(tm.H2D));
    const int32_t* weight_dev = nullptr;
    if (weight_host) {
        GMX_HIP(hipMemcpy(weight.p, weight_host, sizeof(int32_t) * (size_t) E, hipMemcpyHostToDevice));
        weight_dev = weight.p;
        if (g->e_idx2idx.p) {
            hipLaunchKernelGGL(gather_by_order_kernel<int32_t>, dim3(grid_for(E)), dim3(BFS_THREADS), 0, 0, (const int32_t*) weight.p,
                               (const int32_t*) g->e_idx2idx.p, E, weight_sorted.p);
            weight_dev = weight_sorted.p;
        }
    }
    GMX_CHECK(tm.end(tm.H2D));

    msf_state S;
    S.begin = g->begin.p;
    S.idx = g->node_idx.p;
    S.weight = weight_dev;
    S.order = g->e_idx2idx.p;
    S.inv = g->e_idx2idx.p ? inv.p : nullptr;
    S.parent = parent.p;
    S.best = best.p;
    S.flag = flag.p;
    S.in_forest = in_forest.p;
    S.atoms = phase_log ? atoms.p : nullptr;
    S.ctl = ctl.p;
    S.V = V;

    GMX_CHECK(tm.begin(tm.KERNEL));
    GMX_HIP(hipMemsetAsync(ctl.p, 0, sizeof(msf_ctl), 0));
    GMX_HIP(hipMemsetAsync(flag.p, 0, (size_t) V, 0));
    GMX_HIP(hipMemsetAsync(in_forest.p, 0, (size_t) E, 0));
    if (phase_log) GMX_HIP(hipMemsetAsync(atoms.p, 0, sizeof(unsigned int) * (size_t) V, 0));
    if (S.inv) hipLaunchKernelGGL(msf_inverse_kernel, dim3(grid_for(E)), dim3(MSF_THREADS), 0, 0, S.order, E, inv.p);
    int32_t* la = l0.p;
    int32_t* lb = l1.p;
    hipLaunchKernelGGL(msf_next_kernel, dim3(grid_for(V, BFS_ITEMS)), dim3(MSF_THREADS), 0, 0, S, 1, la);
    GMX_HIP(hipGetLastError());
    GMX_CHECK(gmx_read_back(h_ctl, (const msf_ctl*) ctl.p));
    auto selected = [&] {
        msf_word c = 0;
        for (int i = 0; i < BFS_SHARDS; i++) c += h->shard[i].count;
        return (int64_t) c;
    };
    int64_t n = (int64_t) h->listed, m = (int64_t) h->next_slots;   // the list and the slots of its rows
    int64_t rounds = 0, grid_rounds = 0, tail_rounds = 0, slots = 0, count = 0;
    while (n > 0) {
        if (tail_from > 0 && m <= tail_from) {
            phase.begin();
            hipLaunchKernelGGL(msf_tail_kernel, dim3(1), dim3(MSF_TAIL_THREADS), 0, 0, S, la, lb, n, roots.p, to.p);
            GMX_HIP(hipGetLastError());
            GMX_CHECK(gmx_read_back(h_ctl, (const msf_ctl*) ctl.p));
            const float t = phase.end();
            tail_rounds = (int64_t) h->t_merging;
            rounds += tail_rounds;
            slots += (int64_t) h->t_slots;
            count = selected();
            if (phase_log)
                fprintf(stderr, "gmx msf tail: list %lld slots %lld rounds %lld read %lld tail %.3f ms\n", (long long) n, (long long) m,
                        (long long) h->t_rounds, (long long) h->t_slots, t);
            break;
        }
        float pt[3] = {0, 0, 0};
        GMX_HIP(hipMemsetAsync(&ctl.p->listed, 0, 2 * sizeof(msf_word), 0));
        phase.begin();
        GMX_CHECK(gmx_frontier_offsets(g->begin.p, la, n, &fs, nullptr, false));
        hipLaunchKernelGGL(msf_find_kernel, dim3((unsigned) frontier_tiles(n, m)), dim3(MSF_THREADS), 0, 0, S, (const int32_t*) la, n, (const int64_t*) fs.off.p, m);
        pt[0] = phase.end();
        phase.begin();
        hipLaunchKernelGGL(msf_hook_kernel, dim3(gv), dim3(MSF_THREADS), 0, 0, S);
        pt[1] = phase.end();
        phase.begin();
        hipLaunchKernelGGL(msf_next_kernel, dim3(grid_for(V, BFS_ITEMS)), dim3(MSF_THREADS), 0, 0, S, 0, lb);
        pt[2] = phase.end();
        if (phase_log) hipLaunchKernelGGL(msf_maxatom_kernel, dim3(gv), dim3(MSF_THREADS), 0, 0, atoms.p, V, ctl.p);
        GMX_HIP(hipGetLastError());
        GMX_CHECK(gmx_read_back(h_ctl, (const msf_ctl*) ctl.p));
        slots += m;
        const int64_t now = selected();
        if (phase_log) {
            fprintf(stderr, "gmx msf round %lld: list %lld slots %lld selected %lld find %.3f ms hook %.3f ms next %.3f ms max_atomics %u\n", (long long) rounds,
                    (long long) n, (long long) m, (long long) (now - count), pt[0], pt[1], pt[2], h->maxatom);
            GMX_HIP(hipMemsetAsync(&ctl.p->maxatom, 0, sizeof(unsigned int), 0));
        }
        if (now == count) break;   // no cross slot: the last round
        count = now;
        rounds++;
        grid_rounds++;
        n = (int64_t) h->listed;
        m = (int64_t) h->next_slots;
        std::swap(la, lb);
    }

    // ---- finish
    int32_t* comp = nullptr;
    if (comp_host) {
        wbuf<int32_t> minv, size, cflag, rank, cbuf;
        wbuf<char> scan_tmp;
        GMX_CHECK(minv.alloc(V));
        GMX_CHECK(size.alloc(V));
        GMX_CHECK(cflag.alloc(V));
        GMX_CHECK(rank.alloc(V));
        GMX_CHECK(cbuf.alloc(V));
        size_t scan_bytes = 0;
        GMX_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, cflag.p, rank.p, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
        GMX_CHECK(scan_tmp.alloc(scan_bytes));
        phase.begin();
        hipLaunchKernelGGL(msf_compress_kernel, dim3(gv), dim3(MSF_THREADS), 0, 0, parent.p, V, minv.p, size.p);
        hipLaunchKernelGGL(msf_trees_kernel, dim3(gv), dim3(MSF_THREADS), 0, 0, (const int32_t*) parent.p, V, minv.p, size.p);
        hipLaunchKernelGGL(msf_flag_kernel, dim3(gv), dim3(MSF_THREADS), 0, 0, (const int32_t*) parent.p, (const int32_t*) minv.p, V, cflag.p);
        GMX_HIP(rocprim::exclusive_scan((void*) scan_tmp.p, scan_bytes, cflag.p, rank.p, 0, (size_t) V, rocprim::plus<int32_t>(), 0));
        hipLaunchKernelGGL(msf_comp_kernel, dim3(gv), dim3(MSF_THREADS), 0, 0, (const int32_t*) parent.p, (const int32_t*) minv.p, (const int32_t*) rank.p,
                           (const int32_t*) cflag.p, (const int32_t*) size.p, V, cbuf.p, ctl.p);
        GMX_HIP(hipGetLastError());
        const float t = phase.end();
        if (phase_log) fprintf(stderr, "gmx msf finish: components %.3f ms\n", t);
        comp = cbuf.p;
    }
    GMX_CHECK(tm.end(tm.KERNEL));
    GMX_CHECK(gmx_read_back(h_ctl, (const msf_ctl*) ctl.p));
    GMX_CHECK(tm.begin(tm.D2H));
    GMX_HIP(hipMemcpy(in_forest_host, in_forest.p, (size_t) E, hipMemcpyDeviceToHost));
    if (comp) GMX_HIP(hipMemcpy(comp_host, comp, sizeof(int32_t) * (size_t) V, hipMemcpyDeviceToHost));
    GMX_CHECK(tm.end(tm.D2H));
    GMX_CHECK(tm.finish(stats));

    long long total = 0;
    for (int i = 0; i < BFS_SHARDS; i++) total += h->shard[i].weight;
    if (num_edges) *num_edges = count;
    if (total_weight) *total_weight = total;
    if (num_comps) *num_comps = V - count;
    if (comp && (int64_t) h->comps != V - count) {
        gmx_set_error("msf: %lld trees but %lld selected slots of %lld vertices", (long long) h->comps, (long long) count, (long long) V);
        return GMX_ERR_HIP;
    }
    stats->iterations = (int32_t) rounds;
    stats->vertices_reached = comp ? (int64_t) h->largest : 0;
    stats->edges_examined = slots;
    if (getenv("GMX_MSF_LOG"))
        fprintf(stderr, "gmx msf: V %lld E %lld reverse %d rounds %lld grid_rounds %lld tail_rounds %lld slots %lld forest_edges %lld weight %lld comps %lld\n",
                (long long) V, (long long) E, g->has_reverse ? 1 : 0, (long long) rounds, (long long) grid_rounds, (long long) tail_rounds, (long long) slots,
                (long long) count, total, (long long) (V - count));
    return GMX_OK;
}

void gmx_touch_msf() {
    hipFuncAttributes attr;
    (void) hipFuncGetAttributes(&attr, (const void*) msf_tail_kernel);
}
