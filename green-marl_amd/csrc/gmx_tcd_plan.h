// gmx_tcd_plan.h -- the plan gmx_tcd.hip builds from the forward CSR and caches on the graph, and how gmx_lcc.hip (gmx_clustering),
// gmx_ktruss.hip (gmx_ktruss), gmx_kclique.hip (gmx_kclique), gmx_squares.hip (gmx_squares) and gmx_graphlets.hip (gmx_graphlets) get at it: the lookup, the
// empty-graph probe, the group offsets, the symmetric adjacency, the sort by a key.
#ifndef GMX_TCD_PLAN_H_
#define GMX_TCD_PLAN_H_

#include "gmx_internal.h"

struct tcd_plan {
    int64_t V = 0, E = 0, E_up = 0;
    bool ordered = true;
    double build_ms = 0;
    dbuf<int32_t> out_begin, out_idx, up_begin, up_idx;
    dbuf<int64_t> grp_off;   // [V + 1]: the 64-slot groups of the OUT' rows
    dbuf<int32_t> perm;      // [V] caller's id -> plan's id; empty: the identity (ordered == false)
    dbuf<int32_t> deg;       // [V] |N(x)|, by the CALLER's id (where gmx_clustering's finishing kernel needs it)
    // gmx_clustering's additions, built on its first call on the plan (gmx_lcc.hip) and freed with it
    bool lcc_ready = false;
    dbuf<int64_t> up_grp_off;   // [V + 1]: the 64-slot groups of the UP' rows
    int64_t hubs = 0;           // the `hubs` highest plan ids, a multiple of 64 ...
    dbuf<uint32_t> hub_bits;    // ... and UP' among them as a hubs x hubs bit matrix: row u - (V - hubs), bit w - (V - hubs)
    double hub_ms = 0;
    // the symmetric adjacency, built by the first gmx_ktruss or gmx_squares call on the plan (tcd_plan_adjacency) and freed
    // with it: in plan ids, row v = DOWN'(v) then UP'(v) (sorted as it stands), with the edge id -- the position in up_idx --
    // of every slot, and the lower end of every edge id
    bool kt_ready = false;
    dbuf<int32_t> nb_begin;     // [V + 1]
    dbuf<int32_t> nb_idx;       // [2 E_up]
    dbuf<int32_t> nb_eid;       // [2 E_up]
    dbuf<int32_t> up_src;       // [E_up]: the row of edge id e in UP'
    // gmx_kclique's additions, built on its first call on the plan (gmx_kclique.hip) and freed with it: the vertices listed by
    // ascending d = |UP'(v)| (one device sort), and the offsets of the size classes in that list
    bool kc_ready = false;
    dbuf<int32_t> kc_vtx;           // [V]: plan ids by ascending d (ties: ascending id)
    dbuf<int32_t> kc_d;             // [V]: their d
    std::vector<int64_t> kc_below;  // [1026], host: kc_below[t] = vertices with d < t, so a class (lo, hi] is the list's [kc_below[lo + 1], kc_below[hi + 1])
    // gmx_squares's additions, built on its first call on the plan (gmx_squares.hip) and freed with it.  D(u) = |DOWN'(u)| is
    // nb_begin[u + 1] - nb_begin[u] - |UP'(u)| and u's DOWN' slots are numbered from nb_begin[u] - up_begin[u]
    bool sq_ready = false;
    dbuf<int32_t> sq_excl;          // [E_up]: per DOWN' slot (u, v) the sum of |{ w in N'(v') : w < u }| over the slots v' in front of it in u's row
    dbuf<uint32_t> sq_W;            // [V]: W(u), the sum over the whole row: the wedges of u
    dbuf<int32_t> sq_vtx;           // [V]: plan ids by ascending key (ties: ascending id); key = 0 where D(u) < 2, else W(u) + 1
    std::vector<uint32_t> sq_key;   // [V], host: their keys, where the class offsets of a call's thresholds are searched
    int64_t sq_wedges = 0;          // the sum of W(u) over the vertices with D(u) >= 2
};

// All in gmx_tcd.hip:
// *out = g's cached plan, built first if there is none or the cached one has the other order (*built: it was built by this call)
int tcd_plan_get(gmx_graph* g, bool ordered, tcd_plan** out, bool* built);
// *real = the forward slots of g that are no self loop when g has no plan yet (one kernel pass and a read-back), else the
// plan's E_up: zero exactly when there is no edge at all, which an entry asks before it has a plan built
int tcd_real_slots(const gmx_graph* g, int64_t* real);
// the plan's symmetric adjacency (nb_begin, nb_idx, nb_eid, up_src), built unless it is there (kt_ready)
int tcd_plan_adjacency(tcd_plan* p);
// gmx_lcc.hip: the 64-slot groups of the UP' rows (up_grp_off), built unless they are there (lcc_ready): the work items of
// gmx_clustering's walk and of gmx_graphlets' weighted one
int lcc_plan_groups(tcd_plan* p);
// gmx_ktruss.hip: sup[e] = the triangles on edge id e (kt_support_kernel), for an entry that keeps them on the device; the
// adjacency is there; enqueued on stream 0
int kt_support_into(tcd_plan* p, int32_t* sup);
// key_sorted[0, n) = key[0, n) ascending by the bits [0, end_bit), stable, and val_sorted[j] = where key_sorted[j] stood in
// key: the sort of the plan's vertices (edges) by a size that every member of the family does once per plan.  The values
// 0 .. n - 1 and rocPRIM's temporary storage come from the caller's workspace scope; enqueued on s.  *tmp_bytes (if asked
// for) = that storage's size once it is known, 0 before: a caller with its own GMX_ERR_NOMEM texts can tell which allocation it was
int tcd_sort_by_key(const uint32_t* key, uint32_t* key_sorted, int32_t* val_sorted, int64_t n, unsigned end_bit, hipStream_t s, size_t* tmp_bytes = nullptr);
// grp_off[0 .. V] (allocated here) = exclusive scan of the rows' 64-slot groups, a row of d = begin[v + 1] - begin[v] >= 2
// slots having ceil((d - 1) / 64); synchronises s.  Buf: where the temporaries come from, wbuf inside a workspace scope or
// dbuf (defined in gmx_tcd.hip, which instantiates exactly these two explicitly: another Buf is a link error)
template <template <typename> class Buf>
int tcd_group_offsets(const int32_t* begin, int64_t V, dbuf<int64_t>* grp_off, hipStream_t s);

#endif
