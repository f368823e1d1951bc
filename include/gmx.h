/*
 * gmx.h -- C ABI of the MI355X-native Green-Marl graph-kernel hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI: its hot path is the
 * body of three generated C++ functions
 *     void    pagerank(gm_graph& G, double e, double d, int32_t max, double* G_pg_rank);
 *     void    hop_dist(gm_graph& G, int32_t* G_dist, node_t& root);
 *     int64_t triangle_counting(gm_graph& G);
 * (signature rules: /root/reference/src/backend_cpp/gm_cpp_gen.cc:520-608,938-1017;
 *  call sites: apps/output_cpp/src/pagerank_main.cc:28, hop_dist_main.cc:28,
 *  triangle_counting_main.cc:14) that read gm_graph's public CSR arrays
 * (apps/output_cpp/gm_graph/inc/gm_graph.h:133-142).  The C++ entries with
 * exactly those signatures live in green-marl_amd/generated/ and are a few
 * lines each: they hand gm_graph's raw arrays to the functions below.
 * Everything here is extern "C", plain pointers and sizes, int status returns
 * (0 = ok; the reference has no error channel, so the C++ entries turn a
 * non-zero status into fprintf(stderr)+abort()).
 *
 * All file:line citations are relative to /root/reference.
 */
#ifndef GMX_H_
#define GMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMX_OK            0
#define GMX_ERR_ARG      -1   /* bad argument                       */
#define GMX_ERR_HIP      -2   /* a HIP runtime call failed          */
#define GMX_ERR_NODEVICE -3   /* no gfx950 device visible           */
#define GMX_ERR_NOMEM    -4
#define GMX_ERR_STATE    -5   /* object not in the required state   */

/* node_t / edge_t are int32 (gm_graph_typedef.h:17-18, the reference default). */
typedef int32_t gmx_node_t;
typedef int32_t gmx_edge_t;

typedef struct gmx_graph gmx_graph_t;     /* device-resident CSR (+ reverse CSR) */
typedef struct gmx_pr    gmx_pr_t;        /* device-resident PageRank state      */

/* Message for the last non-zero status returned on this thread. */
const char* gmx_last_error(void);

/* ---- device ---- */
int gmx_device_count(int* count);
int gmx_set_device(int device);
typedef struct {
    char     name[128];
    char     arch[32];          /* "gfx950..." */
    int32_t  compute_units;
    int32_t  clock_mhz;
    int64_t  hbm_bytes;
    int32_t  l2_bytes;
    int32_t  lds_bytes_per_cu;
} gmx_device_info_t;
int gmx_device_info(gmx_device_info_t* info);
/* Measured device-to-device copy rate (GB/s, bytes read + bytes written) of a `bytes`-sized buffer, `iters` copies:
 * the achievable HBM ceiling bench.py reports next to the data-sheet peak. */
int gmx_copy_bandwidth(int64_t bytes, int iters, double* gbs);

/* The multi-gigabyte temporaries of graph construction and plan builds come from a workspace that stays allocated for
 * the life of the process (freed device memory is wiped by the driver before reuse, and allocations that need it stall
 * for seconds at RMAT-26 sizes).  gmx_workspace_bytes: what it holds now; gmx_workspace_release: give it back (e.g. once
 * every graph and plan is built; anything built later allocates it again). */
int64_t gmx_workspace_bytes(void);
int gmx_workspace_release(void);

/* ---- graph: replaces the emitted prologue `G.freeze(); G.make_reverse_edges();
 *      [G.do_semi_sort();]` + Shoal copy-in (gm_cpp_gen.cc:1307-1368, 670-778) ---- */

#define GMX_GRAPH_SORT_ROWS    0x1u  /* rows of node_idx are not sorted yet: do_semi_sort on device   */
#define GMX_GRAPH_NO_REVERSE   0x2u  /* do not keep a reverse CSR (BFS top-down only / TC binary search) */
/* Without GMX_GRAPH_SORT_ROWS an upload that builds the reverse CSR on the device (r_begin NULL, no
 * GMX_GRAPH_NO_REVERSE) sorts the forward rows on the way when they are out of order, and then behaves exactly as if
 * GMX_GRAPH_SORT_ROWS had been passed: sorted rows on the device and an e_idx2idx map (gmx_graph_edge_order). */

/* Upload a host CSR.  begin[V+1], node_idx[E] = gm_graph::begin / node_idx.
 * r_begin / r_node_idx = gm_graph::r_begin / r_node_idx, or NULL: the reverse
 * CSR is then built on the device (gm_graph::make_reverse_edges, gm_graph.cc:205-304,
 * followed by do_semi_sort_reverse, :461-466).
 *
 * Validation (GMX_ERR_ARG, the message says what failed): begin[0] = 0, begin[V] = E, begin never decreases, and every
 * node_idx value lies in [0, V).  A reverse CSR the upload keeps (given, without GMX_GRAPH_SORT_ROWS and without
 * GMX_GRAPH_NO_REVERSE) is checked the same way (r_begin[0] = 0, r_begin[V] = E, ...).  These checks run on the device
 * copies, before anything is built from them.  That a given reverse CSR is the transpose of the forward one is NOT
 * checked: it is the caller's responsibility, and every entry that reads the reverse CSR trusts it.
 *
 * Sorted rows ("semi-sorted": every row non-decreasing).  Graphs built on the device (gmx_graph_from_edges,
 * gmx_graph_create_rmat, gmx_graph_symmetrize) and uploads through GMX_GRAPH_SORT_ROWS or a device-built reverse CSR
 * have sorted rows.  The other uploads keep the caller's arrays verbatim (with GMX_GRAPH_NO_REVERSE: the forward ones),
 * in whatever order their rows are, repeats apart from each other included; the validation pass records whether each
 * CSR's rows are sorted.  On such a graph:
 *   - gmx_pagerank_*, gmx_pr_*, gmx_hop_dist, gmx_bfs_*, gmx_bfs_levels, gmx_bc, gmx_bc_batch, gmx_bc_all, gmx_sssp, gmx_avg_teen_cnt, gmx_conduct,
 *     gmx_scc, gmx_wcc, gmx_kcore, gmx_msf, gmx_coloring, gmx_closeness, gmx_communities, gmx_potential_friends, gmx_triangle_counting_directed, gmx_triangle_counting_directed_part, gmx_clustering, gmx_kclique, gmx_squares, gmx_graphlets, gmx_louvain, gmx_v_cover, gmx_random_bipartite_matching, gmx_random_walk_sampling, gmx_node_sampling, gmx_sssp_path_f64, gmx_route_create / gmx_route_query / gmx_bidir_dijkstra and gmx_graph_symmetrize accept any row order and compute what the reference computes on the rows as
 *     stored (gmx_bc's float sums run in the stored slot order; gmx_sssp's len, gmx_sssp_path_f64's cost and prev_edge, the route entries' weight and path_edge, gmx_v_cover's select and gmx_msf's weight and in_forest are indexed by the stored slots);
 *   - gmx_triangle_counting, gmx_triangle_counting_part, gmx_triangle_counting_cn, gmx_common_nbrs,
 *     gmx_common_nbr_counts and gmx_adamic_adar binary-search rows, as the reference does on semi-sorted graphs only (shl_graph.cc:20,
 *     gm_common_neighbor_iter.h): GMX_ERR_STATE when the forward rows are not sorted.  With sorted forward rows and an
 *     unsorted reverse CSR, triangle counting takes the forward-only form of a GMX_GRAPH_NO_REVERSE graph. */
int gmx_graph_upload(const gmx_edge_t* begin, const gmx_node_t* node_idx,
                     const gmx_edge_t* r_begin, const gmx_node_t* r_node_idx,
                     int64_t V, int64_t E, uint32_t flags, gmx_graph_t** out);

/* Build from an unordered host edge list (src[i] -> dst[i]); rows come out
 * semi-sorted, multi-edges and self loops are kept. */
int gmx_graph_from_edges(const gmx_node_t* src, const gmx_node_t* dst,
                         int64_t V, int64_t E, uint32_t flags, gmx_graph_t** out);

/* create_RMAT_graph(N, M, rseed, a, b, c, permute) on the device, bit-compatible
 * with the reference's srand48/drand48 stream (graph_gen.cc:159-287), followed by
 * do_semi_sort + make_reverse_edges as load_binary does
 * (gm_graph_binary_loader.cc:191-197). */
int gmx_graph_create_rmat(int64_t N, int64_t M, long seed, double a, double b, double c,
                          int permute, uint32_t flags, gmx_graph_t** out);

/* Undirected simple version of g (both orientations, no duplicates, no self loops); the result is
 * its own transpose.  Measurement preparation of the triangle-counting config. */
int gmx_graph_symmetrize(const gmx_graph_t* g, gmx_graph_t** out);
/* The same calls for a host side built with GM_EDGE64 (edge_t = int64_t, gm_graph_typedef.h:8-20): edge offsets and edge
 * maps as int64 arrays.  The device keeps 32-bit edge offsets: E must be below 2^31 - 2^27 (GMX_ERR_ARG otherwise). */
int gmx_graph_upload_e64(const int64_t* begin, const gmx_node_t* node_idx, const int64_t* r_begin, const gmx_node_t* r_node_idx,
                         int64_t V, int64_t E, uint32_t flags, gmx_graph_t** out);
int gmx_graph_download_e64(const gmx_graph_t* g, int64_t* begin, gmx_node_t* node_idx, int64_t* r_begin, gmx_node_t* r_node_idx);
int gmx_graph_edge_order_e64(const gmx_graph_t* g, int64_t* e_idx2idx, int* is_identity);
int gmx_graph_reverse_edge_map_e64(const gmx_graph_t* g, int64_t* e_rev2idx);
int gmx_graph_free(gmx_graph_t* g);
int64_t gmx_graph_num_nodes(const gmx_graph_t* g);
int64_t gmx_graph_num_edges(const gmx_graph_t* g);
/* gm_graph's e_idx2idx[E] (gm_graph.h:141, do_semi_sort gm_graph.cc:468-503) after an upload that sorted the rows
 * (GMX_GRAPH_SORT_ROWS, or a device-built reverse CSR): for every slot of the sorted rows, the slot of the uploaded CSR
 * it came from (equal destinations keep their order).  *is_identity = 1 when the upload was already in order; e_idx2idx is then not
 * written.  Edge properties passed later (gmx_sssp's len) are indexed by the UPLOADED slots. */
int gmx_graph_edge_order(const gmx_graph_t* g, gmx_edge_t* e_idx2idx, int* is_identity);
/* gm_graph's e_rev2idx[E] (gm_graph.h:141-142): forward slot mirrored by each slot of the reverse CSR. */
int gmx_graph_reverse_edge_map(const gmx_graph_t* g, gmx_edge_t* e_rev2idx);
/* Copy the device CSR back (any pointer may be NULL).  Lets a host gm_graph be
 * filled from a device-generated graph. */
int gmx_graph_download(const gmx_graph_t* g, gmx_edge_t* begin, gmx_node_t* node_idx,
                       gmx_edge_t* r_begin, gmx_node_t* r_node_idx);

/* ---- run statistics (all optional outputs) ---- */
typedef struct {
    int32_t iterations;       /* pagerank: cnt; hop_dist: levels; tc: 1          */
    int32_t reserved;
    double  last_diff;        /* pagerank: diff of the last iteration            */
    double  kernel_ms;        /* device time of the timed hot loop (hipEvents)   */
    double  h2d_ms;           /* property copy-in  (Shoal copy-in analogue)      */
    double  d2h_ms;           /* property copy-out (Shoal copy-back analogue)    */
    int64_t edges_examined;   /* hop_dist: edges actually inspected              */
    int64_t vertices_reached; /* hop_dist                                         */
    int64_t edges_reached;    /* hop_dist: out-edges of the reached vertices (Graph500 TEPS numerator) */
} gmx_stats_t;

/* ---- whole-kernel entries (what the three generated C++ functions call) ---- */

/* pagerank(G, e, d, max, G_pg_rank): fp64 storage + fp64 arithmetic.
 * rank_host[V] is caller-owned (pagerank_main.cc:18-25) and written on return. */
int gmx_pagerank_f64(gmx_graph_t* g, double e, double d, int32_t max_iter,
                     double* rank_host, gmx_stats_t* stats);
/* Node_Prop<Float> variant (BASELINE config 2): fp32 STORAGE; partial row sums are formed in fp64, rounded to fp32 once
 * per (source tile, row) pair, added exactly in 64-bit fixed point and rounded once more per vertex.  Within 1e-6
 * relative of the fp64 result; not bit- or iteration-comparable with what gm_comp would emit
 * for a Float property (fp32 sums in thread order), whose iteration count near the threshold e may differ. */
int gmx_pagerank_f32(gmx_graph_t* g, float e, float d, int32_t max_iter,
                     float* rank_host, gmx_stats_t* stats);

/* hop_dist(G, G_dist, root): BFS depth along out-edges, INT_MAX = unreached. */
int gmx_hop_dist(gmx_graph_t* g, gmx_node_t root, int32_t* dist_host, gmx_stats_t* stats);

/* hop_dist over several GPUs: replicated CSR, every rank runs gmx_bfs_step_begin /
 * [exchange] / gmx_bfs_step_end per level until the frontier is empty.  step_begin runs a top-down level
 * entirely (needs_exchange = 0: every rank expands the whole, small frontier) or the rank's share of a
 * bottom-up level, writing its slice [slice_offset, slice_offset + slice_words) of the found bitmap
 * (64 vertices per word; needs_exchange = 1 when nranks > 1: all-gather the slices in place).  step_end
 * applies the bitmap to the rank's dist[] replica and returns the next frontier's size -- the same number on
 * every rank, so the ranks agree on direction and termination without further communication. */
typedef struct gmx_bfs gmx_bfs_t;
int gmx_bfs_create(gmx_graph_t* g, int rank, int nranks, gmx_bfs_t** out);
int gmx_bfs_free(gmx_bfs_t* b);
int gmx_bfs_start(gmx_bfs_t* b, gmx_node_t root);
int gmx_bfs_step_begin(gmx_bfs_t* b, int* needs_exchange);
int gmx_bfs_found_bitmap(gmx_bfs_t* b, void** words, int64_t* total_words, int64_t* slice_offset, int64_t* slice_words);
int gmx_bfs_step_end(gmx_bfs_t* b, int64_t* next_count);
int gmx_bfs_download(gmx_bfs_t* b, int32_t* dist_host, gmx_stats_t* stats);

/* The BFS object of `InBFS(v: G.Nodes From s) {..} InReverse {..}` (gm_bfs_template.h:14-312 as instantiated by
 * gm_cpp_gen_bfs.cc:88-275: level_t = short, save_child when DownNbrs is used).
 * gmx_bfs_levels = prepare(root) + do_bfs_forward(): level_host[V] as the template's visited_level (unvisited = -2,
 * gm_bfs_template.h:725), *nlevels = deepest level + 1.
 * gmx_bc = comp_BC(G, BC, Seeds) of apps/src/bc.gm (driver apps/output_cpp/src/bc_main.cc:43): for every seed, the
 * traversal, visit_fw (sigma = Sum over UpNbrs) level by level, visit_rv (delta = Sum over DownNbrs, BC += delta)
 * deepest level first; Float properties, every Sum added in row-slot order.  skip_root = 0 is this fork's bc.gm (the
 * root is visited like any vertex, so its sigma = 1 is overwritten by an empty sum: all sigma 0, NaN wherever a
 * reached vertex has a BFS child); skip_root = 1 is upstream Green-Marl's `(v != s)` form.  bc_host[V] is written. */
int gmx_bfs_levels(gmx_graph_t* g, gmx_node_t root, int16_t* level_host, int32_t* nlevels);
int gmx_bc(gmx_graph_t* g, const gmx_node_t* seeds, int32_t nseeds, int skip_root, float* bc_host, gmx_stats_t* stats);

/* gmx_bc_batch = gmx_bc with the seeds swept `width` at a time (bc_random(G, BC, K) of apps/src/bc_random.gm, driver
 * apps/output_cpp/src/bc_random_main.cc, draws its K seeds and makes one such call).
 * Result: bc_host[V] is byte-identical to gmx_bc(g, seeds, nseeds, skip_root, ...) for every width and every knob below.
 * What that means, per seed s (a column of a batch):
 *   - sigma[v] is the float sum over v's reverse-row slots whose source is one level up, added in slot order from +0.0f;
 *   - delta[v] is the float sum over v's forward-row slots whose target is one level down of
 *     sigma[v] / sigma[w] * (1 + delta[w]), in slot order; repeated slots count repeatedly;
 *   - BC[v] = BC[v] + delta[v] is applied once per seed, in seed order, only for the seeds that reach v, and with skip_root
 *     not for v == s;
 *   - skip_root = 0 is this fork's literal form (bc_random.gm has no (v != s) filter either): every sigma is 0 and the
 *     result is NaN where a reached vertex has a BFS child;
 *   - duplicate seeds are independent columns.
 * width: 0 = the library's choice (GMX_BCB_WIDTH if set, else the measured default, no wider than the seeds need);
 *   1 = gmx_bc's per-seed path itself; 16, 32, 64 = sources per batch; anything else GMX_ERR_ARG.
 * The other argument checks, a seed out of range among them, are gmx_bc's, and so is the error for a graph without its reverse CSR.
 * A batch takes V * (10 * width + 10) + 4096 * width bytes of device memory; when that exceeds the free memory, or
 * GMX_BCB_MEM_MB (MiB) when set, the width is halved down to 16 and below that the call runs per seed.  A batch in which a
 * seed's traversal is deeper than GMX_BCB_MAX_DEPTH levels (default and maximum 254: levels are kept as bytes) runs per
 * seed.  GMX_BCB_LONG_MIN (default 256): rows with at least that many slots are summed by a workgroup, shorter ones by a
 * lane group (1: every row, empty ones included, by a workgroup).  All are read at every call.  GMX_BCB_TRACE=1 prints one line per batch on stderr:
 *   gmx bc_batch batch <i>: seeds <n> width <w> depth <d> path <batched|per-seed> rows <s> short + <k> long, slots <n>
 * stats (may be NULL): iterations = nseeds, vertices_reached = gmx_bc's sum, kernel_ms by events, edges_examined = row
 * slots the batched sweeps walked (0 on the per-seed path). */
int gmx_bc_batch(gmx_graph_t* g, const gmx_node_t* seeds, int32_t nseeds, int skip_root,
                 int32_t width, float* bc_host /* [V] */, gmx_stats_t* stats);

/* gmx_bc_all = comp_BC(G, BC) of apps/src/bc_adj.gm (driver apps/output_cpp/src/bc_adj_main.cc): exact betweenness
 * centrality, every vertex a source in node order.  bc_host[V] holds the bytes of gmx_bc(g, {0, 1, .., V-1}, V, skip_root, ..);
 * skip_root = 1 is bc_adj.gm's `(v != s)` form.  width, the argument checks, the memory rule, the depth cap, the error for a
 * graph without its reverse CSR, the knobs, the trace and the stats are gmx_bc_batch's (iterations = V).  V = 0: GMX_OK.
 *
 * GMX_BCB_MSBFS (0 or 1, read at every call; default 0 for gmx_bc_batch, 1 for gmx_bc_all): the levels of a batch come
 * from one bit-parallel multi-source traversal over the reverse CSR -- a word of `width` bits per vertex, one chain of
 * launches and one host synchronisation per level for all columns -- in place of one traversal per seed.  Same bytes, same
 * stats, same memory (the mask words take the place of the staged levels).  GMX_BCB_MS_LONG_MIN (default 256): reverse rows
 * with at least that many slots are walked by a wave, shorter ones by a lane (1: every row by a wave).  With the knob on,
 * GMX_BCB_TRACE=1 prints after each batch's line
 *   gmx bc_batch msbfs batch <i>: levels <d> rows <s> short + <k> long slots <n> saturated <m>
 * (rows and slots the traversal walked -- a walk stops once every missing column is covered -- and the vertex visits
 * skipped because no column was missing whose front still held a vertex). */
int gmx_bc_all(gmx_graph_t* g, int skip_root, int32_t width, float* bc_host /* [V] */, gmx_stats_t* stats);

/* sssp(G, dist, len, root) (apps/src/sssp.gm; driver apps/output_cpp/src/sssp_main.cc:42): shortest path lengths
 * over out-edges with the caller's edge property len[E] (indexed by forward edge slot), INT_MAX = unreachable.
 * stats: iterations = relaxation rounds, h2d_ms = upload of len, vertices_reached = queue entries over all rounds. */
int gmx_sssp(gmx_graph_t* g, gmx_node_t root, const int32_t* len_host, int32_t* dist_host, gmx_stats_t* stats);

/* sssp_path(G, dist, len, root, prev) (apps/src/sssp_path.gm:1-30; driver apps/output_cpp/src/sssp_path_main.cc:44): gmx_sssp's
 * lengths together with a shortest-path tree.  len_host[E] is indexed like gmx_sssp's len, by the UPLOADED forward slots
 * (through e_idx2idx when the upload sorted the rows), and every value must be >= 0: a negative one gives GMX_ERR_ARG
 * (checked on the device copy before the traversal; the reference would run Bellman-Ford on it).  Path sums must stay
 * below INT_MAX, as for gmx_sssp.
 *   dist_host[V]       exactly what gmx_sssp returns for the same arguments; INT_MAX = unreached; a root outside [0, V)
 *                      gives INT_MAX everywhere.
 *   prev_node_host[V], prev_edge_host[V] (the latter may be NULL; sssp_path_adj.gm's prev_edge)
 *                      -1 (gm_graph::NIL_NODE / NIL_EDGE) for the root and for unreached vertices; otherwise a TIGHT
 *                      in-edge n -> v: prev_edge[v] = e as an UPLOADED forward slot, prev_node[v] = n its source, with
 *                      dist[n] != INT_MAX and dist[n] + len[e] == dist[v].  Following prev_node from any reached vertex
 *                      arrives at the root in fewer than V steps: prev is a shortest-path tree.
 * Canonical choice: the reference's prev depends on thread timing (the first writer of the round in which dist_nxt[v]
 * reached its final value).  Here, where every tight in-edge of v has positive length, prev_edge[v] is the SMALLEST
 * uploaded slot among them (uploaded slots are grouped by source, so prev_node[v] is the smallest tight predecessor): with
 * len >= 1 everywhere the whole output is fixed, bit-identical from run to run and independent of the schedule.  A vertex
 * with a tight in-edge of length 0 gets some tight in-edge, with only the tree property guaranteed.  This tree may differ
 * from the one a particular run of the reference produces; both are shortest-path trees of the same dist.
 * Only the forward CSR is read (a GMX_GRAPH_NO_REVERSE graph works), in any row order.  V = 0: GMX_OK.  E = 0: len_host
 * may be NULL.  stats as for gmx_sssp (iterations = relaxation rounds, kernel_ms, h2d_ms = upload and check of len,
 * edges_examined, vertices_reached = queue entries over all rounds), and d2h_ms = download of the three arrays.
 * GMX_SSSP_PATH_SCHEDULE = round | nearfar picks the schedule (DESIGN.md 4.2b'); the results do not depend on it. */
int gmx_sssp_path(gmx_graph_t* g, gmx_node_t root, const int32_t* len_host /* [E] */, int32_t* dist_host /* [V] */,
                  gmx_node_t* prev_node_host /* [V] */, gmx_edge_t* prev_edge_host /* [V] or NULL */, gmx_stats_t* stats);

/* sssp_path(G, dist, edge_cost, root, end, prev_node, prev_edge) of apps/src/sssp_path_adj.gm:1-33 (driver
 * apps/output_cpp/src/sssp_path_adj_main.cc:107): a route query from root to end with Double edge costs, a predecessor node
 * and a predecessor edge per vertex, pruned against the best distance to end found so far.  The program, per round:
 *     B = dist[end] as the round finds it (DBL_MAX, the emitted +INF, while end is unreached; always, with end = -1);
 *     every n with updated[n] && dist[n] < B, every out-slot e = n -> s: c = dist[n] + cost[e];
 *         if (c < B && dist_nxt[s] > c) { dist_nxt[s] = c; updated_nxt[s] = true; prev_node[s] = n; prev_edge[s] = e; }
 *     then dist = dist_nxt, updated = updated_nxt, updated_nxt = false; the loop ends when nothing is updated.
 * B is a round's value, so what a vertex at or beyond end's distance ends up with depends on the rounds (it may keep a
 * distance that is not its shortest): an asynchronous schedule computes something else there.  The device keeps the
 * synchronous rounds, and with them the whole output is deterministic:
 *   dist_host[V], prev_node_host[V], prev_edge_host[V] (the last may be NULL) are BYTE-IDENTICAL to what the loop above
 *   gives when ONE thread runs it on the graph as uploaded (vertices ascending, a row in uploaded slot order), on every
 *   vertex and for every upload form: per round a vertex whose dist_nxt dropped takes the minimum of the round's offers and,
 *   among the offers equal to it, the one of the smallest UPLOADED slot; a vertex that did not drop keeps its predecessor.
 *   prev_edge is an uploaded forward slot.  Unreached: DBL_MAX, -1, -1.  The root keeps 0, -1, -1 (costs are >= 0).
 * Note that this is not gmx_sssp_path's rule (the smallest tight in-edge overall): the winner is the smallest slot among
 * the offers of the round in which the final distance arrived.
 * cost_host[E] is indexed like gmx_sssp's len, by the UPLOADED forward slots (through e_idx2idx when the upload sorted the
 * rows).  Every cost must satisfy cost >= 0, checked on the device copy before the traversal: a negative cost or a NaN gives
 * GMX_ERR_ARG and gmx_last_error() names the first offending slot; nothing is written.  -0.0 passes (sums start from +0.0,
 * so no distance is ever -0.0); +inf passes and is never offered.  The one operation is dist[n] + cost[e] in double.
 * end = -1 (gm_graph::NIL_NODE): no target, the bound stays DBL_MAX and the call is a double-cost sssp_path over the whole
 * graph; any other end outside [0, V): GMX_ERR_ARG.  A root outside [0, V): DBL_MAX everywhere, -1 predecessors, GMX_OK
 * (gmx_sssp_path's convention).  g, dist_host or prev_node_host NULL: GMX_ERR_ARG.  V = 0: GMX_OK.  E = 0: cost_host may
 * be NULL.  Only the forward CSR is read (a GMX_GRAPH_NO_REVERSE graph works), rows in any order.
 * The per-vertex words, the lists and the device copies of cost are kept on the graph for the next call (24 V + 20 V + 8 E
 * bytes, 16 E when the upload sorted the rows) and freed with it; every call initialises what it reads.
 * A round is three launches over lists (offers and winners over the rows of the queue, commit over the vertices that
 * dropped; gmx_sssp_f64.hip, DESIGN.md 4.2b'').  Read at every call, the result does not depend on them:
 *   GMX_SSSP_F64_TAIL   while the queued rows hold at most this many slots one workgroup runs the rounds in one launch,
 *                       handing back to the grid when the queue outgrows it (0: never; huge: always; default 4096),
 *   GMX_SSSP_F64_LOG=1  one stderr line per call: V, E, root, end, the threshold, rounds (grid + tail, tail launches),
 *                       queue entries, slots, ms (2: before it a line per grid round and per tail launch).
 * stats: iterations = rounds of the loop in which some vertex was updated (0 for a root out of range), edges_examined = row
 * slots walked by the offer pass (the rows of the updated vertices below the bound), vertices_reached = updated vertices
 * summed over the rounds (the root's included).  The reference also visits the root a second time in round 2 (updated_nxt
 * starts as a copy of updated), where it offers what it offered in round 1 and nothing changes: that visit is neither run
 * nor counted.  kernel_ms = device time from the first to the last launch, h2d_ms = upload
 * and check of cost, d2h_ms = download of the three arrays. */
int gmx_sssp_path_f64(gmx_graph_t* g, gmx_node_t root, gmx_node_t end,
                      const double* cost_host /* [E] */, double* dist_host /* [V] */,
                      gmx_node_t* prev_node_host /* [V] */, gmx_edge_t* prev_edge_host /* [V] or NULL */,
                      gmx_stats_t* stats);

/* ---- route queries with Int edge weights: bidir_dijkstra(G, Weight, src, dst, Parent, ParentEdge) of
 * apps/src/bidir_dijkstra.gm and dijkstra(G, Len, root, dest, Parent, ParentEdge) of apps/src/sssp_dijkstra.gm (drivers
 * apps/output_cpp/src/bidir_dijkstra_main.cc:37, sssp_dijkstra_main.cc:37) ----
 * One source, one destination, one route back.  A search from src over out-edges and one from dst over in-edges run in
 * turns, each round expanding the side whose queue holds fewer row slots, and stop when the two balls meet; on a graph
 * without a reverse CSR (GMX_GRAPH_NO_REVERSE) the same code runs with the reverse side never expanded, which is
 * sssp_dijkstra.gm's one-sided search with early exit.  The weights stay on the device in a route object, so that many
 * pairs can be answered on one graph with one weight array (the drivers' pairs-file mode) without uploading it again.
 *
 * gmx_route_create: weight_host[E] is indexed like gmx_sssp's len, by the UPLOADED forward slots (through e_idx2idx when
 * the upload sorted the rows).  Every weight must be >= 0 (zero is allowed), checked on the device copy before anything
 * else: a negative one gives GMX_ERR_ARG, gmx_last_error() names the first offending slot, and no object is returned
 * (*out = NULL).  Path sums must stay below INT_MAX (gmx_sssp's convention).  The object keeps on the device the weights by
 * forward slot and, when the graph has a reverse CSR, by reverse slot, for each reverse slot the uploaded forward slot it
 * stands for (the two CSRs' slots paired in the order of their (dst, src) keys: any row order works, the reverse CSR
 * must be the transpose), and all per-vertex words and queues of a query: 12 E + 52 V bytes.  THE OBJECT BORROWS g: free
 * it before the graph.  E = 0: weight_host may be NULL.  V = 0: GMX_OK (there is no vertex to query).
 *
 * gmx_route_query answers one pair and uploads nothing beyond a few scalars; every call initialises what it reads.
 *   *found  1 iff dst is reachable from src over out-edges.  src == dst is found, with cost 0 and 0 hops.
 *   *cost   the shortest distance: exact, whatever the knobs.  Left alone when not found.
 *   *hops   the number of edges of the returned route (0 when not found).  path_node[k] is the k-th vertex AFTER src (the
 *           last one is dst; get_path does not push the start either), path_edge[k] the UPLOADED forward slot of the edge
 *           into path_node[k], also for the edges the reverse search walked.  Either array may be NULL.  With hops > cap
 *           the first cap entries from the src end are written, *hops still reports the full length, and the call is GMX_OK.
 *   The route: consecutive edges join up from src to dst, each path_edge lies in the row of its source and points at its
 *   path_node, the weights sum to *cost, no vertex repeats (so it has fewer than V edges) -- with zero weights, zero-weight
 *   cycles, parallel edges and self loops.  WHICH of several equally short routes is returned is NOT specified: it may
 *   differ between runs and between knob settings.
 *   src or dst outside [0, V), r, found, cost or hops NULL, cap < 0: GMX_ERR_ARG, nothing is written.
 *
 * gmx_bidir_dijkstra = create + query + free, what the drop-in entries call.  parent_host[V] / parent_edge_host[V] (the
 * latter may be NULL) are -1 everywhere except on the vertices of the returned route other than src, where they hold the
 * predecessor and its uploaded forward slot: get_path(src, dst) walks exactly that route.  Not found: all -1, *found = 0.
 *
 * Not reproduced from the reference (its frontier is gm_mutatable_priority_map_unordered_min, whose order among equal
 * keys is an accident of a heap, so there is no one-thread run to match):
 *   - bidir_dijkstra.gm leaves the residue of both searches in Parent and never initialises ParentEdge off the route;
 *     here both are -1 off the route;
 *   - for src == dst, bidir_dijkstra.gm reports a cycle through src, or False when there is none; here: found, cost 0,
 *     0 hops, all parents -1.
 *
 * Knobs, read at every call; the flag and the cost do not depend on them:
 *   GMX_ROUTE_SIDES=both|forward  forward: never expand the reverse side (default both when a reverse CSR exists);
 *   GMX_ROUTE_TAIL=<slots>        while the side to expand holds at most this many slots one workgroup runs the rounds of
 *                                 both sides in one launch, handing back to the grid when a queue outgrows it (0: never;
 *                                 huge: always; default 4096);
 *   GMX_ROUTE_LOG=1               one stderr line per query:
 *     gmx route: V <V> E <E> src <s> dst <d> sides <both|forward>; tail <slots>; rounds F <n> grid + <n> tail, R <n> grid + <n> tail
 *     in <n> launches; slots F <n> R <n>; queued <n>; found <0|1> cost <c> meet <v> hops <h>; ms <t>
 * stats: iterations = rounds, both sides counted; edges_examined = row slots walked, both sides counted; vertices_reached
 * = queue entries (the two seeds included); kernel_ms = device time from the first launch to the route's extraction, d2h_ms
 * = download of the route; h2d_ms = upload, check and gathers of the weights, filled by gmx_bidir_dijkstra only (a query
 * uploads nothing).  Design and the argument for the stop rule: DESIGN.md 4.2b'''. */
typedef struct gmx_route gmx_route_t;
int gmx_route_create(gmx_graph_t* g, const int32_t* weight_host /* [E] */, gmx_route_t** out);
int gmx_route_free(gmx_route_t* r);
int gmx_route_query(gmx_route_t* r, gmx_node_t src, gmx_node_t dst, int32_t* found, int64_t* cost,
                    gmx_node_t* path_node /* [cap] or NULL */, gmx_edge_t* path_edge /* [cap] or NULL */,
                    int64_t cap, int64_t* hops, gmx_stats_t* stats);
int gmx_bidir_dijkstra(gmx_graph_t* g, const int32_t* weight_host /* [E] */, gmx_node_t src, gmx_node_t dst,
                       gmx_node_t* parent_host /* [V] */, gmx_edge_t* parent_edge_host /* [V] or NULL */,
                       int32_t* found, gmx_stats_t* stats);

/* avg_teen_cnt(G, age, teen_cnt, K) (apps/src/avg_teen_cnt.gm; driver avg_teen_cnt_main.cc:24) and
 * conduct(G, member, num) (apps/src/conduct.gm; driver conduct_main.cc:45): count-reductions over neighbours
 * with the caller's int32 node property; integers exact, the returned float formed by the emitted expression. */
int gmx_avg_teen_cnt(gmx_graph_t* g, const int32_t* age_host, int32_t K, int32_t* teen_cnt_host, float* avg, gmx_stats_t* stats);
int gmx_conduct(gmx_graph_t* g, const int32_t* member_host, int32_t num, float* result, gmx_stats_t* stats);

/* kosaraju(G, mem) (apps/src/kosaraju.gm; driver apps/output_cpp/src/kosaraju_main.cc): the strongly connected
 * components.  *num_comps = their number and comp_host[V] = the component of every vertex -- the same partition and count
 * as the reference, but numbered CANONICALLY: ids run densely over 0 .. count-1 in increasing order of each component's
 * smallest vertex id (the reference numbers them in its sequential DFS finish order).  Deterministic from run to run.
 * Needs the reverse CSR (GMX_ERR_STATE after an upload with GMX_GRAPH_NO_REVERSE).  stats: iterations = outer
 * trim / FW-BW / colouring rounds, vertices_reached = size of the largest SCC, edges_examined = edge slots inspected,
 * kernel_ms = device time, d2h_ms = download of comp. */
int gmx_scc(gmx_graph_t* g, int32_t* comp_host, int64_t* num_comps, gmx_stats_t* stats);

/* Weakly connected components (the reference has no such program): two vertices are in one component when a path joins
 * them with every edge usable in both directions.  The result follows gmx_scc's conventions, so the two can be compared
 * directly (on a symmetric graph they are equal): comp_host[V] = the component of every vertex, ids dense over
 * 0 .. count-1 in increasing order of each component's smallest vertex id, *num_comps = the count.  The bytes are identical
 * from run to run and under every knob below.
 * g == NULL or comp_host == NULL: GMX_ERR_ARG, checked before any device call.  num_comps and stats may be NULL.  V = 0:
 * GMX_OK with count 0.  E = 0: the identity with count V.  Self loops and repeated slots are harmless; rows are read in
 * any order (no GMX_ERR_STATE for unsorted rows).  A GMX_GRAPH_NO_REVERSE graph is accepted and gives the same arrays: only
 * the work differs.  Nothing is cached on the graph.
 * The scheme is Afforest's: K sampling rounds link every vertex with its out-slots 0 .. K-1, the most
 * frequent root g* among 1024 fixed probes names the tree to skip, and the final pass links the whole out-rows and
 * in-rows of the vertices outside that tree -- or, without a reverse CSR, the out-rows of every vertex.
 * stats: iterations = sampling rounds + 1, vertices_reached = size of the largest component, kernel_ms = device time from
 * the first launch to the last (renumbering included), d2h_ms = download of comp, edges_examined = slots read: one per
 * (vertex, round r) with outdeg(v) > r, plus every slot of every row the final pass walks (whole rows, the first K slots
 * of an out-row that sampling already read included); without a reverse CSR or with GMX_WCC_SKIP=0 that is exactly
 * sum_v min(K, outdeg v) + E.
 * Read at every call, the result does not depend on them:
 *   GMX_WCC_SAMPLE_ROUNDS  K, default 2, 0 .. 8,
 *   GMX_WCC_SKIP           0: every vertex is live and only out-rows are walked, as without a reverse CSR,
 *   GMX_WCC_GIANT          <vertex>: g* = that vertex's root after sampling (for tests),
 *   GMX_WCC_LOG            one line per call on stderr: `gmx wcc: V <V> E <E> sample_rounds <K> sampled <n> giant <root>
 *                          skipped <s> live <l> reverse <0|1> final_slots <n> comps <c> largest <m>`, with
 *                          skipped + live = V and sampled + final_slots = edges_examined,
 *   GMX_WCC_PHASES         the device time of the five phases on stderr (tools/wcc_prof.py). */
int gmx_wcc(gmx_graph_t* g, int32_t* comp_host, int64_t* num_comps, gmx_stats_t* stats);

/* k-core decomposition (the reference has no such program): core numbers and the rounds of the peeling that finds them.
 * Slots and degree: every stored slot u -> w with u != w counts once, a repeated slot counts again; self-loop slots are
 * read but ignored.  mode names the slots that make a vertex's degree and the rows that removing it walks: */
#define GMX_KCORE_IN   0   /* degree = in-slots;  removing v lowers the heads of v's out-row */
#define GMX_KCORE_OUT  1   /* degree = out-slots; removing v lowers the tails of v's in-row  */
#define GMX_KCORE_BOTH 2   /* degree = in-slots + out-slots; both rows are walked            */
/* core_host[V]: core[v] = the largest k such that v lies in a set S whose every vertex has degree >= k, counting only slots
 * with both ends in S.  On a symmetric graph (gmx_graph_symmetrize) IN and OUT are the k-core number of the undirected
 * graph and BOTH is twice that.  *max_core = the largest core number.
 * layer_host[V] (or NULL: no layer array is kept or downloaded): the round that removed v under this schedule, which fixes
 * layer and the statistics (core is unique anyway): level k is the smallest degree among the live vertices (the first may
 * be 0); round 0 of a level removes every live vertex of degree <= k, round r+1 those whose degree fell to <= k because of
 * round r's removals; when a round removes nothing the next level starts; the rounds that removed something are numbered
 * 0, 1, 2, ... across the whole run.  On a simple undirected graph layer + 1 is the "onion layer" of v, and sorting by
 * layer gives a degeneracy ordering.  core and layer are byte-identical from run to run and under every knob below: a
 * vertex is queued once, by the decrement that returns k + 1, and rounds are separated by a kernel boundary or a barrier.
 * g == NULL, core_host == NULL (checked before g is touched) or a mode outside 0 .. 2: GMX_ERR_ARG before any device call.
 * layer_host, max_core and stats may be NULL.  V = 0: GMX_OK, *max_core = 0.  Rows are read in any order.  IN reads only
 * the forward rows and takes the in-degrees from the reverse CSR's offsets when the graph has one, otherwise from a
 * histogram of the heads: a GMX_GRAPH_NO_REVERSE graph gives the same arrays.  OUT and BOTH need the reverse CSR:
 * GMX_ERR_STATE without it.  A degree above INT32_MAX (BOTH only): GMX_ERR_ARG.  Nothing is cached on the graph.
 * stats: iterations = rounds that removed something, vertices_reached = vertices with core == max_core, edges_examined =
 * slots of the rows walked by removals (every vertex is removed once: E for IN and OUT, 2 E for BOTH), kernel_ms = device
 * time from the first launch to the last, d2h_ms = the downloads.
 * Read at every call, the result does not depend on them:
 *   GMX_KCORE_TAIL    one workgroup runs the rounds (and the level scans) while the queue to expand holds at most this many
 *                     slots (the live list at most as many entries); 0: never; default 1024,
 *   GMX_KCORE_LOG     one line per call on stderr: `gmx kcore: V <V> E <E> mode <m> reverse <0|1> levels <l> rounds <r>
 *                     scanned <n> grid_rounds <g> tail_rounds <t> slots <s> max_core <k> top <n>`, with grid_rounds +
 *                     tail_rounds = rounds = iterations, slots = edges_examined, top = vertices_reached and scanned = the sum
 *                     over the levels of the live list's length at the level's start (the list is compacted by every
 *                     level's scan: it holds the vertices that were live after round 0 of the level before),
 *   GMX_KCORE_PHASES  the device time of degrees, level scans, grid rounds and tail launches and the largest number of decrements
 *                     one vertex received, on stderr (tools/kcore_prof.py). */
int gmx_kcore(gmx_graph_t* g, int mode, int32_t* core_host, int32_t* layer_host, int32_t* max_core, gmx_stats_t* stats);

/* Minimum spanning forest (the reference has no such program): Boruvka's algorithm in synchronous rounds.
 * Graph read: every stored forward slot u -> w with u != w is an undirected edge {u, w} of weight weight_host[slot]
 * (weight_host[E] by UPLOADED forward slot, as gmx_sssp's len; NULL: every weight 0); a repeated slot is another edge;
 * self-loop slots are read and ignored.  Only the forward CSR is read, in any row order: a GMX_GRAPH_NO_REVERSE graph gives
 * the same bytes.  Nothing is cached on the graph.
 * Order: edges are ordered by (weight, uploaded slot), lexicographic, over the whole int32 range, negative weights
 * included.  That is a strict total order, so the minimum spanning forest is unique: in_forest_host[E] (by uploaded slot,
 * 0 / 1) is exactly what Kruskal's algorithm selects when it takes the slots in that order, byte-identical from run to
 * run, under every knob below, and between an upload that kept the caller's rows and one that sorted them (the tie-break
 * is the uploaded slot, not the device's).  weight_host == NULL: a spanning forest with ties to the lowest slot.
 * *num_edges = the selected slots = V - *num_comps, *total_weight = their int64 sum.  comp_host[V] (or NULL: no component
 * array is built or downloaded) and *num_comps equal gmx_wcc's, with the same canonical numbering.
 * g == NULL, or in_forest_host == NULL with E > 0 (checked before g is touched otherwise): GMX_ERR_ARG before any device
 * call.  The other pointers may be NULL.  V = 0 or E = 0: GMX_OK, no slot selected, comp the identity.
 * The schedule, which fixes the statistics (the forest is unique anyway): round 0 lists every vertex that has an out-slot;
 * a round reads every slot of every listed row; a slot is cross when its two ends lie in different trees at the round's
 * start; every tree takes the smallest key among the cross slots that touch it, at either end; all chosen slots are
 * selected and their trees merged; round r+1 lists the vertices that had a cross out-slot in round r, tested before round
 * r's merges; the run ends when the list is empty or a round finds no cross slot.  At most ceil(log2 V) rounds merge.
 * stats: iterations = rounds that merged something, edges_examined = slots read over all rounds (the last, empty round
 * included), vertices_reached = the largest component when comp_host is given, else 0, kernel_ms = device time from the
 * first launch to the last, h2d_ms = the weights, d2h_ms = the downloads.
 * Read at every call, neither the result nor the statistics depend on them:
 *   GMX_MSF_TAIL    one workgroup runs all remaining rounds once the list's rows hold at most this many slots (they never
 *                   grow again); 0: never; default 4096,
 *   GMX_MSF_LOG     one line per call on stderr: `gmx msf: V <V> E <E> reverse <0|1> rounds <r> grid_rounds <g> tail_rounds
 *                   <t> slots <s> forest_edges <n> weight <w> comps <c>`, with g + t = r = iterations and slots =
 *                   edges_examined,
 *   GMX_MSF_PHASES  per round the device time of its three steps and the largest number of atomics one tree's word
 *                   received, the tail launch and the finish, on stderr (tools/msf_prof.py; synchronises at every step). */
int gmx_msf(gmx_graph_t* g, const int32_t* weight_host, uint8_t* in_forest_host, int64_t* num_edges, int64_t* total_weight, int32_t* comp_host,
            int64_t* num_comps, gmx_stats_t* stats);

/* Greedy vertex colouring (the reference has no such program): first fit in a fixed vertex order, which is unique, computed
 * in parallel rounds by the Jones-Plassmann schedule; colour class 0 is the greedy (lexicographically first) maximal
 * independent set of the same order.
 * Graph: every stored forward slot u -> w with u != w makes u and w neighbours, in whichever direction it is stored; a
 * repeated slot is harmless, self-loop slots are read and ignored, rows are read in any order.  The neighbourhood of a
 * vertex is its out-row plus its in-row, so the entry needs the reverse CSR: GMX_ERR_STATE on a GMX_GRAPH_NO_REVERSE graph.
 * A graph stored in one direction only gives the same bytes as its symmetrised form.  Nothing is cached on the graph.
 * Order: u is earlier than w when (prio[u], -u) > (prio[w], -w): the larger priority first, ties to the lower id.
 * prio_host[V], or NULL: prio[v] = outdeg(v) + indeg(v), all stored slots counted (repeats and self loops included) from
 * the CSR offsets alone, as an unsigned 32-bit sum: largest degree first.  The priority is a key only; any int32 values
 * are compared without overflow.  prio_host all zero: first fit in id order.
 * color_host[V]: color[v] = the smallest colour >= 0 that no earlier neighbour of v holds -- what one thread produces when
 * it takes the vertices in that order.  *num_colors = the largest colour + 1 (0 for V = 0).
 * depth_host[V] (or NULL: nothing is kept or downloaded): the number of vertices on the longest chain of successively
 * earlier neighbours that ends at v, minus 1; 0 when v has no earlier neighbour.  depth is defined on the graph and the
 * order; under the schedule below it is the round that coloured v.  Both arrays are byte-identical from run to run, under
 * every knob below and between upload forms.
 * g == NULL or color_host == NULL (checked before g is touched): GMX_ERR_ARG before any device call.  prio_host,
 * depth_host, num_colors and stats may be NULL.  V = 0: GMX_OK.  E = 0 or only self loops: every colour 0 in one round.
 * Schedule (it fixes the statistics): round 0 colours every vertex without an earlier neighbour, round r+1 those whose
 * last earlier neighbour was coloured in round r; rounds are separated by a kernel boundary or a workgroup barrier.  A
 * ready vertex takes the smallest colour none of its neighbours holds (the later ones hold none yet), then lowers the
 * pending count of every neighbour without a colour; the decrement that returns 1 queues that neighbour exactly once.
 * stats: iterations = rounds = max(depth) + 1, vertices_reached = the size of colour class 0, edges_examined = 6 E (both
 * rows of every vertex are read to count, to colour and to release; the extra window passes below are not counted),
 * kernel_ms = device time from the first launch to the last, h2d_ms = the priorities, d2h_ms = the downloads.
 * Read at every call, neither the result nor the statistics depend on them:
 *   GMX_COLOR_TAIL       one workgroup runs the rounds while the queue holds at most this many entries + row slots; 0:
 *                        never; default 1024,
 *   GMX_COLOR_WAVE_MIN   rows (out-slots + in-slots) of at least this many slots are coloured by a wave with a bitmap in
 *                        LDS, shorter ones by 16 lanes with a 64-bit mask; at most and by default 65,
 *   GMX_COLOR_BLOCK_MIN  rows of at least this many slots are coloured by a workgroup; at most 8192 (the bits of a wave's
 *                        LDS slice), default 256,
 *   GMX_COLOR_WINDOW     bits of the workgroup's bitmap, a multiple of 64 in 64 .. 262144 (default: 32 KB of LDS); a row
 *                        that may need a colour beyond it is walked again per window of colours, floor(color / window)
 *                        extra passes,
 *   GMX_COLOR_LOG        one line per call on stderr: `gmx color: V <V> E <E> user_prio <0|1> rounds <r> grid_rounds <g>
 *                        tail_rounds <t> group <n> wave <n> block <n> passes <p> colors <c> class0 <n>`, with g + t = r =
 *                        iterations, group + wave + block = V, passes = the extra window passes, colors = *num_colors
 *                        and class0 = vertices_reached,
 *   GMX_COLOR_PHASES     the device time of count, colour per regime, release and tail launches on stderr
 *                        (tools/color_prof.py). */
int gmx_coloring(gmx_graph_t* g, const int32_t* prio_host, int32_t* color_host, int32_t* depth_host, int32_t* num_colors, gmx_stats_t* stats);

/* Closeness, harmonic centrality and eccentricity (the reference has no such program): the hop distances between every
 * vertex and a set of sources, folded per vertex into four exact integers.  With them come the diameter (max ecc), the
 * radius (min ecc over vertices with reach > 0) and the Wiener index (sum of far).  mode names the direction: */
#define GMX_CLOSE_OUT  0   /* d(v -> s): v's distances TO the sources along out-edges; pulls over forward rows; forward CSR only */
#define GMX_CLOSE_IN   1   /* d(s -> v): distances FROM the sources to v; pulls over reverse rows; needs the reverse CSR        */
#define GMX_CLOSE_BOTH 2   /* stored slots read as undirected edges; pulls over both rows; needs the reverse CSR               */
/* Sources: sources == NULL means every vertex is a source (nsources is ignored).  Otherwise the sums run over the listed
 * sources only (pivot sampling; what the estimate means is the caller's business); a source listed twice is two
 * independent columns and counts twice.  A source outside [0, V) or nsources < 0: GMX_ERR_ARG.  nsources == 0 with a list:
 * all-zero outputs, GMX_OK.
 * Per vertex v, with D(v, s) the hop distance in the mode's direction, over the columns s with 0 < D(v, s) < infinity (a
 * column whose source is v itself contributes nothing):
 *   reach_host[v] = the number of such columns,
 *   far_host[v]   = sum of D,
 *   ecc_host[v]   = max of D, 0 when reach[v] == 0,
 *   harm_host[v]  = sum of R(D) with R(l) = floor(2^32 / l) in 64-bit integer arithmetic: harm / 2^32 is the harmonic
 *                   centrality from below, 0 <= exact - harm / 2^32 < reach * 2^-32.
 * The fixed point is deliberate: all four outputs are integer sums or maxima, so they do not depend on any order.  THE
 * BYTES OF ALL FOUR ARRAYS ARE IDENTICAL UNDER EVERY KNOB, SWEEP WIDTH AND ROW REGIME BELOW, FROM RUN TO RUN AND BETWEEN
 * UPLOAD FORMS, AND EQUAL A ONE-THREAD BFS FROM EVERY SOURCE.  Closeness (reach / far), the Wasserman-Faust form and harm /
 * 2^32 as doubles are derived on the host (gmx.py closeness_of / harmonic_of, generated/closeness.cc), never on the device.
 * Any output pointer and stats may be NULL.  g == NULL or a mode outside 0 .. 2: GMX_ERR_ARG.  V = 0: GMX_OK.  IN or BOTH
 * on a graph without its reverse CSR: GMX_ERR_STATE; OUT works on a GMX_GRAPH_NO_REVERSE graph.  Rows are read in any
 * order; repeats and self loops are harmless.  Nothing is cached on the graph.
 * Schedule: the sources are taken 64 * words at a time (a sweep); a sweep is a bit-parallel multi-source traversal with
 * `words` 64-bit words per vertex in each of seen / front / next.  Level l >= 1 is one pass over all vertices: a vertex that
 * misses no column whose front is not empty only clears its next words (saturated); the others OR the front words over
 * their row -- by their own lane, or listed and by a wave for rows of at least GMX_CLOSE_LONG_MIN slots -- until every
 * missing column is covered, and add the popcount of the new columns to their own four accumulators.  No atomic touches
 * the state or a result after the seeding.  A sweep ends with the first level that finds nothing; the host reads the
 * new-pair counts of GMX_CLOSE_BATCH levels in one copy (at most one read per level), and a level launched past the
 * sweep's last finds every vertex saturated and changes nothing.  There is NO DEPTH CAP: levels are int32 and nothing
 * is stored per level.  The cost with all sources is
 * (V / (64 * words)) sweeps x depth levels, each a pass over the vertices: the entry is meant for graphs up to about 2^18
 * vertices with all sources, or for pivot lists on large ones.
 * stats: iterations = level passes launched (each sweep's final empty one included), vertices_reached = pairs = sum of
 * reach, edges_examined = row slots read, kernel_ms = device time from the first launch to the last (events), h2d_ms =
 * the source list, d2h_ms = the downloads.
 * Read at every call; the outputs and pairs do not depend on them, the other statistics do:
 *   GMX_CLOSE_WORDS     1, 2 or 4 words per vertex (64, 128 or 256 sources a sweep), halved while half as many words
 *                       still hold all the sources; default 4,
 *   GMX_CLOSE_BATCH     levels launched per host read, 1 .. 4; default 4; levels is a multiple of it,
 *   GMX_CLOSE_LONG_MIN  rows of at least this many slots (BOTH: forward + reverse) are walked by a wave; 1: every row;
 *                       default 128,
 *   GMX_CLOSE_LOG       one line per call on stderr: `gmx close: V <n> E <n> mode <m> sources <n> words <B> sweeps <n> levels
 *                       <n> lane <n> wave <n> saturated <n> slots <n> pairs <n>`, with sweeps = ceil(sources / (64 B)),
 *                       lane + wave + saturated = V * levels, levels = iterations, slots = edges_examined and pairs =
 *                       vertices_reached. */
int gmx_closeness(gmx_graph_t* g, int mode, const gmx_node_t* sources, int32_t nsources, int64_t* far_host, int32_t* reach_host, int32_t* ecc_host,
                  uint64_t* harm_host, gmx_stats_t* stats);

/* communities(G, comm) (apps/src/communities.gm:1-24; driver apps/output_cpp/src/communities_main.cc:19): label-propagation
 * community detection.  comm[x] = x; then every vertex x counts the labels of its out-neighbours, once per slot (a
 * repeated slot counts again, a self loop counts x's own label), keeps its label if that label has the highest count, and
 * otherwise takes the most frequent one -- until nothing changes.  Three things the reference leaves to its map class and
 * to thread timing are fixed here:
 *   tie        among the labels with the highest count the SMALLEST is taken (what gm_map_small's ordered iteration gives,
 *              gm_map.h:165-177), and only when the vertex's own label is not among them;
 *   no edges   a vertex without out-neighbours keeps its label (GetMaxKey on an empty map is undefined in the reference);
 *   schedule   the reference updates comm in place from many threads.  Here round r = 0, 1, ... is two half-rounds: vertex v
 *              belongs to half  h(v, r) = fmix32(uint32(v) ^ (uint32(r) * 0x9E3779B9u)) & 1,  fmix32 the murmur3 finaliser
 *              (h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16).  Half 0 runs first, then
 *              half 1; a half-round evaluates its vertices against one snapshot of comm and all its new labels are stored
 *              together before the next half-round starts.  This is one interleaving of the reference's loop, it is
 *              deterministic, and it converges where plain synchronous rounds swap labels for ever (a star, a 2-cycle).
 * Rounds run until one changes no label or max_rounds rounds have run (a directed chain needs about V of them under any
 * schedule).  *rounds = rounds that changed a label; *converged = 1 exactly when comm_host is a fixpoint of the rule (every
 * vertex with out-neighbours holds a label whose count over its row is the row's maximum) -- what any terminating run of
 * the reference returns -- decided, when max_rounds cut the run, by one more evaluation pass that writes nothing.
 * comm_host[V]: labels are vertex ids in [0, V); bit-identical from run to run (integer counts only).
 * max_rounds < 0 or comm_host == NULL: GMX_ERR_ARG.  rounds, converged, stats may be NULL.  V = 0: GMX_OK.  E = 0 or
 * max_rounds = 0: the identity labels, converged as defined.  Rows are read in any order, with repeats: no GMX_ERR_STATE
 * for unsorted rows.  Only the forward CSR is needed; with a reverse CSR only the vertices whose rows saw a label change
 * are evaluated again (GMX_COMM_WORKLIST=0 turns that off), which changes the work and not the result: a
 * GMX_GRAPH_NO_REVERSE graph gives identical arrays.  GMX_COMM_WAVE_MIN, GMX_COMM_BLOCK_MIN and GMX_COMM_LDS_SLOTS (read
 * at every call) move the row-length thresholds between the three evaluation kernels and size their tables (DESIGN.md
 * 4.2e); the results do not depend on them.
 * stats: iterations = *rounds, kernel_ms = device time from the first launch to the last commit, d2h_ms = download of
 * comm, vertices_reached = vertex evaluations over all half-rounds, edges_examined = slots read by them. */
int gmx_communities(gmx_graph_t* g, int32_t max_rounds, gmx_node_t* comm_host /* [V] */,
                    int32_t* rounds, int32_t* converged, gmx_stats_t* stats);

/* potential_friends(G, potFriend) (apps/src/potential_friends.gm:1-8; driver apps/output_cpp/src/potential_friends_main.cc:18):
 *     Foreach(v) Foreach(u: v.Nbrs)(u != v) Foreach(w: u.Nbrs)(w != u && w != v) If (!v.HasEdgeTo(w)) v.potFriend.Add(w);
 * the friends of friends that v has no edge to.  u is itself a slot of row(v), so the filters u != v and w != u never change
 * what is added, and the result is the set
 *     PF(v) = ( union of row(u) over the slots u of row(v) )  minus  row(v)  minus  {v}.
 * A set: repeated slots and self loops change nothing.  The result covers the vertices v_lo <= v < v_hi as a CSR:
 *   pf_begin_host[v_hi - v_lo + 1]   pf_begin[0] = 0, pf_begin[i + 1] - pf_begin[i] = |PF(v_lo + i)|; always written;
 *   *total                           pf_begin[v_hi - v_lo]; always written (total may be NULL);
 *   pf_idx_host[cap]                 pf_idx[pf_begin[i] .. pf_begin[i + 1]) = PF(v_lo + i), ASCENDING and distinct (the order in
 *                                    which gm_node_set iterates, gm_set.h:289-343, in both of its forms).
 * Sizing protocol, as for gmx_common_nbrs: pf_idx_host is written only when it is not NULL and *total <= cap; otherwise not
 * one element of it is touched and the call still returns GMX_OK.  The caller sizes with pf_idx_host = NULL, cap = 0 and calls
 * again.  The sizing call evaluates the set sizes only; it does not pay for a fill.
 * GMX_ERR_ARG unless 0 <= v_lo <= v_hi <= V, pf_begin_host != NULL and cap >= 0.  An empty range, V = 0 or E = 0: GMX_OK with an
 * all-zero pf_begin.  The reference decides HasEdgeTo by binary search and needs semi-sorted rows; this entry does not: rows
 * are read in any order, with repeats, and there is no GMX_ERR_STATE.  Only the forward CSR is read: a GMX_GRAPH_NO_REVERSE
 * graph gives identical arrays.  Sets and integers only: the result is bit-identical from run to run.  Counts, prefix sums
 * and two-hop lengths are 64-bit on host and device.
 * Device memory is bounded whatever the result size: the filled lists are staged in a device buffer of at most
 * GMX_PF_BATCH_BYTES (default 256 MiB) and copied to pf_idx_host batch by batch over consecutive vertices; a single set
 * larger than the budget forms a batch of its own.  Everything else (lengths, counts, row lists, bitmaps) comes from the
 * workspace.
 * Knobs, read from the environment at every call; the results do not depend on them.  With
 * L(v) = sum of outdeg(u) over the slots u of row(v), the two-hop items of v:
 *   GMX_PF_WAVE_MAX    (128)      the largest L evaluated by one wave with a table in LDS;
 *   GMX_PF_BLOCK_MAX   (2048)     the largest L evaluated by a workgroup with a table in LDS; longer rows use a V-bit map;
 *   GMX_PF_LDS_SLOTS   (4096)     slots of the workgroup's table, a power of two in [512, 16384] (a wave's table has an
 *                                 eighth); a row whose table fills is evaluated with a bit map instead;
 *   GMX_PF_LDS_BITS    (1048576)  the largest V whose bit map stays in LDS (at most 1048576 = 128 KiB); above it every
 *                                 workgroup of the grid has a map in global memory;
 *   GMX_PF_BATCH_BYTES.
 * stats: iterations = batches downloaded (0 for a sizing call), edges_examined = the sum of L(v) over the range (exact),
 * vertices_reached = vertices of the range with a non-empty set, kernel_ms = device time, d2h_ms = the downloads. */
int gmx_potential_friends(gmx_graph_t* g, gmx_node_t v_lo, gmx_node_t v_hi,
                          int64_t* pf_begin_host /* [v_hi - v_lo + 1] */,
                          gmx_node_t* pf_idx_host /* [cap] or NULL */, int64_t cap,
                          int64_t* total, gmx_stats_t* stats);

/* triangle_counting(G) with the emitted multiplicity rule. */
int gmx_triangle_counting(gmx_graph_t* g, int64_t* count, gmx_stats_t* stats);
/* Multi-GPU form (replicated CSR, final all-reduce of int64): the count contributed by part
 * `part` of `nparts` of the edge slots (dealt in blocks, round-robin); the parts add up to the full count. */
int gmx_triangle_counting_part(gmx_graph_t* g, int part, int nparts, int64_t* count, gmx_stats_t* stats);

/* triangle_counting_directed(G) (apps/src/triangle_counting_directed.gm):
 *     Foreach(v) Foreach(u: v.Nbrs) Foreach(w: v.Nbrs)(w > u)
 *         If (w.HasEdgeFrom(u) || w.HasEdgeTo(u)) T++;
 * With adj(u, w) = (u -> w in E or w -> u in E):
 *     T = sum over v of #{ ordered slot pairs (i, j) of row v : node_idx[i] < node_idx[j], adj(node_idx[i], node_idx[j]) }.
 *   - Repeated slots of row v count multiply, as in gmx_triangle_counting; the adjacency test is boolean.
 *   - Self loops take part literally: with v in row(v), every pair (v, w) with w != v of that row counts, because v -> w
 *     exists.  A pair needs two distinct values, so a self loop alone adds nothing.
 *   - HasEdgeTo / HasEdgeFrom are set membership: the reference binary-searches a semi-sorted row (gm_graph.cc:60-66) and
 *     its generated prologue semi-sorts, so on rows in any order the result is defined by membership, not by a failed search.
 *   - `w > u` only picks every unordered pair of distinct values of a row once: T does not depend on the vertex numbering.
 *   - On a symmetric graph without self loops and repeated slots T = 3 x gmx_triangle_counting: every triangle is seen
 *     once from each corner.
 * g == NULL, count == NULL or a part outside [0, nparts): GMX_ERR_ARG.  V = 0 or E = 0: GMX_OK with *count = 0.  Rows are
 * read in any order, with repeats, and only the forward CSR is read: a GMX_GRAPH_NO_REVERSE graph works and there is no
 * GMX_ERR_STATE.  The first call on a graph builds a plan from the forward CSR (two CSRs renumbered by ascending undirected
 * degree and the work items), cached on the graph and freed with it; its transient buffers are 2 x 2E
 * 64-bit keys, and when they or the plan cannot be allocated the call returns GMX_ERR_NOMEM and the message says how many
 * bytes were asked for.  Integers only: the count is exact and the same from run to run.
 * gmx_triangle_counting_directed_part: the work items (a vertex and 64 slots of its row) are dealt round-robin to nparts
 * parts; the parts' counts add up to the whole for any nparts.
 * Knobs, read from the environment at every call; the count does not depend on them:
 *   GMX_TCD_NO_ORDER=1   the plan keeps the graph's numbering (the cached plan is rebuilt when the knob changes);
 *   GMX_TCD_CAP          (1024) row entries a wave stages in LDS, clamped to [64, 1024]; longer rows are searched in memory;
 *   GMX_TCD_ALONE        (4) a lane walks a side of up to this many entries by itself;
 *   GMX_TCD_RATIO        (4) a wave streams the upper list of u while it is at most this many times the tail of the row;
 *   GMX_TCD_LOG=1        one line on stderr per call: the plan, the work items staged and in memory, the slots per regime.
 * stats: iterations = 1, kernel_ms = the count kernel only (the plan is graph preprocessing); everything else zero. */
int gmx_triangle_counting_directed(gmx_graph_t* g, int64_t* count, gmx_stats_t* stats);
int gmx_triangle_counting_directed_part(gmx_graph_t* g, int part, int nparts, int64_t* count, gmx_stats_t* stats);

/* Per-vertex triangle counts and local clustering coefficients (the reference has no such program).
 * Graph read: the stored slots as an undirected simple graph, as gmx_wcc, gmx_msf and gmx_closeness in mode BOTH read them:
 *     N(v) = { u != v : v -> u or u -> v is stored };  self loops and repeated slots change nothing.
 *   deg_host[V]  (int32)  deg[v] = |N(v)|;
 *   tri_host[V]  (int64)  tri[v] = #{ unordered {u, w} in N(v) : w in N(u) }, the triangles through v;
 *   lcc_host[V]  (double) lcc[v] = (double) (2 * tri[v]) / (double) ((int64) deg[v] * (deg[v] - 1)) when deg[v] >= 2, else +0.0:
 *                one IEEE division of two exact integers (numpy gives the same bytes from the same integers);
 *   *triangles = (sum of tri) / 3, *wedges = sum of deg (deg - 1) / 2.  Transitivity is 3 * triangles / wedges, the average
 *                clustering coefficient the mean of lcc; both are left to the caller.
 * Each of the three arrays may be NULL: it is then neither written nor downloaded.  wedges and stats may be NULL.  The arrays
 * are indexed by the caller's vertex ids.  Integers only on the device: everything is exact and byte-identical from run to run
 * and under every knob below.
 * triangles == NULL (checked before g is touched) or g == NULL: GMX_ERR_ARG before any device call.  V = 0: GMX_OK, nothing is
 * written.  E = 0 or self loops only: GMX_OK, zero arrays, *triangles = *wedges = 0.  Rows are read in any order, with repeats,
 * and only the forward CSR is read: a GMX_GRAPH_NO_REVERSE graph works and there is no GMX_ERR_STATE.
 * Plan: gmx_triangle_counting_directed's, cached on the graph and shared with it (whichever of the two is called first builds
 * it; GMX_LCC_NO_ORDER and GMX_TCD_NO_ORDER each rebuild a cached plan of the other order).  The first gmx_clustering call adds
 * the work items of the upper lists and the adjacency among the H highest plan ids as an H x H bit matrix (H = 65536, or
 * 131072 above 2^24 vertices, at most V, rounded down to a multiple of 64; rebuilt when H changes).  When the plan, the matrix
 * or the call's per-vertex scratch cannot be allocated: GMX_ERR_NOMEM, and the message gives the byte count.
 * On a symmetric graph without self loops and repeated slots *triangles = gmx_triangle_counting and
 * 3 * *triangles = gmx_triangle_counting_directed.
 * Knobs, read from the environment at every call; the results do not depend on them:
 *   GMX_LCC_NO_ORDER=1   the plan keeps the graph's numbering; no hub matrix then (the highest ids are no hubs);
 *   GMX_LCC_HUBS         H (0: no hubs);
 *   GMX_LCC_CAP          (1024) upper-list entries a wave stages in LDS, clamped to [64, 1024]; longer ones are searched in memory;
 *   GMX_LCC_ALONE        (4) a lane walks a side of up to this many entries by itself;
 *   GMX_LCC_RATIO        (4) a wave streams the upper list of u while it is at most this many times the tail;
 *   GMX_LCC_HUB_TAIL     (4) against a hub u the tail is probed while it is at most this many times the upper list of u;
 *   GMX_LCC_PLAIN=1      the credits of the third corner as one global atomic per match instead of the packed LDS counters
 *                        (the form the counters are measured against, tools/lcc_prof.py);
 *   GMX_LCC_LOG=1        one line on stderr per call: `gmx clustering: plan V <V> E <E> up <|UP'|> order <degree|identity>
 *                        built <0|1> build_ms <ms> hubs <H> hub_ms <ms>; cap <c> alone <a> ratio <r> hub_tail <t> w <lds|global>;
 *                        items <staged> staged + <memory> memory; slots <alone> alone + <list> list + <tail> tail + <hub> hub +
 *                        <empty> empty; credits <lds> lds + <global> global`: work items by where their list is searched, slots
 *                        by regime (alone: walked by one lane, bit probes included; hub: bit probes by the wave), third-corner
 *                        credits by route (lds + global = *triangles).
 * stats: iterations = 1, kernel_ms = the count kernel and the finishing kernel (the plan is graph preprocessing),
 * edges_examined = |UP'| (the undirected edges), vertices_reached = vertices with tri > 0, d2h_ms = the downloads. */
int gmx_clustering(gmx_graph_t* g, int64_t* tri_host, int32_t* deg_host, double* lcc_host, int64_t* triangles, int64_t* wedges, gmx_stats_t* stats);

/* Bridges, articulation points, biconnected components (blocks) and 2-edge-connected components (the reference has no
 * such program).  As gmx_clustering reads it, the stored slots form an undirected simple graph: every forward slot u -> w
 * with u != w denotes the edge {u, w}, w -> u and repeats of either denote the same edge, self-loop slots are read and
 * ignored.  Any row order.  The entry walks out-rows and in-rows, so it needs the reverse CSR: GMX_ERR_STATE on a
 * GMX_GRAPH_NO_REVERSE graph.  Nothing is cached on the graph.
 * bridge_host[E], by UPLOADED forward slot: 1 when the slot's edge is a bridge (its removal disconnects its component);
 * every slot of that edge gets it, self-loop slots get 0.  *num_bridges counts undirected edges, not slots.
 * artic_host[V]: 1 when removing v raises the number of components.  *num_artic = their number.
 * block_host[E], by uploaded slot: the biconnected component of the slot's edge, -1 for a self-loop slot.  The ids are
 * dense over 0 .. *num_blocks - 1 and increase with each block's smallest uploaded slot, so they are identical between a
 * verbatim upload and a sorting upload of the same arrays.
 * tecc_host[V]: the 2-edge-connected component of v -- its component once the bridges are removed -- numbered exactly as
 * gmx_wcc numbers components: dense, by smallest vertex, an isolated vertex its own component.  *num_tecc = their number
 * = the weak components + *num_bridges.
 * The result is unique: all arrays are exact and byte-identical from run to run and under every knob below.
 * g == NULL: GMX_ERR_ARG before any device call.  Every output pointer and stats may be NULL; an array that is NULL is
 * neither built nor downloaded.  V = 0: GMX_OK with all counts 0.  E = 0: no blocks, tecc is the identity.
 * Method (it fixes the statistics): the roots are the smallest vertex of every weak component (gmx_wcc's forest).  One
 * level-synchronous BFS from all roots over out-rows and in-rows gives level[] and par[w] = the smallest vertex of the
 * previous level with a slot to w.  Every forward slot u -> w that is no self loop and no tree slot (par[u] != w and
 * par[w] != u) then walks its tree cycle: of the two cursors x = u, y = w the one of the greater level (x on a tie) has
 * its tree edge joined to the class of the walk's first edge and moves to its parent, until they meet.  The classes of
 * tree edges are the blocks; a tree edge alone in its class is a bridge.  A cursor may jump: skip[v] = t records that all
 * tree edges from v up to its ancestor t are in one class, written by every walk for the vertices it moved from.
 * stats: iterations = levels of the spanning forest (max level + 1), vertices_reached = tree edges = V - weak components,
 * edges_examined = cursor moves of the walks (`steps`: with GMX_BICC_SKIP=0 exactly the sum over the walked slots of the
 * two path lengths to the lowest common ancestor, else a number that depends on the order of the walks), kernel_ms =
 * device time from the first launch to the last, d2h_ms = the downloads, h2d_ms = 0.
 * Read at every call, no result byte depends on them:
 *   GMX_BICC_TAIL    one workgroup runs the BFS levels while the level's rows hold at most this many slots; 0: never;
 *                    default 1024,
 *   GMX_BICC_SKIP    0: no jumps and no skip[] writes; default 1,
 *   GMX_BICC_WALKS   at most this many forward slots per walk launch, in device slot order, so that later walks see the
 *                    facts of earlier ones; 0: one launch; default 1048576,
 *   GMX_BICC_LOG     one line per call on stderr: `gmx bicc: V <V> E <E> levels <l> roots <r> tree <t> walks <w> steps <s>
 *                    jumps <j> links <k> grid_levels <g> tail_levels <t> blocks <b> bridges <b> artic <a> tecc <c>`, with
 *                    g + t = l = iterations, tree = vertices_reached, steps = edges_examined, walks = the walked slots,
 *                    links = the joins that found two different class roots; a count that was not asked for is -1,
 *   GMX_BICC_PHASES  the device time of forest, walks and finish on stderr (tools/bicc_prof.py). */
int gmx_biconnected(gmx_graph_t* g, uint8_t* bridge_host, uint8_t* artic_host, int32_t* block_host, int32_t* tecc_host, int64_t* num_blocks,
                    int64_t* num_bridges, int64_t* num_artic, int64_t* num_tecc, gmx_stats_t* stats);

/* k-truss decomposition and per-edge triangle support (the reference has no such program).  The stored slots are read
 * exactly as gmx_clustering reads them, N(v) = { u != v : v -> u or u -> v is stored }: self loops and repeated slots change
 * nothing, rows may be in any order, and only the forward CSR is read (a GMX_GRAPH_NO_REVERSE graph works; there is no
 * GMX_ERR_STATE).
 * support_host[E], by UPLOADED forward slot: |N(u) & N(w)| for the slot u -> w, the triangles through its edge.  Every slot
 * of one undirected edge gets the same value, in either direction and including repeats; self-loop slots get 0.
 * truss_host[E], by uploaded slot: the truss number of the slot's edge, the largest k such that the edge lies in a subgraph
 * in which every edge is in at least k - 2 triangles of that subgraph: at least 2 for every real edge, 0 for a self-loop
 * slot.  *max_truss = the largest truss number (0 when there is no edge), *num_edges = the undirected edges.
 * Each array may be NULL and is then neither built nor downloaded.  truss_host == NULL means no peeling at all: the call
 * stops after the support phase (the cheap "triangles per edge" query), *max_truss = 0 and iterations = 0.  With both NULL
 * only *num_edges is produced.  num_edges and stats may be NULL.
 * g == NULL, or max_truss == NULL (checked before g is touched): GMX_ERR_ARG before any device call.  V = 0: GMX_OK, no array
 * is written, the counts are 0.  E = 0 or self loops only: GMX_OK, zero arrays, answered without a plan.  When the plan's
 * additions or the call's per-edge scratch cannot be allocated: GMX_ERR_NOMEM, and the message gives the byte count.  More
 * than 2^30 - 1 undirected edges: GMX_ERR_ARG (the symmetric adjacency has 32-bit offsets).
 * The device uses integers only; truss numbers are unique by definition and support is a count: both arrays are
 * byte-identical from run to run and under every knob, and between a verbatim and a sorting upload of the same arrays.
 * Method (it fixes the statistics):
 *   plan     gmx_triangle_counting_directed's and gmx_clustering's, cached on the graph and shared with both (whichever entry
 *            is called first builds it; GMX_KTRUSS_NO_ORDER, GMX_LCC_NO_ORDER and GMX_TCD_NO_ORDER each rebuild a cached
 *            plan of the other order).  The edge id of an undirected edge is its position in the plan's upper lists.  The
 *            first gmx_ktruss call adds the symmetric adjacency in plan ids with the edge id of every slot, built from the
 *            upper lists with one device sort, and frees it with the plan.
 *   support  one work item per edge id: the shorter row of its two ends is walked, the longer one binary-searched; no atomics.
 *   peeling  synchronous rounds over one word sup[e] per edge that only falls by atomic decrements, and a round stamp per
 *            edge ("not queued", or the round that removes it).  A level's value s is the smallest sup among the live edges
 *            (levels jump to it, as gmx_kcore's do); round 0 of a level stamps and queues every live edge with sup <= s.  A
 *            round processes its queue: every queued edge e = {a, b} gets truss s + 2, and for every x in N(a) & N(b), with
 *            e1 = {a, x} and e2 = {b, x} (the shorter row is walked -- ties: the lower plan id -- the longer one searched),
 *            the triangle still exists when neither e1 nor e2 was removed in an EARLIER round.  Then: both in this round's
 *            queue: nothing; only e1: e2 is decremented iff id(e) < id(e1), and symmetrically; neither: both are
 *            decremented.  Each vanishing triangle so decrements each surviving edge exactly once.  The decrement that
 *            returns s + 1 stamps the edge with the next round and appends it to the next queue, exactly once; edges already
 *            queued for the next round keep being decremented.  When a round queues nothing, a compacting scan of the live
 *            list finds the next s.  Rounds that removed something are numbered 0, 1, 2, ... across the run; they are
 *            separated by a kernel boundary or, in the one-workgroup tail, by a barrier.  The queue's rows go through the
 *            merge-path tile (in the tail: a wave per row); a queue entry is the end with the shorter row.
 * Every loop ends by construction: no kernel waits for a value another workgroup writes, a tail launch returns to the host
 * when its queue outgrows its capacity or no edge is left, and the host loop is bounded by "every level removes at least one
 * edge" (a level that queues nothing is GMX_ERR_HIP).
 * stats: iterations = rounds that removed something, vertices_reached = undirected edges with truss == *max_truss,
 * edges_examined = slots of the shorter rows walked by the removals = the sum over the edges of min(deg(a), deg(b)),
 * independent of order and knobs (0 without peeling), kernel_ms = device time from the first launch after the plan to the
 * last (the plan and its additions are graph preprocessing), d2h_ms = the downloads, h2d_ms = 0.
 * Read at every call, no result byte depends on them:
 *   GMX_KTRUSS_NO_ORDER=1  the plan keeps the graph's numbering;
 *   GMX_KTRUSS_TAIL        one workgroup runs the rounds (and the level scans between them) while the queue's rows hold at most
 *                          this many slots; 0: never; default 1024, taken over from gmx_kcore (flat from 0 to 4096 on RMAT-20);
 *   GMX_KTRUSS_LOG         one line per call on stderr: `gmx ktruss: plan V <V> E <E> up <|UP'|> order <degree|identity>
 *                          built <0|1> adj_built <0|1>; support plain triangles <T>; levels <l> rounds <r> scanned <n>
 *                          grid_rounds <g> tail_rounds <t> slots <s> max_truss <k> top <n>`, with g + t = r = iterations, slots =
 *                          edges_examined, top = vertices_reached, T = the sum of the supports / 3 and scanned = the entries of
 *                          the live lists the level scans read (no line when the call is answered without a plan or with
 *                          both arrays NULL);
 *   GMX_KTRUSS_PHASES      the device time of the plan additions, support, level scans, grid rounds, tail launches and finish, and the
 *                          largest number of decrements one edge received, on stderr (tools/ktruss_prof.py). */
int gmx_ktruss(gmx_graph_t* g, int32_t* truss_host, int32_t* support_host, int32_t* max_truss, int64_t* num_edges, gmx_stats_t* stats);

/* k-clique counting, in total and through every vertex, 3 <= k <= 8 (the reference has no such program).  The stored slots
 * are read exactly as gmx_clustering and gmx_ktruss read them, N(v) = { u != v : v -> u or u -> v is stored }: self loops and
 * repeated slots change nothing, rows may be in any order, and only the forward CSR is read (a GMX_GRAPH_NO_REVERSE graph
 * works; there is no GMX_ERR_STATE).
 * *cliques = the number of k-element vertex sets that are pairwise adjacent.  count_host[V] (int64, by the caller's vertex
 * id) = the number of those sets that contain v, so that sum(count) == k * *cliques; k = 3 gives gmx_clustering's tri[] and
 * triangles.  count_host may be NULL and is then neither built nor downloaded: the cheap total-only query, whose last level is
 * a popcount and not an enumeration.  All sums are 64-bit and wrap modulo 2^64.  stats may be NULL.
 * cliques == NULL, k outside 3 .. 8 or g == NULL (checked in this order, before g is touched): GMX_ERR_ARG before any device
 * call.  V = 0: GMX_OK, nothing is written but *cliques = 0.  E = 0 or self loops only: GMX_OK, zeros, answered without a plan.
 * When the plan's additions, the per-vertex scratch or the global class's matrices cannot be allocated: GMX_ERR_NOMEM, and the
 * message gives the byte count.  Without the degree order an upper list whose bit matrix has 2^31 words or more (over 2^18
 * entries) is GMX_ERR_ARG; the degree order keeps every list below 2^16 entries.
 * Integers only: both results are unique and byte-identical from run to run and under every knob.
 * Method:
 *   plan     gmx_triangle_counting_directed's, gmx_clustering's and gmx_ktruss's, cached on the graph and shared with them
 *            (whichever entry is called first builds it; GMX_KCLIQUE_NO_ORDER, GMX_KTRUSS_NO_ORDER, GMX_LCC_NO_ORDER and
 *            GMX_TCD_NO_ORDER each rebuild a cached plan of the other order).  The first gmx_kclique call adds the vertices
 *            listed by ascending d = |UP'(v)| (one device sort) and the offset of every d <= 1025 in that list, and frees
 *            them with the plan.
 *   matrix   for a plan vertex v with S = UP'(v) (ascending plan ids, local index = position in S), row i of the local bit
 *            matrix is A[i] = { j > i : S_j in UP'(S_i) }: UP'(S_i) is streamed and searched in S.
 *   count    a k-clique whose lowest plan id is v is a (k-1)-clique of that local DAG: P_1 = all; choose i_1, P_2 = A[i_1];
 *            choose i_2 in P_2, P_3 = P_2 & A[i_2]; ... after k - 2 choices the last set is only popcounted.  Only the chosen
 *            indices are kept; a word of P_t is the AND of at most six rows' words and is recomputed where it is read.
 *   credits  a chosen index gets its subtree's total when the walk returns, the members of the last set +1 each into 64-bit
 *            counters per local index, v the vertex total; the counters are flushed once per vertex to an array in plan ids,
 *            which is permuted back on the device before the download.
 *   classes  one launch each over a range of the list: wave (d <= 64: a word per row, a wave per vertex, a lane per i_1),
 *            small (d <= min(256, cap)) and large (d <= cap): a workgroup per vertex with matrix, counters and list in
 *            dynamic LDS (11 KiB; 140 KiB, one workgroup per CU), a wave per i_1 and a lane per i_2; global (d > cap): the
 *            same with matrix and counters in workspace memory, one workgroup per vertex, dealt in batches; skipped
 *            (d < k - 1): never launched.
 * Every loop ends by construction and no kernel waits for a value that another workgroup writes.
 * stats: iterations = 1, edges_examined = |UP'|, vertices_reached = the vertices with count > 0 (0 when count_host == NULL),
 * kernel_ms = device time from the first launch after the plan to the last (the plan and its additions are graph
 * preprocessing), d2h_ms = the downloads, h2d_ms = 0.
 * Read at every call, no result byte depends on them:
 *   GMX_KCLIQUE_NO_ORDER=1     the plan keeps the graph's numbering;
 *   GMX_KCLIQUE_CAP            the large class's bound, default 1024, clamped to [64, 1024]: lowered, small graphs reach the
 *                              global class;
 *   GMX_KCLIQUE_WAVE=0         the wave class goes to the small class's kernel;
 *   GMX_KCLIQUE_BATCH_BYTES    matrices and counters of one global-class launch, default 256 MiB (a vertex that needs more
 *                              is a batch by itself);
 *   GMX_KCLIQUE_PLAIN=1        every per-vertex credit as one global atomic, without the counters (the form they are measured
 *                              against);
 *   GMX_KCLIQUE_LOG=1          one line on stderr: `gmx kclique: plan V <V> E <E> up <|UP'|> order <degree|identity> built <0|1>
 *                              classes_built <0|1>; k <k> cap <c> counts <lds|global|none>; items <a> wave + <b> small + <c> large
 *                              + <d> global + <e> skipped; batches <n> cliques <C>`, a + b + c + d + e = V (no line when the
 *                              call is answered without a plan);
 *   GMX_KCLIQUE_PHASES         the device time of the plan additions, the matrices (every class launched once more, stopping
 *                              behind its matrix), each class's count kernel less that share, and the finish, on stderr
 *                              (tools/kclique_prof.py).  The extra launches lie inside the timed span: kernel_ms of such a
 *                              call includes them, so take kernel_ms from calls without this knob. */
int gmx_kclique(gmx_graph_t* g, int32_t k, int64_t* count_host, int64_t* cliques, gmx_stats_t* stats);

/* 4-cycle (square) counting, in total and through every vertex (the reference has no such program).  The stored slots are
 * read exactly as gmx_clustering, gmx_ktruss and gmx_kclique read them, N(v) = { u != v : v -> u or u -> v is stored }: self
 * loops and repeated slots change nothing, rows may be in any order, and only the forward CSR is read (a
 * GMX_GRAPH_NO_REVERSE graph works; there is no GMX_ERR_STATE).
 * A square is a set of four distinct vertices {a, b, c, d} with the edges ab, bc, cd, da present, counted once per such cycle;
 * chords are allowed: K4 holds three squares, on one vertex set.  On a bipartite graph these are its butterflies.
 * *squares = the number of squares.  count_host[V] (int64, by the caller's vertex id) = the number of squares through v, so
 * that sum(count) == 4 * *squares.  count_host may be NULL and is then neither built nor downloaded: the cheap total-only
 * query, which walks the wedges once and scatters no credit.  Results are exact while 2 * count[v] < 2^63 for every v (the
 * end-vertex credits are accumulated doubled); beyond that they are unspecified.  stats may be NULL.
 * squares == NULL or g == NULL (checked in this order, before g is touched): GMX_ERR_ARG before any device call.  V = 0: GMX_OK,
 * nothing is written but *squares = 0.  E = 0 or self loops only: GMX_OK, zeros, answered without a plan.  When the plan's
 * additions, the per-vertex scratch or the global class's counters cannot be allocated: GMX_ERR_NOMEM, and the message gives
 * the byte count.  A graph with 2^30 undirected edges or more is GMX_ERR_ARG (the symmetric adjacency has 32-bit offsets).
 * Integers only: both results are unique and byte-identical from run to run and under every knob.
 * Method:
 *   plan     the one gmx_triangle_counting_directed, gmx_clustering, gmx_ktruss and gmx_kclique share, cached on the graph, with
 *            the symmetric adjacency gmx_ktruss adds to it (row v = DOWN'(v) then UP'(v), sorted; whichever of the two entries
 *            is called first builds it).  GMX_SQUARES_NO_ORDER and the other entries' NO_ORDER knobs each rebuild a cached plan
 *            of the other order.  The first gmx_squares call adds, and frees with the plan: per slot (u, v) of DOWN' the prefix
 *            length |{ w in N'(v) : w < u }| (one binary search; kept as running sums inside u's row), W(u) = their sum over
 *            u's row = the wedges of u, D(u) = |DOWN'(u)| (read off the adjacency), and the vertices listed by ascending W
 *            (one device sort, the vertices with D(u) < 2 in front), whose keys the host keeps to find the class offsets.
 *   count    in plan ids every square has one highest vertex u; its opposite vertex w and both middle vertices are below u.
 *            c_u(w) = |{ v in DOWN'(u) : w in N'(v) }| for w < u: the squares with top u and opposite w number C(c_u(w), 2).
 *            Pass 1 walks the wedges u - v - w and adds 1 to the entry of w in a table keyed by w.  Without count_host the add
 *            returns the count before: the c adds to one entry return 0, 1, ..., c - 1 in some order, which sum to C(c, 2),
 *            and there is no second pass.
 *   credits  pass 2 walks the same wedges with x = c_u(w) - 1: v takes x (summed over the slot's wedges first: one 64-bit
 *            atomic per DOWN' slot), w and u take x into a doubled accumulator (u's share by one wave reduction), which is
 *            halved at the end: the c wedges to w give (c - 1) each, 2 C(c, 2) together.  count = mid + end2 / 2, held in plan
 *            ids and permuted back on the device before the download.  No result depends on the order of the adds.
 *   classes  one launch each over a range of the list.  The routing rule is part of the contract:
 *              skipped  D(u) < 2: never launched;
 *              wave     live, WAVE_MAX > 0 and W(u) <= WAVE_MAX: a wave per vertex, an open-addressing table (key w, count) of
 *                       at least 2 W(u) slots in the wave's LDS slice, LDS atomics;
 *              block    live, not wave, W(u) <= LDS_SLOTS / 2: the same with a workgroup per vertex, the table in dynamic LDS;
 *              global   the rest: u int32 counters per vertex in workspace memory, dealt in batches of at most BATCH_BYTES: the
 *                       list is cut greedily, a batch's vertices each get as many counters (a multiple of 64) as its highest
 *                       plan id needs, and a vertex that alone exceeds the budget is a batch by itself.  Per batch a counting,
 *                       a crediting (not without count_host) and a zeroing step; zeroing walks the wedges again and stores 0.
 *                       The vertices with W(u) > SPLIT, a suffix of the batch, run in a launch of their own in every step: u is
 *                       cut into min(ceil(W / SPLIT), D, 1024) ranges of DOWN'(u) of about equal wedges, a workgroup each.
 * Every loop ends by construction and no kernel waits for a value that another workgroup writes.
 * stats: iterations = 1, edges_examined = the wedges walked = the sum of W(u) over the vertices with D(u) >= 2,
 * vertices_reached = the vertices with count > 0 (0 when count_host == NULL), kernel_ms = device time from the first launch
 * after the plan and its additions to the last, d2h_ms = the downloads, h2d_ms = 0.
 * Read at every call, no result byte depends on them:
 *   GMX_SQUARES_NO_ORDER=1     the plan keeps the graph's numbering;
 *   GMX_SQUARES_WAVE_MAX       default 128, clamped to [0, 128]; 0: no wave class;
 *   GMX_SQUARES_LDS_SLOTS      table slots (8 bytes each) of a block-class workgroup, default 4096, clamped to [64, 18432];
 *   GMX_SQUARES_BATCH_BYTES    counters of one global-class batch, default 1 GiB;
 *   GMX_SQUARES_SPLIT          default 4096, at least 1;
 *   GMX_SQUARES_PLAIN=1        every credit, u's included, as one global atomic per wedge (the form the others are measured
 *                              against);
 *   GMX_SQUARES_LOG=1          one line on stderr: `gmx squares: plan V <V> E <E> up <|UP'|> order <degree|identity> built <0|1>
 *                              adj_built <0|1> classes_built <0|1>; wave_max <n> lds_slots <n> split <n> batch_bytes <n> counts
 *                              <lds|global|none>; items <a> wave + <b> block + <c> global (<s> split) + <e> skipped; wedges <n>
 *                              batches <n> squares <n>`, the thresholds as in force, a + b + c + e = V (no line when the call is
 *                              answered without a plan);
 *   GMX_SQUARES_PHASES         the device time of the additions (the adjacency included when this call builds it), each class
 *                              and the finish, on stderr (tools/squares_prof.py).  It synchronises between the classes: take
 *                              kernel_ms from calls without this knob. */
int gmx_squares(gmx_graph_t* g, int64_t* count_host, int64_t* squares, gmx_stats_t* stats);

/* 4-node graphlet census and graphlet degree vectors (the reference has no such program): every connected subgraph on 2, 3
 * and 4 vertices, in total and per vertex by orbit.  The stored slots are read exactly as gmx_clustering, gmx_ktruss, gmx_kclique
 * and gmx_squares read them, N(v) = { u != v : v -> u or u -> v is stored }: self loops and repeated slots change nothing, rows
 * may be in any order, and only the forward CSR is read (a GMX_GRAPH_NO_REVERSE graph works; there is no GMX_ERR_STATE).
 * Graphlets and orbits, numbered as in ORCA:
 *   G0 edge: 0 (the degree).   G1 path on 3: 1 end, 2 middle.   G2 triangle: 3.   G3 path on 4: 4 end, 5 inner.
 *   G4 claw: 6 leaf, 7 centre.   G5 4-cycle: 8.   G6 paw (a triangle with a tail): 9 the tail's end, 10 the two triangle corners
 *   away from the tail, 11 the corner that carries the tail.   G7 diamond (K4 minus an edge): 12 the two corners of degree 2, 13
 *   the two of degree 3.   G8 K4: 14.
 * induced = 1: gdv_host[v * 15 + k] (int64, row-major by the caller's vertex id) = the INDUCED subgraphs in which v sits at
 * orbit k, and totals[0 .. 8] = the induced subgraphs of G0 .. G8.  induced = 0: the subgraph (non-induced) counts n_k, the
 * convention of gmx_squares: gdv[v][8] is gmx_squares' count[v] and gdv[v][14] gmx_kclique's at k = 4, and totals counts
 * subgraphs.  In either convention gdv[v][0] and gdv[v][3] are gmx_clustering's deg[v] and tri[v].  gdv_host may be NULL and is
 * then neither built nor downloaded: the cheap totals-only query, which runs no per-vertex kernel (one pass over the edges, and
 * the total-only modes of gmx_squares and gmx_kclique).  stats may be NULL.
 * Arithmetic is in unsigned 64-bit words.  The induced counts are an integer-linear function of the n_k, so a wrap-around in an
 * n_k is harmless: every returned number is exact whenever it fits an int64 itself (and gdv[v][8] while 2 * n8 < 2^64, as for
 * gmx_squares).  C(x, 2) and C(d, 3) divide before they multiply (the even factor by two, the multiple of three by three), so
 * that they do not wrap where the binomial fits: a star of 3.4 million leaves has d (d - 1) (d - 2) > 2^64 and C(d, 3) < 2^63.
 * totals == NULL, induced outside {0, 1} or g == NULL (checked in this order, before g is touched): GMX_ERR_ARG before any device
 * call.  V = 0: GMX_OK, nothing is written but totals = 0.  E = 0 or self loops only: GMX_OK, zeros, answered without a plan.
 * When the scratch cannot be allocated: GMX_ERR_NOMEM, and the message gives the byte count.  Before it returns the entry
 * verifies the sum identities of the orbits (sum o4 = sum o5, sum o6 = 3 sum o7, sum o9 = sum o11 = sum o10 / 2, sum o12 = sum
 * o13, and the agreement with the triangles walked, the squares and the 4-cliques): a broken one is GMX_ERR_HIP with a text.
 * Integers only: every result is unique and byte-identical from run to run and under every knob.
 * Method: on the plan the counting family shares and its symmetric adjacency, in plan ids.  t(e), the
 * triangles on every edge, from gmx_ktruss' support kernel; d from the rows, T(v) as half the sum of t(e) over v's row; two
 * passes of row sums (sum (d_u - 1), sum C(d_u - 1, 2), sum t, sum t (d_u - 2), sum C(t, 2); then sum S(u) and sum T(u)); one
 * weighted walk of the triangles that credits every corner with the support of the opposite edge minus one (orbit 12); the
 * per-vertex words of gmx_squares and gmx_kclique at their default thresholds, kept on the device; a finishing kernel that
 * forms the fifteen counts, applies the transform, sends the rows back through perm and sums the columns.
 * stats: iterations = 1, edges_examined = the triangles walked (0 when gdv_host == NULL: there is no walk), vertices_reached =
 * the vertices with a non-zero entry among the orbits 4 .. 14 of the rows returned (0 when gdv_host == NULL), kernel_ms = device
 * time from the support kernel to the finish (the first call on a plan includes the additions of gmx_squares and gmx_kclique),
 * d2h_ms = the downloads, h2d_ms = 0.
 * Read at every call, no result byte depends on them:
 *   GMX_GRAPHLETS_NO_ORDER=1   the plan keeps the graph's numbering;
 *   GMX_GRAPHLETS_PLAIN=1      the walk as one work item per edge with one 64-bit global atomic per match (the form the default
 *                              is measured against); the squares and the 4-cliques keep their default credits;
 *   GMX_GRAPHLETS_CAP          list entries (and 32-bit counters) a wave stages in LDS, default 512, clamped to [64, 1024]; a
 *                              longer list is searched in memory and credits by global atomics;
 *   GMX_GRAPHLETS_LONG         default 2048, at least 1: a row of more slots is cut into 64-slot groups in the row passes;
 *   GMX_GRAPHLETS_LOG=1        one line on stderr: `gmx graphlets: plan V <V> E <E> up <|UP'|> order <degree|identity> built <0|1>
 *                              adj_built <0|1> groups_built <0|1> squares_built <0|1> kclique_built <0|1>; cap <n> long <n> counts
 *                              <lds|global|none> induced <0|1>; items <a> staged + <b> memory; long_rows <n>; triangles <n>;
 *                              totals <G0> ... <G8>` (no line when the call is answered without a plan);
 *   GMX_GRAPHLETS_PHASES       the device time of the plan additions, the support kernel, the passes, the walk, the squares, the
 *                              4-cliques and the finish, on stderr (tools/graphlets_prof.py).  It synchronises between them:
 *                              take kernel_ms from calls without this knob. */
int gmx_graphlets(gmx_graph_t* g, int induced, int64_t* gdv_host, int64_t* totals, gmx_stats_t* stats);

/* Louvain modularity communities (the reference has no such program).  The graph is read as gmx_msf reads it: every stored
 * forward slot u -> w of weight x is an undirected edge; weight_host[E] is int32 by UPLOADED forward slot, NULL = every weight
 * is 1; only the forward CSR is read, rows in any order, and a repeated slot is another edge (its weights add).  The symmetric
 * integer matrix A: a slot with u != w adds x to A[u][w] and to A[w][u], a self-loop slot adds 2x to A[u][u].  k[u] = the sum
 * of row u of A, m2 = the sum of all k = 2 sum x.  A weight below 1 is GMX_ERR_ARG, found by a device pass before any other
 * work.  Weights go up to 2^31 - 1 and E stays below the int32 limit, so m2 < 2^63; every product below is formed in signed
 * 128-bit integers.  The form is closed under contraction (A'[C][D] = the sum of A[u][w] over u in C, w in D): level 0 is the
 * contraction of the doubled slot list under the identity map, and every level runs the same code.
 * One level, on n level vertices with comm[i] = i and tot[c] = k[c]: q = Qnum = m2 intra - sum_c tot[c]^2, intra = the sum of
 * A[u][w] over the pairs with comm[u] == comm[w].  Round r = 0, 1, ... of the level is two half-rounds; vertex i belongs to
 * half fmix32(uint32(i) ^ (uint32(r) * 0x9E3779B9u)) & 1 (gmx_communities' hash), half 0 first.  A half-round evaluates every
 * vertex of its half against ONE snapshot of comm and tot: with c = comm[i], e[D] = the sum of A[i][w] over w != i with
 * comm[w] == D (e[c] exists even when it is 0) and score(D) = m2 e[D] - k[i] (tot[D] - (D == c ? k[i] : 0)), i keeps c when
 * score(c) is the maximum over the keys of e, otherwise it takes the SMALLEST D with the maximum score.  All moves of the
 * half-round are applied together (comm[i] = D, tot[c] -= k[i], tot[D] += k[i]) and Qnum is evaluated exactly: if something
 * moved and the new Qnum is not strictly greater than q, the half-round is rolled back (comm, tot and q as before); otherwise
 * q takes the new value.  A round that keeps no move ends the level, and so do max_rounds rounds, kept or not.  The level's
 * non-empty labels are renumbered in ascending label order and the next level is the contraction.  A level that kept no move
 * ends the run, and so does reaching max_levels levels.
 * comm_host[V] = for each original vertex the community it lies in after the last level that kept a move, numbered as gmx_wcc
 * numbers components (by ascending smallest member); *num_comms; *num_levels = the levels that kept a move; *intra = the final
 * intra; *modularity = (double) Qnum / ((double) m2 * (double) m2): one correctly rounded conversion of the 128-bit numerator,
 * one multiply, one divide, on the host; 0.0 when m2 == 0.  max_levels == 0 gives the identity and the singletons' modularity.
 * GMX_ERR_ARG before g is touched otherwise: g == NULL, comm_host == NULL with V > 0, max_levels < 0, max_rounds < 1.  V = 0 or
 * E = 0: GMX_OK, identity labels.  Every other out-pointer and stats may be NULL.  Nothing is cached on the graph.
 * Integers only: the partition and the modularity are byte-identical to a one-thread run of this schedule, from run to run,
 * under every knob and upload form.
 * Method: per half-round the rows of the half are evaluated in three row-length regimes (short: 16 lanes per
 * row, labels and weights in registers; wave: an open-addressing table label -> 64-bit sum in the wave's LDS slice; block: the
 * same table in the workgroup's LDS; rows whose table fills: passes over disjoint label classes, any row length and label
 * count), every table entry is scored with tot[D] gathered from the snapshot and the 128-bit (score, smaller label) maximum is
 * reduced; moves go to a pending list (i, old, new); commit applies them with 64-bit atomics on tot; one sweep of the entries
 * gives intra and a 128-bit reduction sum tot^2; a one-wave judge keeps or sets the roll-back flag, which the undo kernel
 * obeys; the host reads one record per round.  Contraction: keys (comm[u] << 32 | comm[w]), a device sort, a reduce-by-key of
 * the weights, row offsets and k; the level maps are composed on the device and gmx_wcc's scan gives the final numbering.
 * Every loop ends by construction and no kernel waits for a value that another workgroup writes.
 * stats: iterations = the rounds that kept a move, over all levels; vertices_reached = *num_comms; edges_examined = the sum
 * over the levels of (rounds run, the last empty or rolled-back one included) x (entries of the level's merged adjacency,
 * diagonal included); h2d_ms = the weights, kernel_ms = first launch to last, d2h_ms = the downloads.
 * Read at every call, no result byte and no stat depends on them:
 *   GMX_LOUVAIN_WAVE_MIN     rows of fewer entries are short; default 33, clamped to [1, 33] (a short row lies in registers);
 *   GMX_LOUVAIN_BLOCK_MIN    rows of this many entries or more get a workgroup; default 256, at least 1;
 *   GMX_LOUVAIN_LDS_SLOTS    the workgroup's table, default 4096, the power of two at or below the value clamped to
 *                            [512, 8192]; a wave's table has an eighth of it;
 *   GMX_LOUVAIN_LOG=1        one line on stderr: `gmx louvain: V <V> E <E> weighted <0|1> levels <l> rounds <rounds run> rollbacks
 *                            <n> cuts <levels ended by max_rounds> moves <moves kept> sizes <n/nnz of every level run, or -> comms
 *                            <c> intra <i> overflowed <rows sent to the class passes>` (no line for V = 0 or E = 0);
 *   GMX_LOUVAIN_PHASES       per level the contraction's device time, per round the time of its evaluate and of its
 *                            commit-measure-judge-undo launches, on stderr (tools/louvain_prof.py).  It synchronises. */
int gmx_louvain(gmx_graph_t* g, const int32_t* weight_host, int32_t max_levels, int32_t max_rounds, gmx_node_t* comm_host, int32_t* num_comms,
                int32_t* num_levels, double* modularity, int64_t* intra, gmx_stats_t* stats);

/* The common-neighbour iterator, gm_common_neighbor_iter(G, s, d) (gm_common_neighbor_iter.cc:21-44): the slots of s's
 * row, in order and with their multiplicity, whose value occurs in d's row (Foreach(u: s.CommonNbrs(d)) <=>
 * Foreach(u: s.Nbrs)(d.isNbr(u)), gm_common_neighbor_iter.h:11-17).  gmx_common_nbrs lists them for one pair (*n = how
 * many there are; at most cap are written), gmx_common_nbr_counts counts them for many pairs, and
 * gmx_triangle_counting_cn is triangle counting written with the iterator
 *   Foreach(v: G.Nodes) Foreach(u: v.Nbrs)(u > v) Foreach(w: v.CommonNbrs(u))(w > u) T += 1;
 * (equal to gmx_triangle_counting on a symmetric graph; on a directed one it asks for u -> w where the emitted
 * triangle_counting.gm asks for w -> u). */
int gmx_common_nbrs(gmx_graph_t* g, gmx_node_t s, gmx_node_t d, gmx_node_t* out, int64_t cap, int64_t* n);
int gmx_common_nbr_counts(gmx_graph_t* g, const gmx_node_t* src, const gmx_node_t* dst, int64_t npairs, int64_t* counts);
int gmx_triangle_counting_cn(gmx_graph_t* g, int64_t* count, gmx_stats_t* stats);

/* adamicAdar(G, aa) (apps/src/adamicAdar.gm; driver apps/output_cpp/src/adamicAdar_main.cc:25), the application that
 * computes with the iterator: for every forward edge slot e = (from -> to)
 *     aa[e] = sum over the items n of gm_common_neighbor_iter(G, from, to) -- the slots of row(from), in slot order and
 *             with their multiplicity, whose value occurs in row(to) -- of 1.0 / log((double) outdeg(n)),
 * outdeg(n) = begin[n+1] - begin[n], in IEEE double without fast-math.  What the formula gives is what is returned: a
 * common neighbour of out-degree 1 contributes +inf (the edge's value is +inf), one of out-degree 0 contributes -0.0, an
 * edge without common neighbours gets exactly +0.0, and no value is NaN.  The order of the additions inside one edge's
 * sum is the device's, not the slot order (a distinct value that row(from) repeats m times enters as m * its term), but
 * it is fixed: the result is bit-identical from run to run, and within (k + 2) * 2^-52 relative of the slot-order sum
 * for an edge with k items.  Repeated slots (from, to) of a multigraph get the same value.
 * aa_host[E] is indexed like gmx_sssp's len: by the UPLOADED slots (through e_idx2idx when the upload sorted the rows).
 * Only the forward CSR is read (a GMX_GRAPH_NO_REVERSE graph works); forward rows uploaded verbatim and out of order give
 * GMX_ERR_STATE, as for the iterator.  E = 0: GMX_OK, nothing written.  stats: iterations = 1, kernel_ms = device time
 * (weights, work list and the intersections), d2h_ms = download of aa, edges_examined = items over all slots (exact). */
int gmx_adamic_adar(gmx_graph_t* g, double* aa_host /* [E] */, gmx_stats_t* stats);

/* v_cover(G, select) (apps/src/v_cover.gm; driver apps/output_cpp/src/v_cover_main.cc:24): the greedy vertex cover
 *     Deg = Degree() + InDegree();  Covered = select = False;  remain = 2 E;
 *     While (remain > 0) { the edge s -> t with !(Covered[s] && Covered[t]) of maximal Deg[s] + Deg[t] is selected;
 *                          remain -= that maximum;  Deg[s] = Deg[t] = 0;  Covered[s] = Covered[t] = True; }
 *     Return Count(Covered);
 * The reference's parallel arg-max breaks ties by thread timing (its driver prints "may be non-deterministic").  The
 * device is deterministic and equal to the reference run with ONE thread: among the edges of maximal Deg[s] + Deg[t] the
 * lowest forward slot wins.  Everything else is literal: duplicate edges are separate slots, and a selected self loop
 * takes 2 Deg[s] from `remain` but only Deg[s] from the degree sum, so the loop can stop with uncovered vertices left.
 * `remain` is kept in 64 bits here; the reference's Int overflows from E = 2^30 upward, and this entry takes E < 2^30
 * (GMX_ERR_ARG otherwise: the incident lists keep 32-bit offsets).
 * select_host[E] (0 / 1) is indexed, and ties are decided, by the UPLOADED slots like gmx_sssp's len (through e_idx2idx
 * when the upload sorted the rows): the result is the same for every upload form, and rows are read in any order.
 * *covered = the number of covered vertices.  Needs the reverse CSR (GMX_ERR_STATE after an upload with
 * GMX_GRAPH_NO_REVERSE).  g == NULL, covered == NULL, or select_host == NULL with E > 0: GMX_ERR_ARG.  V = 0 or E = 0:
 * GMX_OK, *covered = 0, select_host untouched.
 * The arg-max per selected edge is replaced by rounds that pick every locally dominant edge at once, O(E) work in total
 * (gmx_vcover.hip); the first call builds a plan (per vertex its incident edges sorted by the other
 * end's degree), cached on the graph and freed with it.  Read at every call, the result does not depend on them:
 *   GMX_VC_TAIL  a round with at most this many active vertices hands the rest to one workgroup (0: never; huge: all),
 *   GMX_VC_WAVE  a list with at least this many entries left is advanced by a wave (0: always; huge: always a lane),
 *   GMX_VC_LOG=1 one stderr line per call: plan built / reused, V, E, list entries, rounds, picks, kept, counters, ms.
 * stats: iterations = parallel rounds, kernel_ms = device time without the plan build, edges_examined = list entries
 * skipped + vertex evaluations + list entries walked, vertices_reached = covered, edges_reached = selected edges,
 * d2h_ms = download of select. */
int gmx_v_cover(gmx_graph_t* g, uint8_t* select_host /* [E], uploaded slots, 0/1 */, int32_t* covered, gmx_stats_t* stats);

/* random_bipartite_matching(G, isLeft, Match) (apps/src/random_bipartite_matching.gm; the reference ships no driver): a
 * maximal matching of a bipartite graph whose edges lead from left to right vertices, by rounds of
 *     1. proposals: every unmatched left n sets Suitor[t] = n at every unmatched neighbour t (an intended write-write race);
 *     2. replies:   every unmatched right t with a suitor n sets Suitor[n] = t and clears its own;
 *     3. commit:    every left n with a reply t: Match[n] = t, Match[t] = n, count++;
 * until a round makes no proposal.  The race makes a parallel reference run depend on thread timing.  The device is
 * deterministic and equal to the reference run with ONE thread: Foreach visits vertices in ascending id and a row in slot
 * order, so the last writer wins -- Suitor[t] is the LARGEST unmatched left n with an edge n -> t, and a left keeps the
 * LARGEST right that replied to it.  *count = the matched pairs (the program's return value); match_host[v] = the partner
 * of v, -1 (gm_graph::NIL_NODE) for every vertex left unmatched.  Suitor is internal.
 * Only rows of vertices with is_left != 0 are read: edges out of right vertices, right self loops included, are ignored as
 * the literal loop ignores them; duplicate slots are harmless.  An edge from a left to a left vertex breaks the program's
 * precondition ("every edge is from left node to right node"): GMX_ERR_ARG, gmx_last_error() names one such edge, and
 * match_host is untouched (found on the device by the first proposal pass, not by a sweep of its own).
 * Only the forward CSR is read (a GMX_GRAPH_NO_REVERSE graph works), rows in any order, repeats included; the result is
 * indexed by vertex and so the same for every upload form.  g == NULL, count == NULL, or is_left_host / match_host ==
 * NULL with V > 0: GMX_ERR_ARG.  V = 0: GMX_OK, *count = 0.  E = 0: GMX_OK, all -1.  Nothing is cached on the graph.
 * A round is three launches over lists (the rows of the live lefts, the rights that got a proposal, the live lefts);
 * a left is live while it is unmatched and proposed in the round before (gmx_match.hip).  Read at every
 * call, the result does not depend on them:
 *   GMX_RBM_TAIL   once the live rows hold at most this many slots one workgroup runs the rest (0: never; huge: all),
 *   GMX_RBM_LOG=1  one stderr line per call: V, E, lefts, the threshold, rounds grid + tail, matched, proposals, slots, ms
 *                  (2: before it a line per grid round: live lefts, slots, proposals, touched rights, host-clock ms).
 * stats: iterations = rounds that made a proposal, vertices_reached = *count, edges_reached = proposals summed over the
 * rounds (a proposal is a slot (n, t) of a live left with t unmatched at the round's start: schedule-independent),
 * edges_examined = slots read, h2d_ms = upload of is_left, d2h_ms = download of match, kernel_ms = device time from the
 * first to the last launch. */
int gmx_random_bipartite_matching(gmx_graph_t* g, const uint8_t* is_left_host /* [V], 0/1 */,
                                  gmx_node_t* match_host /* [V], partner or -1 */, int32_t* count, gmx_stats_t* stats);

/* ---- the sampling programs (apps/src/parallel_random_walk_jump_sampling.gm, random_node_sampling.gm,
 * random_degree_node_sampling.gm; gmx_walk.hip) ----
 * The stream.  Every entry below takes uint64_t* rng_state in and out: a 48-bit state x.  A draw is
 *     x = (0x5DEECE66D * x + 0xB) mod 2^48,   u = x / 2^48 as a double
 * which is exactly what erand48 returns.  Uniform() is one draw, PickRandom() is (node_t)(u * (double) V) and
 * n.PickRandomNbr() is node_idx[begin[n] + (edge_t)(u * (double) deg(n))] on the rows as stored on the device (what
 * gmx_graph_download returns).  On return *rng_state is the state after the last draw the program run by ONE thread
 * consumed, so consecutive calls continue one stream.  The host shim's gm_rt_uniform(0) is the same stream; its state
 * after gm_rt_set_num_threads(1) is 0x0AA849495101.
 * Not reproduced from the reference: its pick_random_node() draws from libc rand(), which is not a portable stream, and
 * its pick_random_out_neighbor() returns node_idx[begin[node]] + rand() % outCount, which adds the offset to a vertex id
 * (gm_graph.h:379-391).
 *
 * gmx_random_walk_sampling: parallel_random_walk_jump_sampling(G, p_size, p_jump, num_tokens; Selected), as one thread runs it:
 *     Token = TokenNxt = 0; Selected = False
 *     S = {}; do { S.add(PickRandom()) } while (|S| < num_tokens);  Token[n] = 1 for n in S
 *     N = (int64)((float) V * p_size)                  -- a float multiply, as the emitted C++ does
 *     count = 0
 *     while (count < N && rounds < max_rounds):
 *       for n = 0 .. V-1 with Token[n] > 0:
 *         if (!Selected[n]) { Selected[n] = True; count++ }
 *         Token[n] times:  jump = (deg(n) == 0) || (Uniform() < (double) p_jump)      -- no draw when deg(n) == 0
 *                          m = jump ? PickRandom() : n.PickRandomNbr();  TokenNxt[m]++
 *       Token = TokenNxt; TokenNxt = 0; rounds++
 * selected_host, token_host (the final Token; may be NULL), *count, *rounds and *rng_state are byte-identical to that loop,
 * whatever the knobs below say.  max_rounds is ours: with p_jump = 0 on a closed component the reference never returns
 * (the drop-in passes INT32_MAX).  N <= 0: the tokens are placed, no round runs, Selected is all false.
 * GMX_ERR_ARG, with nothing written: num_tokens < 1 or > V (the reference loops for ever above V), p_size or p_jump not a
 * number, N > V, max_rounds < 0, V = 0, or g, rng_state, selected_host, count or rounds NULL.
 * Only the forward CSR is read, rows in any order, repeats and self loops included.  Read at every call, the results do
 * not depend on them:
 *   GMX_RW_TAIL   with at most this many tokens one workgroup runs the rounds, up to 1024 per launch (0: never; huge: always),
 *   GMX_RW_ORDER  sort | dense | auto: how a grid round brings the vertices it touched into ascending order,
 *   GMX_RW_LOG=1  one stderr line per call: V, tokens, the threshold, batches of the initial set, rounds grid + tail, tail
 *                 launches, sort rounds, dense rounds (the ordering of the initial set counts, the last round needs none), draws,
 *                 count, ms (2: before it a line per grid round / tail launch).
 * stats: iterations = *rounds, vertices_reached = *count, edges_examined = tokens moved over all rounds, kernel_ms = device
 * time from the first to the last launch, d2h_ms = the downloads. */
int gmx_random_walk_sampling(gmx_graph_t* g, float p_size, float p_jump, int32_t num_tokens, int32_t max_rounds,
                             uint64_t* rng_state, uint8_t* selected_host /* [V] */, int32_t* token_host /* [V] or NULL */,
                             int64_t* count, int32_t* rounds, gmx_stats_t* stats);

/* random_node_sampling(G, N; S) (by_degree = 0) and random_degree_node_sampling(G, N; S) (by_degree = 1): vertex v takes
 * draw v + 1 of the stream as dice and is selected when
 *     dice < 1 / (double) N                                             (by_degree = 0)
 *     dice < ((double) deg(v) / (double) degSum) * (double) N           (by_degree = 1; degSum = E as int64)
 * evaluated literally in IEEE double: E = 0 gives NaN and so the empty set, N = 0 without degrees gives every vertex.
 * The state advances by V.  selected_host[v] = 0/1, *count = the vertices selected.  One kernel; forward CSR only.
 * g, rng_state or count NULL, or selected_host NULL with V > 0: GMX_ERR_ARG.  V = 0: GMX_OK, *count = 0, state unchanged.
 * stats: iterations = 1, vertices_reached = *count, edges_examined = V, kernel_ms, d2h_ms. */
int gmx_node_sampling(gmx_graph_t* g, int by_degree, int32_t N, uint64_t* rng_state, uint8_t* selected_host /* [V] */,
                      int64_t* count, gmx_stats_t* stats);

/* ---- device-resident PageRank stepping (bench.py / multi-GPU driver) ----
 * A gmx_pr_t owns the rows [row_lo,row_hi) of the (internally relabelled) graph
 * and a full replica of the contribution vector.  One step = one PageRank
 * iteration over the owned rows.  With nranks > 1 the caller exchanges the
 * owned slice of the new contribution vector between steps (all-gather over
 * RCCL); slices are equal sized and contiguous by construction. */
#define GMX_PR_F32 4
#define GMX_PR_F64 8
/* options bit flags */
#define GMX_PR_RELABEL   0x1u   /* degree-sorted internal numbering (default on in whole-kernel entries) */
#define GMX_PR_HOT_LDS   0x2u   /* keep the hottest contributions in LDS */
#define GMX_PR_SLICED    0x4u   /* split in-edges by source slice, one slice per XCD L2 (needs GMX_PR_RELABEL) */
#define GMX_PR_COLD_PB   0x8u   /* with GMX_PR_SLICED: edges from the cold sources (the tail of the degree order, past what the
                                   L2s hold; GMX_PR_COLD=<hot ids per rank range> overrides the size rule) leave the pull
                                   sweep and go through plan-time-ordered destination bins: no 128-byte line per gather */
/* The option set the whole-kernel entries use for a graph of V vertices on nranks ranks. */
uint32_t gmx_pr_default_options(int64_t V, int nranks);
int gmx_pr_create(gmx_graph_t* g, int elem_bytes, int rank, int nranks, uint32_t options, gmx_pr_t** out);
int gmx_pr_free(gmx_pr_t* p);
int gmx_pr_reset(gmx_pr_t* p, double d);                 /* rank = 1/N, contrib = rank/outdeg, cnt = 0 */
/* Enqueue one iteration on `stream` (a hipStream_t, NULL = default stream). Asynchronous. */
int gmx_pr_step(gmx_pr_t* p, void* stream);
/* Row chunks: with C > 1 a step is enqueued as C pieces (gmx_pr_step_chunk 0..C-1, in that order), each
 * finishing the new contributions of one sub-range [offset, offset+count) of the rank's exchanged prefix
 * (gmx_pr_chunk_range; identical on every rank, together they tile [0, gmx_pr_exchange_count)), so that
 * the exchange of chunk c runs while chunk c+1 is computed.  The sub-ranges are walked from the back: the
 * first pieces hold most of the rows but few edges, the last one the hubs.  gmx_pr_step() enqueues all
 * chunks.  Only the sliced variant splits; otherwise the chunk count stays 1.
 * gmx_pr_contrib_next_full is the replica the running step writes. */
int gmx_pr_set_chunks(gmx_pr_t* p, int chunks);
int gmx_pr_num_chunks(gmx_pr_t* p, int* chunks);
int gmx_pr_chunk_range(gmx_pr_t* p, int chunk, int64_t* offset, int64_t* count);
int gmx_pr_step_chunk(gmx_pr_t* p, int chunk, void* stream);
int gmx_pr_contrib_next_full(gmx_pr_t* p, void** dev_ptr, int64_t* count);
/* Peer push: the exchange of the N > 1 step without a collective kernel.  The host side passes the ranks'
 * replica handles around (gmx_pr_contrib_buffers -> gmx_ipc_export -> its own transport -> gmx_ipc_open) and
 * hands the mapped pointers to gmx_pr_set_peers (arrays of nranks entries, own entry ignored).  After
 * gmx_pr_step_chunk(c, stream), gmx_pr_push_chunk(c, stream) copies the chunk's piece into every peer's
 * replica on per-peer copy streams (SDMA over xGMI), ordered after the chunk's kernels;
 * gmx_pr_push_current pushes the whole exchanged prefix of the current replica (after a reset);
 * gmx_pr_push_join makes `stream` wait for all copies issued so far.  The caller then runs its per-step
 * barrier (e.g. the all-reduce of diff): a rank may start the next step only after every rank's copies
 * have completed. */
#define GMX_IPC_HANDLE_BYTES 64
int gmx_ipc_export(void* dev_ptr, void* handle /* GMX_IPC_HANDLE_BYTES */);
int gmx_ipc_open(const void* handle, void** dev_ptr);
int gmx_ipc_close(void* dev_ptr);
int gmx_pr_contrib_buffers(gmx_pr_t* p, void** buf0, void** buf1, int64_t* bytes);
int gmx_pr_set_peers(gmx_pr_t* p, void* const* peer_buf0, void* const* peer_buf1);
int gmx_pr_push_chunk(gmx_pr_t* p, int chunk, void* stream);
int gmx_pr_push_current(gmx_pr_t* p, void* stream);
int gmx_pr_push_join(gmx_pr_t* p, void* stream);
/* Packed form of the push ("send only what is read").  Rank q reads source w iff w has an out-edge into a row q owns;
 * on an 8-rank partition of RMAT-26 that is 46 % of the (source, reader) incidences of the full prefixes.  The plan of a
 * rank (nranks > 1, degree order) holds, per peer, the sorted positions of ITS range that the peer reads and the
 * positions of the peer's range that IT reads -- the same list on both sides by construction (gmx_pr_packed_info
 * returns GMX_ERR_STATE when the plan has none).  gmx_pr_push_packed(c) gathers the chunk's entries of those lists into a
 * staging buffer and copies each peer's piece into the peer's landing zone (double buffered by replica parity; wired
 * up like the replicas: gmx_pr_recv_buffers -> gmx_ipc_export -> transport -> gmx_ipc_open -> gmx_pr_set_peers_packed
 * with the offset of the caller's segment in each peer's zone = the peer's recv_offsets[caller]); chunk -1 pushes the
 * current replica's whole prefix (after a reset).  After the per-step barrier gmx_pr_unpack(c) scatters what has landed
 * into the replica the next step reads (c = -1: all chunks).  Positions nobody reads are never touched: afterwards the
 * replicas agree with an all-gather only on the positions gmx_pr_recv_list names. */
int gmx_pr_packed_info(gmx_pr_t* p, int64_t* send_counts, int64_t* recv_counts, int64_t* recv_offsets);   /* [nranks] each, elements */
int gmx_pr_recv_buffers(gmx_pr_t* p, void** buf0, void** buf1, int64_t* bytes);
int gmx_pr_set_peers_packed(gmx_pr_t* p, void* const* peer_recv0, void* const* peer_recv1, const int64_t* my_offset, const int64_t* my_count);
int gmx_pr_push_packed(gmx_pr_t* p, int chunk, void* stream);
int gmx_pr_unpack(gmx_pr_t* p, int chunk, void* stream);
int gmx_pr_recv_list(gmx_pr_t* p, int r, void** dev_ptr, int64_t* count);
/* Pipelined form of the pushed step (plans with every in-edge binned: gmx_pr_gather_classes returns 2, else 0).
 * Phase 1 of the binned sweep is the only part of a step that reads the peers' contributions, and most of its work
 * sits in the tiles of the hub sources, whose contributions are the small LAST chunk of every rank's exchange.  So:
 *   gmx_pr_step_gather(p, 0, s)   phase 1 over the tiles that hold hub sources only   (needs the peers' last chunk)
 *   gmx_pr_step_gather(p, 1, s)   phase 1 over the other tiles                        (needs all chunks)
 *   gmx_pr_step_chunk(p, c, s) / gmx_pr_push_chunk(p, c, s) for c = 0 .. chunks-1 as before (the chunks' copies
 *   alternate between two sets of copy streams, so the hub chunk does not queue behind the tail chunk)
 * and the caller may start class 0 of the next step as soon as every rank's LAST chunk has landed
 * (gmx_pr_push_join_chunk(p, chunks-1, s) + its barrier), while the earlier chunks are still travelling; class 1
 * waits for those.  Without the gather calls gmx_pr_step_chunk(p, 0, s) enqueues phase 1 itself. */
/* All launches of one gmx_pr_t (gmx_pr_step, gmx_pr_step_gather, gmx_pr_step_chunk) must be enqueued in call order on
 * ONE stream: the persistent kernels of the binned sweep draw their work from device counters that advance from
 * launch to launch, and the host passes each launch the value it expects to find. */
int gmx_pr_gather_classes(gmx_pr_t* p, int* classes);
int gmx_pr_gather_items(gmx_pr_t* p, int tile_class, int64_t* items);   /* phase-1 work items of a class (set by gmx_pr_set_chunks) */
int gmx_pr_step_gather(gmx_pr_t* p, int tile_class, void* stream);
int gmx_pr_push_join_chunk(gmx_pr_t* p, int chunk, void* stream);
/* Device pointer + element count of the slice of the *current* contribution
 * vector this rank produced in the last step (for the exchange), and of the
 * whole replica. */
int gmx_pr_contrib_slice(gmx_pr_t* p, void** dev_ptr, int64_t* count);
int gmx_pr_contrib_full(gmx_pr_t* p, void** dev_ptr, int64_t* count);
/* Leading entries of every rank's range that have to be exchanged: vertices without out-edges are never
 * gathered and sit at the end of each range in the degree order (same value on every rank; <= slice count). */
int gmx_pr_exchange_count(gmx_pr_t* p, int64_t* count);
/* Device pointer to the fp64 `diff` partial of the last step (1 element). */
int gmx_pr_diff_ptr(gmx_pr_t* p, void** dev_ptr);
/* Blocking: returns diff of the last step (local rows only). */
int gmx_pr_diff(gmx_pr_t* p, void* stream, double* diff);
/* Blocking: ranks of the owned rows scattered into rank_host[V] at original
 * vertex ids (other entries untouched). */
int gmx_pr_download(gmx_pr_t* p, void* rank_host);
/* Device timing of the kernels of gmx_pr_step (the row-reduction kernel plus its small fix-up /
 * combine / diff-reduce kernels: together they move the algorithmic bytes of one iteration), with
 * hipEvents recorded on the stream they are launched on.  enable != 0 starts a fresh
 * measurement; gmx_pr_kernel_time blocks until the recorded steps finished and returns their
 * count and mean duration (bench.py's roofline.achieved uses exactly this). */
int gmx_pr_timing(gmx_pr_t* p, int enable);
int gmx_pr_kernel_time(gmx_pr_t* p, int32_t* launches, double* mean_ms);
/* '+'-joined names of those kernels as rocprofv3 prints them (prefix match). */
const char* gmx_pr_kernel_name(gmx_pr_t* p);
/* Algorithmic bytes / edges one step of this rank processes. */
int gmx_pr_work(gmx_pr_t* p, int64_t* edges, int64_t* rows, int64_t* algorithmic_bytes);
/* The binned part of the plan (GMX_PR_COLD_PB): hot ids per rank range (-1 = no binned part, 0 = every edge is
 * binned), edges taken out of the pull sweep, and the items ((tile, row) pair sums + cell padding) phase 2 streams. */
int gmx_pr_cold_info(gmx_pr_t* p, int64_t* hot_ids, int64_t* cold_edges, int64_t* padded_items);
/* Which code paths a step of the binned part takes, computed on the host from the plan's work lists (no launch, no device
 * read; all zero without a binned part).  Forms, in index order: edge, generic pair, E1, E2, E4, E8, H; tile modes: edge,
 * pair, classed, singles.  A phase-1 SEGMENT is what one call of the prefetch loop walks: a generic pair item, or the piece
 * of a classed item inside one class stream; a super-step is 1024 groups. */
typedef struct gmx_pr_cold_shape {
    int64_t groups[7];        /* tile-major groups (32 entries) the phase-1 items hold, by form */
    uint32_t supersteps[7];   /* bit min(n, 31): some segment of the form runs n whole super-steps (edge form: bit 0 only) */
    int64_t items2_sole;      /* phase-2 items that finish their bin themselves */
    int64_t items2_chunk;     /* phase-2 items that are one chunk of a split bin */
    int64_t bins_few;         /* split bins phase 3 adds with the few-slot kernel (<= 8 chunks) ... */
    int64_t bins_many;        /* ... and with the many-slot kernel */
    int64_t tiles_by_mode[4]; /* tiles with edges, by how they are stored */
    int32_t fused;            /* 1: phases 2-3 apply the PageRank update themselves (every in-edge binned, every bin has items) */
} gmx_pr_cold_shape_t;
int gmx_pr_cold_shape(gmx_pr_t* p, gmx_pr_cold_shape_t* out);

#ifdef __cplusplus
}
#endif
#endif
