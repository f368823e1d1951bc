// bidir_dijkstra.cc -- bodies of the generated `bidir_dijkstra` (bidir_dijkstra.gm), of the `get_path` it has in common with
// sssp_dijkstra.gm, and of the call both programs' entries make (`dijkstra` itself: sssp_dijkstra.cc), MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze(); G.make_reverse_edges() (InNbrs).  The weights are indexed by G's forward
// edge slots and stay the caller's; ParentEdge comes back in the same slots.  Both programs run on the device's route engine
// (gmx.h, gmx_bidir_dijkstra).  The device mirror of a gm_graph always has its reverse CSR, so both search from the two ends;
// GMX_ROUTE_SIDES=forward gives sssp_dijkstra.gm's one-sided search with early exit, and flag and cost are the same either
// way.  Parent / ParentEdge are NIL off the returned route, and src == dst is found with the empty route: the two departures
// from the reference that gmx.h documents.
#include "bidir_dijkstra.h"
#include "gmx.h"

#include <vector>

bool gm_route_entry(const char* who, gm_graph& G, int32_t* G_Weight, node_t src, node_t dst, node_t* G_Parent, edge_t* G_ParentEdge) {
    static_assert(sizeof(node_t) == sizeof(gmx_node_t), "Parent is exchanged as gmx_node_t");
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    // edge_t is 64 bits wide in the GM_EDGE64 build: the device's slots pass through a temporary there
    std::vector<gmx_edge_t> slots;
    gmx_edge_t* parent_edge = (gmx_edge_t*) G_ParentEdge;
    if (sizeof(edge_t) != sizeof(gmx_edge_t) && G_ParentEdge != NULL) {
        slots.resize((size_t) G.num_nodes() + 1);
        parent_edge = slots.data();
    }
    int32_t found = 0;
    if (dev == NULL || gmx_bidir_dijkstra(dev, G_Weight, src, dst, G_Parent, parent_edge, &found, &st) != GMX_OK) {
        fprintf(stderr, "%s: %s\n", who, gmx_last_error());
        abort();
    }
    if (parent_edge != (gmx_edge_t*) G_ParentEdge)
        for (node_t v = 0; v < G.num_nodes(); v++) G_ParentEdge[v] = (edge_t) slots[(size_t) v];
    return found != 0;
}

bool bidir_dijkstra(gm_graph& G, int32_t* G_Weight, node_t& src, node_t& dst, node_t* G_Parent, edge_t* G_ParentEdge) {
    gm_rt_initialize();
    G.freeze();
    G.make_reverse_edges();
    const bool found = gm_route_entry("bidir_dijkstra", G, G_Weight, src, dst, G_Parent, G_ParentEdge);
    gm_rt_cleanup();
    return found;
}

// bidir_dijkstra.gm:125-137 = sssp_dijkstra.gm:57-70, on the host: the path after begin up to end along prev_node, and the
// sum of its edge costs from end backwards; nothing and 0 when end has no predecessor.  begin itself is not pushed.
int32_t get_path(gm_graph& G, node_t& begin, node_t& end, node_t* G_prev_node, edge_t* G_prev_edge, int32_t* G_edge_cost, gm_node_seq& Q) {
    (void) G;
    int32_t total_cost = 0;
    node_t n = end;
    if (G_prev_node[end] != gm_graph::NIL_NODE) {
        while (n != begin) {
            Q.push_front(n);
            const edge_t e = G_prev_edge[n];
            total_cost += G_edge_cost[e];
            n = G_prev_node[n];
        }
    }
    return total_cost;
}
