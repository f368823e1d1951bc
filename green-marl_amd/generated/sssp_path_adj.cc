// sssp_path_adj.cc -- bodies of the generated `sssp_path` and `get_path` procedures of sssp_path_adj.gm, MI355X build.
// Emitted prologue of sssp_path: gm_rt_initialize(); G.freeze();  (Nbrs and ToEdge only: no reverse edges, no semi-sorted
// rows.)  G_edge_cost is indexed by G's forward edge slots and stays the caller's; G_prev_edge comes back in the same slots.
// The device runs the loop as one thread of the reference would (gmx.h, gmx_sssp_path_f64).
#include "sssp_path_adj.h"
#include "gmx.h"

#include <vector>

void sssp_path(gm_graph& G, double* G_dist, double* G_edge_cost, node_t& root, node_t& end, node_t* G_prev_node, edge_t* G_prev_edge) {
    static_assert(sizeof(node_t) == sizeof(gmx_node_t), "prev_node is exchanged as gmx_node_t");
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    // edge_t is 64 bits wide in the GM_EDGE64 build: the device's slots pass through a temporary there
    std::vector<gmx_edge_t> slots;
    gmx_edge_t* prev_edge = (gmx_edge_t*) G_prev_edge;
    if (sizeof(edge_t) != sizeof(gmx_edge_t) && G_prev_edge != NULL) {
        slots.resize((size_t) G.num_nodes() + 1);
        prev_edge = slots.data();
    }
    if (dev == NULL || gmx_sssp_path_f64(dev, root, end, G_edge_cost, G_dist, G_prev_node, prev_edge, &st) != GMX_OK) {
        fprintf(stderr, "sssp_path: %s\n", gmx_last_error());
        abort();
    }
    if (prev_edge != (gmx_edge_t*) G_prev_edge)
        for (node_t v = 0; v < G.num_nodes(); v++) G_prev_edge[v] = (edge_t) slots[(size_t) v];
    gm_rt_cleanup();
}

// sssp_path_adj.gm:36-48, on the host: the path after begin up to end along prev_node, and the sum of its edge costs
// from end backwards; nothing and 0 when end has no predecessor.  begin itself is not pushed.
double get_path(gm_graph& G, node_t& begin, node_t& end, node_t* G_prev_node, edge_t* G_prev_edge, double* G_edge_cost, gm_node_seq& Q) {
    (void) G;
    double total_cost = 0.0;
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
