// sssp_dijkstra.cc -- body of the generated `dijkstra` procedure of sssp_dijkstra.gm, MI355X build.  Emitted prologue:
// gm_rt_initialize(); G.freeze();  (Nbrs and ToEdge only.)  It runs on the engine of bidir_dijkstra.cc, which also holds the
// `get_path` the two programs have in common: flag and route are what a one-sided search would return, found from both ends
// (GMX_ROUTE_SIDES=forward searches from root only).  Parent / ParentEdge are NIL off the returned route.
#include "sssp_dijkstra.h"

bool gm_route_entry(const char* who, gm_graph& G, int32_t* G_Weight, node_t src, node_t dst, node_t* G_Parent, edge_t* G_ParentEdge);   // bidir_dijkstra.cc

bool dijkstra(gm_graph& G, int32_t* G_Len, node_t& root, node_t& dest, node_t* G_Parent, edge_t* G_ParentEdge) {
    gm_rt_initialize();
    G.freeze();
    const bool found = gm_route_entry("dijkstra", G, G_Len, root, dest, G_Parent, G_ParentEdge);
    gm_rt_cleanup();
    return found;
}
