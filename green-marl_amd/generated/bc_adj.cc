// bc_adj.cc -- body of the generated `comp_BC(G, BC)` procedure of bc_adj.gm, MI355X build: exact betweenness centrality,
// bc.gm's sweeps from every vertex as source, `For (s: G.Nodes)`, in node order, with upstream's (v != s) filters
// (bc_adj.gm:17, :21) -- gmx_bc_all with skip_root = 1.  Emitted prologue: gm_rt_initialize(); G.freeze();
// G.make_reverse_edges();  (UpNbrs walks the reverse rows.)
#include "bc_adj.h"
#include "gmx.h"

void comp_BC(gm_graph& G, float* G_BC) {
    gm_rt_initialize();
    G.freeze();
    G.make_reverse_edges();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    if (dev == NULL || gmx_bc_all(dev, /*skip_root*/ 1, /*width*/ 0, G_BC, &st) != GMX_OK) {
        fprintf(stderr, "comp_BC: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
}
