// graphlets.cc -- body of the `graphlets` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The results come from the device (gmx_graphlets: row sums over the
// triangle supports, one weighted walk of the triangles, the squares and the 4-cliques, then the transform to induced
// counts); it reads the forward CSR the device mirror keeps, in any row order.  The node property is indexed by node id and
// stays the caller's.
#include "graphlets.h"
#include "gmx.h"

void graphlets(gm_graph& G, int64_t* G_gdv, int64_t* totals) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    if (dev == NULL || gmx_graphlets(dev, 1, G_gdv, totals, &st) != GMX_OK) {
        fprintf(stderr, "graphlets: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
}
