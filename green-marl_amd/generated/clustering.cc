// clustering.cc -- body of the `clustering` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The counts come from the device (gmx_clustering); it reads the forward
// CSR the device mirror keeps, in any row order, and caches its plan on the mirror.
#include "clustering.h"
#include "gmx.h"

int64_t clustering(gm_graph& G, int64_t* G_tri, double* G_lcc, int64_t& wedges) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t triangles = 0, w = 0;
    if (dev == NULL || gmx_clustering(dev, G_tri, NULL, G_lcc, &triangles, &w, &st) != GMX_OK) {
        fprintf(stderr, "clustering: %s\n", gmx_last_error());
        abort();
    }
    wedges = w;
    gm_rt_cleanup();
    return triangles;
}
