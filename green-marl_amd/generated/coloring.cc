// coloring.cc -- bodies of the `coloring` procedures, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze(); G.make_reverse_edges();  (a vertex's neighbours are its out-row and its
// in-row.)  The colours come from the device (gmx_coloring: Jones-Plassmann rounds that compute the one-thread first fit);
// it reads both CSRs the device mirror keeps, in any row order.
#include "coloring.h"
#include "gmx.h"

int32_t coloring(gm_graph& G, int32_t* G_prio, int32_t* G_color) {
    gm_rt_initialize();
    G.freeze();
    G.make_reverse_edges();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int32_t colors = 0;
    if (dev == NULL || gmx_coloring(dev, G_prio, G_color, NULL, &colors, &st) != GMX_OK) {
        fprintf(stderr, "coloring: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return colors;
}

int32_t coloring(gm_graph& G, int32_t* G_color) { return coloring(G, (int32_t*) NULL, G_color); }
