// wcc.cc -- body of the `wcc` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The components come from the device (gmx_wcc: neighbour sampling,
// then the rows of the vertices outside the giant tree); it reads the CSRs the device mirror keeps, in any row order.
#include "wcc.h"
#include "gmx.h"

int32_t wcc(gm_graph& G, node_t* G_comp) {
    static_assert(sizeof(node_t) == sizeof(int32_t), "gmx_wcc writes 32-bit component ids");
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t count = 0;
    if (dev == NULL || gmx_wcc(dev, (int32_t*) G_comp, &count, &st) != GMX_OK) {
        fprintf(stderr, "wcc: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return (int32_t) count;
}
