// kosaraju.cc -- body of the generated `kosaraju` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The components come from the device (gmx_scc: trim, forward-backward
// reachability and colouring); the reverse CSR they need is the one the device mirror keeps.
#include "kosaraju.h"
#include "gmx.h"

int32_t kosaraju(gm_graph& G, int32_t* G_mem) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t count = 0;
    if (dev == NULL || gmx_scc(dev, G_mem, &count, &st) != GMX_OK) {
        fprintf(stderr, "kosaraju: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return (int32_t) count;
}
