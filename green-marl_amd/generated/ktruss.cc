// ktruss.cc -- body of the `ktruss` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The results come from the device (gmx_ktruss: per-edge support, then
// peeling in queue rounds); it reads the forward CSR the device mirror keeps, in any row order.  The edge properties are
// indexed by the forward edge slot and stay the caller's.
#include "ktruss.h"
#include "gmx.h"

int32_t ktruss(gm_graph& G, int32_t* G_truss, int32_t* G_support) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int32_t max_truss = 0;
    int64_t num_edges = 0;
    if (dev == NULL || gmx_ktruss(dev, G_truss, G_support, &max_truss, &num_edges, &st) != GMX_OK) {
        fprintf(stderr, "ktruss: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return max_truss;
}
