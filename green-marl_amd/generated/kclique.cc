// kclique.cc -- body of the `kclique` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The results come from the device (gmx_kclique: bit matrices among every
// vertex's upper neighbours, counted by AND and popcount); it reads the forward CSR the device mirror keeps, in any row order.
// The node property is indexed by node id and stays the caller's.
#include "kclique.h"
#include "gmx.h"

int64_t kclique(gm_graph& G, int32_t k, int64_t* G_cnt) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t cliques = 0;
    if (dev == NULL || gmx_kclique(dev, k, G_cnt, &cliques, &st) != GMX_OK) {
        fprintf(stderr, "kclique: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return cliques;
}
