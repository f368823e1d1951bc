// louvain.cc -- body of the `louvain` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The partition comes from the device (gmx_louvain: integer scores in
// 128 bits, half-rounds judged by the exact modularity numerator); it reads the forward CSR the device mirror keeps, in any row
// order.  The edge property is indexed by the forward edge slot, the node property by node id; both stay the caller's.
#include "louvain.h"
#include "gmx.h"

double louvain(gm_graph& G, int32_t* G_weight, node_t* G_comm) {
    static_assert(sizeof(node_t) == sizeof(gmx_node_t), "gmx_louvain writes one gmx_node_t per node");
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    double q = 0.0;
    if (dev == NULL || gmx_louvain(dev, G_weight, 32, 64, (gmx_node_t*) G_comm, NULL, NULL, &q, NULL, &st) != GMX_OK) {
        fprintf(stderr, "louvain: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return q;
}
