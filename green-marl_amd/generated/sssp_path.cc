// sssp_path.cc -- bodies of the generated `sssp_path` and `get_path` procedures, MI355X build.
// Emitted prologue of sssp_path: gm_rt_initialize(); G.freeze();   G_len is indexed by the forward edge slot and stays the
// caller's, as in sssp.cc.  G_prev is a shortest-path tree of G_dist: where several predecessors are equally short the
// device records the smallest (gmx.h, gmx_sssp_path), the reference whichever thread wrote first.
#include "sssp_path.h"
#include "gmx.h"

void sssp_path(gm_graph& G, int32_t* G_dist, int32_t* G_len, node_t& root, node_t* G_prev) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    if (dev == NULL || gmx_sssp_path(dev, root, G_len, G_dist, G_prev, NULL, &st) != GMX_OK) {
        fprintf(stderr, "sssp_path: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
}

// sssp_path.gm:33-42, on the host: the path begin .. end along prev, or nothing when end has no predecessor
void get_path(gm_graph& G, node_t& begin, node_t& end, node_t* G_prev, gm_node_seq& Q) {
    (void) G;
    node_t t = end;
    if (G_prev[end] != gm_graph::NIL_NODE) {
        while (t != begin) {
            Q.push_front(t);
            t = G_prev[t];
        }
        Q.push_front(t);
    }
}
