// closeness.cc -- bodies of the `closeness` procedures, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze(); and, for the modes that pull over in-rows, G.make_reverse_edges().
// The integers come from the device (gmx_closeness: bit-parallel multi-source traversals, 64 sources or more a sweep); it
// reads the CSRs the device mirror keeps, in any row order.  Closeness and the harmonic centrality are derived here.
#include "closeness.h"
#include "gmx.h"

static void closeness_call(gm_graph& G, int mode, const node_t* sources, int32_t nsources, double* G_closeness, double* G_harmonic, int32_t* G_ecc) {
    gm_rt_initialize();
    G.freeze();
    if (mode != GMX_CLOSE_OUT) G.make_reverse_edges();
    const size_t V = (size_t) G.num_nodes();
    std::vector<int64_t> far(G_closeness ? V + 1 : 0);
    std::vector<int32_t> reach(G_closeness ? V + 1 : 0);
    std::vector<uint64_t> harm(G_harmonic ? V + 1 : 0);
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    if (dev == NULL || gmx_closeness(dev, mode, sources, nsources, G_closeness ? far.data() : NULL, G_closeness ? reach.data() : NULL, G_ecc,
                                     G_harmonic ? harm.data() : NULL, &st) != GMX_OK) {
        fprintf(stderr, "closeness: %s\n", gmx_last_error());
        abort();
    }
    for (size_t v = 0; v < V; v++) {
        if (G_closeness) G_closeness[v] = far[v] > 0 ? (double) reach[v] / (double) far[v] : 0.0;
        if (G_harmonic) G_harmonic[v] = (double) harm[v] / 4294967296.0;
    }
    gm_rt_cleanup();
}

void closeness(gm_graph& G, int mode, double* G_closeness, double* G_harmonic, int32_t* G_ecc) {
    closeness_call(G, mode, NULL, 0, G_closeness, G_harmonic, G_ecc);
}

void closeness(gm_graph& G, int mode, const std::vector<node_t>& pivots, double* G_closeness, double* G_harmonic, int32_t* G_ecc) {
    static const node_t none = 0;   // (a list of no pivots is still a list)
    closeness_call(G, mode, pivots.empty() ? &none : pivots.data(), (int32_t) pivots.size(), G_closeness, G_harmonic, G_ecc);
}

void closeness(gm_graph& G, int mode, gm_node_seq& Pivots, double* G_closeness, double* G_harmonic, int32_t* G_ecc) {
    std::vector<node_t> pivots;
    gm_node_seq::seq_iter it = Pivots.prepare_seq_iteration();
    while (it.has_next()) pivots.push_back(it.get_next());
    closeness(G, mode, pivots, G_closeness, G_harmonic, G_ecc);
}
