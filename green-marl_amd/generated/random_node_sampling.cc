// random_node_sampling.cc -- body of the generated `random_node_sampling` procedure, MI355X build.  Emitted prologue:
// gm_rt_initialize(); G.freeze();  Vertex v takes draw v + 1 of thread 0's stream of the runtime shim (the program run by
// one thread) and joins S when dice < 1 / (Double) N; the state is stored back advanced by V (gmx.h: the stream).
#include "random_node_sampling.h"
#include "gmx.h"

#include <vector>

void random_node_sampling(gm_graph& G, int32_t N, gm_node_set& S) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t count = 0;
    std::vector<uint8_t> sel((size_t) G.num_nodes() + 1);
    if (dev == NULL || gmx_node_sampling(dev, 0, N, gm_rt_rand_state(0), sel.data(), &count, &st) != GMX_OK) {
        fprintf(stderr, "random_node_sampling: %s\n", gmx_last_error());
        abort();
    }
    for (node_t v = 0; v < G.num_nodes(); v++)   // (S.Add: members the caller put in before stay)
        if (sel[v]) S.add(v);
    gm_rt_cleanup();
}
