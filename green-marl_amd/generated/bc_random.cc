// bc_random.cc -- body of the generated `bc_random` procedure, MI355X build: estimated betweenness centrality from K
// random sources (apps/src/bc_random.gm).  Emitted prologue as comp_BC's (bc.cc).  The emission draws `s = G.PickRandom()`
// at the top of every iteration of `While (k < K)` and nothing else in the loop consumes rand(), so the K draws made here
// up front, in loop order, are the emission's; the K traversals and sweeps are then one gmx_bc_batch call, whose result is
// the sequential loop's bit for bit (include/gmx.h).  GMX_BC_SKIP_ROOT as in bc.cc: bc_random.gm lacks the `(v != s)`
// filters too.
#include "bc_random.h"
#include "gmx.h"
#include <vector>

void bc_random(gm_graph& G, float* G_BC, int32_t K) {
    gm_rt_initialize();
    G.freeze();
    G.make_reverse_edges();
    std::vector<node_t> seeds;
    for (int32_t k = 0; k < K; k++) seeds.push_back(G.pick_random_node());
    const char* skip = getenv("GMX_BC_SKIP_ROOT");
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    if (dev == NULL || gmx_bc_batch(dev, seeds.data(), (int32_t) seeds.size(), skip && atoi(skip) != 0, 0, G_BC, &st) != GMX_OK) {
        fprintf(stderr, "bc_random: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
}
