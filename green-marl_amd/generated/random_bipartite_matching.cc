// random_bipartite_matching.cc -- body of the generated `random_bipartite_matching` procedure, MI355X build.  Emitted
// prologue: gm_rt_initialize(); G.freeze();  (Nbrs only: no reverse edges, no semi-sorted rows.)  The node properties
// G_isLeft and G_Match are indexed by vertex.  The device runs the loop as one thread of the reference would: a right takes
// its largest proposing left, a left its largest replying right (gmx.h).
#include "random_bipartite_matching.h"
#include "gmx.h"

int32_t random_bipartite_matching(gm_graph& G, bool* G_isLeft, node_t* G_Match) {
    static_assert(sizeof(bool) == sizeof(uint8_t), "isLeft is exchanged as bytes");
    static_assert(sizeof(node_t) == sizeof(gmx_node_t), "Match is exchanged as gmx_node_t");
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int32_t count = 0;
    if (dev == NULL || gmx_random_bipartite_matching(dev, (const uint8_t*) G_isLeft, (gmx_node_t*) G_Match, &count, &st) != GMX_OK) {
        fprintf(stderr, "random_bipartite_matching: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return count;
}
