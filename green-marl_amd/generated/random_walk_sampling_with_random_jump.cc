// random_walk_sampling_with_random_jump.cc -- the generated `random_walk_sampling_with_random_jump` procedure.  One walker
// takes N dependent steps: the program is serial by nature and has no device entry.  This is the host loop, on the same
// stream as the device programs: G.PickRandom() is (node_t) (Uniform() * (double) V) here (the reference's draws from libc
// rand(), which is not a portable stream) and n.PickRandomNbr() is gm_graph::pick_random_out_neighbor.
#include "random_walk_sampling_with_random_jump.h"

void random_walk_sampling_with_random_jump(gm_graph& G, int32_t N, double c, gm_node_set& S) {
    gm_rt_initialize();
    G.freeze();
    if (G.num_nodes() == 0) return;
    node_t n = (node_t) (gm_rt_uniform(0) * (double) G.num_nodes());
    int32_t count = 0;
    while (count < N) {
        S.add(n);
        count++;
        if (G.begin[n + 1] == G.begin[n] || gm_rt_uniform(0) < c)
            n = (node_t) (gm_rt_uniform(0) * (double) G.num_nodes());
        else
            n = G.pick_random_out_neighbor(n);
    }
    gm_rt_cleanup();
}
