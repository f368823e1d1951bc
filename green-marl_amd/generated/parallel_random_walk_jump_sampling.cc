// parallel_random_walk_jump_sampling.cc -- body of the generated `parallel_random_walk_jump_sampling` procedure, MI355X
// build.  Emitted prologue: gm_rt_initialize(); G.freeze();  (Nbrs only: no reverse edges, no semi-sorted rows.)  The device
// runs the program as one thread of the reference would, on thread 0's stream of the runtime shim, and the state it leaves
// is stored back, so a Uniform() after the call continues where the program stopped (gmx.h: the stream).  The program has
// no round limit: INT32_MAX is passed, and with p_jump = 0 on a closed component it does not return, like the reference.
#include "parallel_random_walk_jump_sampling.h"
#include "gmx.h"

void parallel_random_walk_jump_sampling(gm_graph& G, float p_size, float p_jump, int32_t num_tokens, bool* G_Selected) {
    static_assert(sizeof(bool) == sizeof(uint8_t), "Selected is exchanged as bytes");
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t count = 0;
    int32_t rounds = 0;
    if (dev == NULL || gmx_random_walk_sampling(dev, p_size, p_jump, num_tokens, INT32_MAX, gm_rt_rand_state(0), (uint8_t*) G_Selected, NULL, &count,
                                                &rounds, &st) != GMX_OK) {
        fprintf(stderr, "parallel_random_walk_jump_sampling: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
}
