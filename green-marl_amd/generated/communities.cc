// communities.cc -- body of the generated `communities` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The labels come from the device (gmx_communities: half-rounds of
// label counting over the forward rows; the reverse CSR of the device mirror feeds the work list).  The reference's loop
// has no bound; GMX_COMM_MAX_ROUNDS (default 1000) is the device's.
#include "communities.h"
#include "gmx.h"

void communities(gm_graph& G, node_t* G_Comm) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    const char* env = getenv("GMX_COMM_MAX_ROUNDS");
    const int32_t max_rounds = env && *env ? (int32_t) std::max(0, atoi(env)) : 1000;
    int32_t rounds = 0, converged = 0;
    if (dev == NULL || gmx_communities(dev, max_rounds, G_Comm, &rounds, &converged, NULL) != GMX_OK) {
        fprintf(stderr, "communities: %s\n", gmx_last_error());
        abort();
    }
    if (!converged) fprintf(stderr, "communities: no fixpoint after %d rounds (GMX_COMM_MAX_ROUNDS)\n", (int) max_rounds);
    gm_rt_cleanup();
}
