// kcore.cc -- body of the `kcore` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The core numbers come from the device (gmx_kcore, mode IN: peeling in
// queue rounds); it reads the forward CSR the device mirror keeps, in any row order.
#include "kcore.h"
#include "gmx.h"

int32_t kcore(gm_graph& G, int32_t* G_core) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int32_t max_core = 0;
    if (dev == NULL || gmx_kcore(dev, GMX_KCORE_IN, G_core, NULL, &max_core, &st) != GMX_OK) {
        fprintf(stderr, "kcore: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return max_core;
}
