// msf.cc -- body of the `msf` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The forest comes from the device (gmx_msf: Boruvka's rounds); it reads
// the forward CSR the device mirror keeps, in any row order.  The edge properties are indexed by the forward edge slot and
// stay the caller's: the weights are copied in and the flags out on every call.
#include "msf.h"
#include "gmx.h"

int64_t msf(gm_graph& G, int32_t* G_weight, bool* G_in_forest) {
    static_assert(sizeof(bool) == sizeof(uint8_t), "gmx_msf writes one byte per edge slot");
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t total = 0;
    if (dev == NULL || gmx_msf(dev, G_weight, (uint8_t*) G_in_forest, NULL, &total, NULL, NULL, &st) != GMX_OK) {
        fprintf(stderr, "msf: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return total;
}
