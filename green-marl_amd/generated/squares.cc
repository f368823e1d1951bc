// squares.cc -- body of the `squares` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The results come from the device (gmx_squares: the wedges below every
// vertex counted into a table keyed by their far end); it reads the forward CSR the device mirror keeps, in any row order.
// The node property is indexed by node id and stays the caller's.
#include "squares.h"
#include "gmx.h"

int64_t squares(gm_graph& G, int64_t* G_cnt) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t n = 0;
    if (dev == NULL || gmx_squares(dev, G_cnt, &n, &st) != GMX_OK) {
        fprintf(stderr, "squares: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return n;
}
