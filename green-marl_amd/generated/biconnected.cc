// biconnected.cc -- body of the `biconnected` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze(); G.make_reverse_edges();   The results come from the device (gmx_biconnected: a spanning forest
// and one walk per non-tree slot); it reads both CSRs the device mirror keeps, in any row order.  The edge properties are
// indexed by the forward edge slot and stay the caller's.
#include "biconnected.h"
#include "gmx.h"

int64_t biconnected(gm_graph& G, bool* G_bridge, bool* G_artic, int32_t* G_block, int32_t* G_tecc, int64_t& num_bridges, int64_t& num_artic,
                    int64_t& num_tecc) {
    static_assert(sizeof(bool) == sizeof(uint8_t), "gmx_biconnected writes one byte per flag");
    gm_rt_initialize();
    G.freeze();
    G.make_reverse_edges();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t blocks = 0, nb = 0, na = 0, nt = 0;
    if (dev == NULL || gmx_biconnected(dev, (uint8_t*) G_bridge, (uint8_t*) G_artic, G_block, G_tecc, &blocks, &nb, &na, &nt, &st) != GMX_OK) {
        fprintf(stderr, "biconnected: %s\n", gmx_last_error());
        abort();
    }
    num_bridges = nb;
    num_artic = na;
    num_tecc = nt;
    gm_rt_cleanup();
    return blocks;
}
