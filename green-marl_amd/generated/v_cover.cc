// v_cover.cc -- body of the generated `v_cover` procedure, MI355X build.  Emitted prologue: gm_rt_initialize(); G.freeze();
// G.make_reverse_edges();  (InDegree needs the reverse edges; Nbrs, InDegree and ToEdge need no semi-sorted rows.)  The
// edge property G_select is indexed by G's forward edge slots: the mirror reports its result in the uploaded slots, which
// are G's.  The device runs the loop as one thread of the reference would: ties go to the lowest slot (gmx.h).
#include "v_cover.h"
#include "gmx.h"

int32_t v_cover(gm_graph& G, bool* G_select) {
    static_assert(sizeof(bool) == sizeof(uint8_t), "select is exchanged as bytes");
    gm_rt_initialize();
    G.freeze();
    G.make_reverse_edges();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int32_t covered = 0;
    if (dev == NULL || gmx_v_cover(dev, (uint8_t*) G_select, &covered, &st) != GMX_OK) {
        fprintf(stderr, "v_cover: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return covered;
}
