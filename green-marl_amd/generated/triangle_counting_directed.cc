// triangle_counting_directed.cc -- body of the generated `triangle_counting_directed` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze(); G.do_semi_sort();  (HasEdgeTo marks the procedure NEED_SEMI_SORT,
// src/backend_cpp/gm_cpp_gen_misc_check.cc:40-47).  The device entry itself reads rows in any order.
#include "triangle_counting_directed.h"
#include "gmx.h"

int64_t triangle_counting_directed(gm_graph& G) {
    gm_rt_initialize();
    G.freeze();
    G.do_semi_sort();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    int64_t T = 0;
    if (dev == NULL || gmx_triangle_counting_directed(dev, &T, &st) != GMX_OK) {
        fprintf(stderr, "triangle_counting_directed: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
    return T;
}
