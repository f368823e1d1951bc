// adamicAdar.cc -- body of the generated `adamicAdar` procedure, MI355X build.  Emitted prologue: gm_rt_initialize();
// G.freeze(); G.do_semi_sort();  (Sum(n: from.Nbrs)(n.IsNbrFrom(to)) is rewritten into from.CommonNbrs(to), which needs
// semi-sorted rows.)  The edge property G_aa is indexed by G's forward edge slots after that prologue: the mirror is
// uploaded from the sorted rows, so the device's slots are G's.
#include "adamicAdar.h"
#include "gmx.h"

void adamicAdar(gm_graph& G, double* G_aa) {
    gm_rt_initialize();
    G.freeze();
    G.do_semi_sort();
    gmx_graph_t* dev = G.device_mirror();
    gmx_stats_t st;
    if (dev == NULL || (G.num_edges() > 0 && gmx_adamic_adar(dev, G_aa, &st) != GMX_OK)) {
        fprintf(stderr, "adamicAdar: %s\n", gmx_last_error());
        abort();
    }
    gm_rt_cleanup();
}
