// graphlets_main.cc -- 4-node graphlet census driver on the common protocol: `<graph> <threads> <nfs>`.  The kernel is
// gmx_graphlets on the graph's device mirror (the graphlets procedure's call, with the statistics), induced counts.  The
// report is the nine lines `edges =`, `paths3 =`, `triangles =`, `paths4 =`, `claws =`, `cycles4 =`, `paws =`, `diamonds =`,
// `cliques4 =` and `top = <the lowest vertex id with the largest number of 4-cliques through it>`.
#include "common_main.h"
#include "graphlets.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int64_t> gdv;
    int64_t totals[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    gmx_stats_t st;
    gm_app app;
    app.setup([&](gm_graph& G) {
            gdv.assign(((size_t) G.num_nodes() + 1) * 15, 0);
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_graphlets(dev, 1, gdv.data(), totals, &st) != GMX_OK) {
                fprintf(stderr, "graphlets: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            const int64_t V = (int64_t) G.num_nodes();
            static const char* const names[9] = {"edges", "paths3", "triangles", "paths4", "claws", "cycles4", "paws", "diamonds", "cliques4"};
            int64_t top = 0;
            for (int64_t v = 1; v < V; v++)
                if (gdv[(size_t) v * 15 + 14] > gdv[(size_t) top * 15 + 14]) top = v;
            for (int j = 0; j < 9; j++) printf("%s = %lld\n", names[j], (long long) totals[j]);
            printf("top = %lld\n", (long long) top);
            return true;
        });
    return app.exec(argc, argv);
}
