// louvain_main.cc -- Louvain modularity communities driver on the common protocol.  The weights are (rand % 100) + 1 drawn from
// gm_rand32 in slot order, as msf_main.cc draws its weights.  The kernel is gmx_louvain on the graph's device mirror (the
// louvain procedure's call, with the counts that the procedure does not return); the report is the four lines
// `num_communities = <n>`, `num_levels = <levels that kept a move>`, `modularity = <Q, 17 significant digits>` and
// `largest_community = <members of the largest community>`.
#include "common_main.h"
#include "louvain.h"
#include "gm_rand.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int32_t> weight;
    std::vector<gmx_node_t> comm;
    int32_t num_comms = 0, num_levels = 0;
    double q = 0.0;
    gmx_stats_t st;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) {
            gm_rand32 rng;
            weight.resize((size_t) G.num_edges());
            for (int32_t& w : weight) w = (rng.rand() % 100) + 1;   // 1 .. 100
            comm.assign((size_t) G.num_nodes() + 1, 0);
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_louvain(dev, weight.data(), 32, 64, comm.data(), &num_comms, &num_levels, &q, NULL, &st) != GMX_OK) {
                fprintf(stderr, "louvain: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            const int64_t V = (int64_t) G.num_nodes();
            std::vector<int64_t> size((size_t) num_comms + 1, 0);
            int64_t largest = 0;
            for (int64_t v = 0; v < V; v++) {
                const int64_t s = ++size[(size_t) comm[(size_t) v]];
                if (s > largest) largest = s;
            }
            printf("num_communities = %d\n", (int) num_comms);
            printf("num_levels = %d\n", (int) num_levels);
            printf("modularity = %.17g\n", q);
            printf("largest_community = %lld\n", (long long) largest);
            return true;
        });
    return app.exec(argc, argv);
}
