// msf_main.cc -- minimum spanning forest driver on the common protocol.  The weights are (rand % 100) + 1 drawn from
// gm_rand32 in slot order, as sssp_main.cc draws its lengths.  The kernel is gmx_msf on the graph's device mirror, which
// also returns the counts that the msf procedure does not; the report is the four lines `forest_edges = <n>`,
// `total_weight = <w>`, `num_components = <c>` and `rounds = <rounds that merged something>`.
#include "common_main.h"
#include "msf.h"
#include "gm_rand.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int32_t> weight;
    std::vector<uint8_t> in_forest;
    int64_t forest_edges = 0, total_weight = 0, num_components = 0;
    gmx_stats_t st;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) {
            gm_rand32 rng;
            weight.resize((size_t) G.num_edges());
            for (int32_t& w : weight) w = (rng.rand() % 100) + 1;   // 1 .. 100
            in_forest.assign((size_t) G.num_edges() + 1, 0);
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_msf(dev, weight.data(), in_forest.data(), &forest_edges, &total_weight, NULL, &num_components, &st) != GMX_OK) {
                fprintf(stderr, "msf: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            printf("forest_edges = %lld\n", (long long) forest_edges);
            printf("total_weight = %lld\n", (long long) total_weight);
            printf("num_components = %lld\n", (long long) num_components);
            printf("rounds = %lld\n", (long long) st.iterations);
            return true;
        });
    return app.exec(argc, argv);
}
