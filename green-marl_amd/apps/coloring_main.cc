// coloring_main.cc -- greedy vertex colouring driver on the common protocol: `<graph> <threads> <nfs> [degree|id]`.  Order
// degree (the default) is largest degree first, id is first fit in id order (priorities all zero).  The driver builds the
// reverse edges and calls gmx_coloring on the graph's device mirror, for the statistics.  The report is the three lines
// `num_colors = <n>`, `independent_set = <vertices of colour 0>` and `rounds = <rounds of the schedule>`.
#include "common_main.h"
#include "coloring.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int32_t> color, prio;
    bool by_id = false;
    int32_t colors = 0;
    gmx_stats_t st;
    gm_app app;
    app.usage("[degree|id]")
        .args([&](const std::vector<std::string>& a) {
            if (a.empty() || a[0] == "degree") by_id = false;
            else if (a[0] == "id") by_id = true;
            else return false;
            return true;
        })
        .setup([&](gm_graph& G) {
            color.assign((size_t) G.num_nodes() + 1, 0);
            if (by_id) prio.assign((size_t) G.num_nodes() + 1, 0);
            G.make_reverse_edges();
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_coloring(dev, by_id ? prio.data() : NULL, color.data(), NULL, &colors, &st) != GMX_OK) {
                fprintf(stderr, "coloring: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            printf("num_colors = %d\n", (int) colors);
            printf("independent_set = %lld\n", (long long) st.vertices_reached);
            printf("rounds = %lld\n", (long long) st.iterations);
            return true;
        });
    return app.exec(argc, argv);
}
