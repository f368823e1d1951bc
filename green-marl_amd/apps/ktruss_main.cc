// ktruss_main.cc -- k-truss decomposition driver on the common protocol: `<graph> <threads> <nfs>`.  The kernel is gmx_ktruss
// on the graph's device mirror (the ktruss procedure's call, with the statistics).  The report is the five lines
// `max_truss = <k>`, `max_truss_edges = <undirected edges with that number>`, `num_edges = <undirected edges>`,
// `triangles = <sum of the support over the undirected edges / 3>` and `rounds = <rounds that removed something>`.
#include "common_main.h"
#include "ktruss.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int32_t> support;
    std::vector<int32_t> truss;
    int32_t max_truss = 0;
    int64_t num_edges = 0;
    gmx_stats_t st;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) {
            support.assign((size_t) G.num_edges() + 1, 0);
            truss.assign((size_t) G.num_edges() + 1, 0);
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_ktruss(dev, truss.data(), support.data(), &max_truss, &num_edges, &st) != GMX_OK) {
                fprintf(stderr, "ktruss: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            // one (edge, support) key per slot; the repeats and the other orientation of an edge fall together
            const int64_t V = (int64_t) G.num_nodes();
            std::vector<std::pair<int64_t, int32_t>> keys;
            for (int64_t u = 0; u < V; u++)
                for (edge_t e = G.begin[u]; e < G.begin[u + 1]; e++) {
                    const int64_t w = (int64_t) G.node_idx[e];
                    if (w != u) keys.push_back({std::min(u, w) * V + std::max(u, w), support[(size_t) e]});
                }
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            int64_t sum = 0;
            for (const auto& k : keys) sum += k.second;
            printf("max_truss = %d\n", (int) max_truss);
            printf("max_truss_edges = %lld\n", (long long) st.vertices_reached);
            printf("num_edges = %lld\n", (long long) num_edges);
            printf("triangles = %lld\n", (long long) (sum / 3));
            printf("rounds = %lld\n", (long long) st.iterations);
            return true;
        });
    return app.exec(argc, argv);
}
