// kclique_main.cc -- k-clique counting driver on the common protocol: `<graph> <threads> <nfs> [k=4]`, 3 <= k <= 8.  The
// kernel is gmx_kclique on the graph's device mirror (the kclique procedure's call, with the statistics).  The report is the
// four lines `k = <k>`, `cliques = <k-cliques of the graph>`, `max_count = <the largest number of them through one vertex>`
// and `top = <the lowest vertex id with that count>`.
#include "common_main.h"
#include "kclique.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int64_t> count;
    int32_t k = 4;
    int64_t cliques = 0;
    gmx_stats_t st;
    gm_app app;
    app.usage("[k=4]")
        .args([&](const std::vector<std::string>& a) {
            if (!a.empty()) k = (int32_t) atoi(a[0].c_str());
            return k >= 3 && k <= 8;
        })
        .setup([&](gm_graph& G) {
            count.assign((size_t) G.num_nodes() + 1, 0);
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_kclique(dev, k, count.data(), &cliques, &st) != GMX_OK) {
                fprintf(stderr, "kclique: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            const int64_t V = (int64_t) G.num_nodes();
            int64_t top = 0;
            for (int64_t v = 1; v < V; v++)
                if (count[(size_t) v] > count[(size_t) top]) top = v;
            printf("k = %d\n", (int) k);
            printf("cliques = %lld\n", (long long) cliques);
            printf("max_count = %lld\n", (long long) (V ? count[(size_t) top] : 0));
            printf("top = %lld\n", (long long) top);
            return true;
        });
    return app.exec(argc, argv);
}
