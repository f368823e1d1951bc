// kcore_main.cc -- k-core decomposition driver on the common protocol: `<graph> <threads> <nfs> [in|out|both]`.  Mode in is
// the kcore procedure; out and both build the reverse edges and call gmx_kcore on the graph's device mirror.  The report
// is the three lines `max_core = <k>`, `max_core_size = <vertices of that core>` and `rounds = <rounds that removed something>`.
#include "common_main.h"
#include "kcore.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int32_t> core;
    int mode = GMX_KCORE_IN;
    int32_t max_core = 0;
    gmx_stats_t st;
    gm_app app;
    app.usage("[in|out|both]")
        .args([&](const std::vector<std::string>& a) {
            if (a.empty() || a[0] == "in") mode = GMX_KCORE_IN;
            else if (a[0] == "out") mode = GMX_KCORE_OUT;
            else if (a[0] == "both") mode = GMX_KCORE_BOTH;
            else return false;
            return true;
        })
        .setup([&](gm_graph& G) {
            core.assign((size_t) G.num_nodes() + 1, 0);
            if (mode != GMX_KCORE_IN) G.make_reverse_edges();
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_kcore(dev, mode, core.data(), NULL, &max_core, &st) != GMX_OK) {
                fprintf(stderr, "kcore: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            printf("max_core = %d\n", (int) max_core);
            printf("max_core_size = %lld\n", (long long) st.vertices_reached);
            printf("rounds = %lld\n", (long long) st.iterations);
            return true;
        });
    return app.exec(argc, argv);
}
