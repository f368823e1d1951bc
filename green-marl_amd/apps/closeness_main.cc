// closeness_main.cc -- distance-centrality driver on the common protocol: `<graph> <threads> <nfs> [in|out|both]` (out is
// the default).  in and both build the reverse edges.  The driver calls gmx_closeness on the graph's device mirror with
// every vertex a source, for the exact integers.  The report is the four lines `diameter = <max ecc>`, `radius = <min ecc
// over the vertices with reach > 0>` (0 when there is none), `wiener = <sum of far>` and `top = <vertex of largest harm,
// ties to the lower id>`.
#include "common_main.h"
#include "closeness.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int64_t> far;
    std::vector<int32_t> reach, ecc;
    std::vector<uint64_t> harm;
    int mode = GMX_CLOSE_OUT;
    gmx_stats_t st;
    gm_app app;
    app.usage("[in|out|both]")
        .args([&](const std::vector<std::string>& a) {
            if (a.empty() || a[0] == "out") mode = GMX_CLOSE_OUT;
            else if (a[0] == "in") mode = GMX_CLOSE_IN;
            else if (a[0] == "both") mode = GMX_CLOSE_BOTH;
            else return false;
            return true;
        })
        .setup([&](gm_graph& G) {
            const size_t n = (size_t) G.num_nodes() + 1;
            far.assign(n, 0);
            reach.assign(n, 0);
            ecc.assign(n, 0);
            harm.assign(n, 0);
            if (mode != GMX_CLOSE_OUT) G.make_reverse_edges();
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_closeness(dev, mode, NULL, 0, far.data(), reach.data(), ecc.data(), harm.data(), &st) != GMX_OK) {
                fprintf(stderr, "closeness: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            int32_t diameter = 0, radius = 0;
            int64_t wiener = 0, top = 0;
            bool any = false;
            for (int64_t v = 0; v < (int64_t) G.num_nodes(); v++) {
                diameter = std::max(diameter, ecc[v]);
                if (reach[v] > 0 && (!any || ecc[v] < radius)) {
                    radius = ecc[v];
                    any = true;
                }
                wiener += far[v];
                if (harm[v] > harm[top]) top = v;
            }
            printf("diameter = %d\n", (int) diameter);
            printf("radius = %d\n", (int) radius);
            printf("wiener = %lld\n", (long long) wiener);
            printf("top = %lld\n", (long long) top);
            return true;
        });
    return app.exec(argc, argv);
}
