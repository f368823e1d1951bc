// clustering_main.cc -- per-vertex triangle counts and clustering coefficients, driver on the common protocol:
// `<graph> <threads> <nfs>`.  The kernel is the clustering procedure.  The report is the five lines `triangles = <T>`,
// `wedges = <W>`, `transitivity = <3 T / W, or 0 without wedges>`, `avg_clustering = <the sum of lcc in id order, added
// sequentially in double, over V>` (both %.17g) and `top = <lowest id of the largest tri>`.
#include "common_main.h"
#include "clustering.h"

int main(int argc, char** argv) {
    std::vector<int64_t> tri;
    std::vector<double> lcc;
    int64_t triangles = 0, wedges = 0;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) {
            tri.assign((size_t) G.num_nodes() + 1, 0);
            lcc.assign((size_t) G.num_nodes() + 1, 0.0);
            return true;
        })
        .kernel([&](gm_graph& G) {
            triangles = clustering(G, tri.data(), lcc.data(), wedges);
            return true;
        })
        .report([&](gm_graph& G) {
            const int64_t V = (int64_t) G.num_nodes();
            double sum = 0;
            int64_t top = 0;
            for (int64_t v = 0; v < V; v++) {
                sum += lcc[(size_t) v];
                if (tri[(size_t) v] > tri[(size_t) top]) top = v;
            }
            printf("triangles = %lld\n", (long long) triangles);
            printf("wedges = %lld\n", (long long) wedges);
            printf("transitivity = %.17g\n", wedges ? (double) (3 * triangles) / (double) wedges : 0.0);
            printf("avg_clustering = %.17g\n", V ? sum / (double) V : 0.0);
            printf("top = %lld\n", (long long) top);
            return true;
        });
    return app.exec(argc, argv);
}
