// adamicAdar_main.cc -- Adamic-Adar edge score driver; command line and output of the reference's
// apps/output_cpp/src/adamicAdar_main.cc: the edge property is the app's, run() is the adamicAdar call, and the report is
// the first 101 nonzero entries as `<slot>-> <value>`.
#include "common_main.h"
#include "adamicAdar.h"

int main(int argc, char** argv) {
    std::vector<double> aa;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) { aa.assign((size_t) G.num_edges(), 0.0); return true; })
        .kernel([&](gm_graph& G) { adamicAdar(G, aa.data()); return true; })
        .report([&](gm_graph& G) {
            int max_cnt = 0;
            for (edge_t i = 0; i < G.num_edges(); i++) {
                if (aa[i] != 0) {
                    printf("%d-> %5.5f\n", (int) i, aa[i]);
                    if (max_cnt++ == 100) break;
                }
            }
            return true;
        });
    return app.exec(argc, argv);
}
