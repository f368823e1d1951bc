// bc_random_main.cc -- estimated-betweenness-centrality benchmark driver; command line and output of the reference's
// apps/output_cpp/src/bc_random_main.cc (K = 10 random sources :23, BC[0..3] printed with %0.9lf :28-31).
// The reference's process reaches bc_random with the C library's unseeded rand() stream untouched, and G.PickRandom() draws
// the sources from it.  Here the device runtime has drawn from that process-wide stream while the graph was loaded (see
// sssp_path_main.cc), so the driver puts the stream back to its start -- srand(1) is the unseeded state -- before the call.
#include "common_main.h"
#include "bc_random.h"

int main(int argc, char** argv) {
    std::vector<float> BC;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) { BC.assign((size_t) G.num_nodes(), 0.0f); return true; })
        .kernel([&](gm_graph& G) {
            srand(1);
            bc_random(G, BC.data(), 10);
            return true;
        })
        .report([&](gm_graph& G) {
            for (node_t v = 0; v < 4 && v < G.num_nodes(); v++) printf("BC[%d] = %0.9lf\n", (int) v, (double) BC[v]);
            return true;
        });
    return app.exec(argc, argv);
}
