// kosaraju_main.cc -- strongly connected components benchmark driver; command line and output of the reference's
// apps/output_cpp/src/kosaraju_main.cc: the membership array is the app's, run() is the kosaraju call, and the report is
// the one line `num_membership = <count>`.
#include "common_main.h"
#include "kosaraju.h"

int main(int argc, char** argv) {
    std::vector<int32_t> membership;
    int32_t num_membership = 0;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) { membership.assign((size_t) G.num_nodes(), 0); num_membership = 0; return true; })
        .kernel([&](gm_graph& G) { num_membership = kosaraju(G, membership.data()); return true; })
        .report([&](gm_graph& G) {
            printf("num_membership = %d\n", (int) num_membership);
            return true;
        });
    return app.exec(argc, argv);
}
