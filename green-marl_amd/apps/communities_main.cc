// communities_main.cc -- label-propagation communities benchmark driver; command line and output of the reference's
// apps/output_cpp/src/communities_main.cc: the label array is the app's, run() is the communities call, and the report is
// the header line followed by the first ten non-empty labels with their sizes.
#include "common_main.h"
#include "communities.h"

int main(int argc, char** argv) {
    std::vector<node_t> comm;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) { comm.assign((size_t) G.num_nodes(), 0); return true; })
        .kernel([&](gm_graph& G) { communities(G, comm.data()); return true; })
        .report([&](gm_graph& G) {
            std::vector<int> size((size_t) G.num_nodes(), 0);
            for (node_t i = 0; i < G.num_nodes(); i++) size[(size_t) comm[i]]++;
            printf("Community\t#Nodes\t\t(showing max 10 entries)\n");
            for (node_t i = 0, shown = 0; shown < 10 && i < G.num_nodes(); i++)
                if (size[(size_t) i] > 0) {
                    printf("%d\t\t%d\n", (int) i, size[(size_t) i]);
                    shown++;
                }
            return true;
        });
    return app.exec(argc, argv);
}
