// random_bipartite_matching_main.cc -- maximal bipartite matching driver.  The reference ships no driver for
// apps/src/random_bipartite_matching.gm: this one is this tree's own, on the command line of the others.  Any graph is
// made a valid input by running on its bipartite double cover H: 2 V vertices, v < V is left and keeps G's row v with every
// target shifted by + V, the vertices V .. 2 V - 1 are right and have no out-edges.  No edge is dropped.
#include "common_main.h"
#include "random_bipartite_matching.h"

int main(int argc, char** argv) {
    gm_graph H;
    bool* is_left = NULL;
    node_t* match = NULL;
    int count = 0;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) {
            const node_t V = G.num_nodes();
            for (node_t v = 0; v < 2 * (int64_t) V; v++) H.add_node();
            for (node_t v = 0; v < V; v++)
                for (edge_t e = G.begin[v]; e < G.begin[v + 1]; e++) H.add_edge(v, G.node_idx[e] + V);
            H.freeze();
            is_left = new bool[2 * (size_t) V + 1];
            match = new node_t[2 * (size_t) V + 1];
            for (size_t v = 0; v < 2 * (size_t) V; v++) is_left[v] = v < (size_t) V;
            return true;
        })
        .kernel([&](gm_graph&) { count = random_bipartite_matching(H, is_left, match); return true; })
        .report([&](gm_graph&) {
            printf("matching size = %d\n", count);
            return true;
        });
    const int rc = app.exec(argc, argv);
    delete[] is_left;
    delete[] match;
    return rc;
}
