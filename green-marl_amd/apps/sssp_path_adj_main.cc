// sssp_path_adj_main.cc -- route query between two vertices with double edge costs.  The reference's driver
// (apps/output_cpp/src/sssp_path_adj_main.cc) reads an adjacency-list file with costs and edge keys, through the Avro
// loader too, which the host library here does not have: this driver is this tree's own, on the command line of the others,
//     sssp_path_adj <graph_name> <num_threads> <nfspath> <root> <end>
// with costs ((rand() % 100) + 1) / 10.0 drawn from gm_rand32 in slot order, and prints the reference driver's report
// (:114-139) with vertex ids for node keys and the edge slot for the edge key: `PATH NOT FOUND`, or `<root> -> <end>`,
// `    Costs are <total>`, `    Number of links is <n>` and the first 20 links `        <slot>: <from> - <to>`.
#include "common_main.h"
#include "sssp_path_adj.h"
#include "gm_rand.h"

int main(int argc, char** argv) {
    node_t root = 0, end = 0;
    std::vector<double> cost, dist;
    std::vector<node_t> prev_node;
    std::vector<edge_t> prev_edge;
    gm_node_seq Q;
    double total_cost = 0.0;
    gm_app app;
    app.usage(" <root> <end>")
        .args([&](const std::vector<std::string>& a) {
            if (a.size() < 2) return false;
            root = (node_t) atol(a[0].c_str());
            end = (node_t) atol(a[1].c_str());
            return true;
        })
        .setup([&](gm_graph& G) {
            if (root < 0 || root >= G.num_nodes() || end < 0 || end >= G.num_nodes()) {
                printf("root and end must be vertices of [0, %ld)\n", (long) G.num_nodes());
                return false;
            }
            gm_rand32 rng;
            dist.assign((size_t) G.num_nodes(), 0.0);
            prev_node.assign((size_t) G.num_nodes(), (node_t) gm_graph::NIL_NODE);
            prev_edge.assign((size_t) G.num_nodes(), (edge_t) gm_graph::NIL_EDGE);
            cost.resize((size_t) G.num_edges() + 1);
            for (size_t e = 0; e < (size_t) G.num_edges(); e++) cost[e] = ((rng.rand() % 100) + 1) / 10.0;   // 0.1 .. 10.0
            return true;
        })
        .kernel([&](gm_graph& G) {
            sssp_path(G, dist.data(), cost.data(), root, end, prev_node.data(), prev_edge.data());
            total_cost = get_path(G, root, end, prev_node.data(), prev_edge.data(), cost.data(), Q);
            return true;
        })
        .report([&](gm_graph& G) {
            if (Q.get_size() == 0) {
                printf("PATH NOT FOUND\n");
                return true;
            }
            printf("%d -> %d\n", (int) root, (int) end);
            printf("    Costs are %lf\n", total_cost);
            printf("    Number of links is %d\n", Q.get_size());
            gm_node_seq::seq_iter it = Q.prepare_seq_iteration();
            int cutoff = 20;
            node_t from = root;
            while (it.has_next()) {
                const node_t n = it.get_next();
                const edge_t e = prev_edge[(size_t) n];
                if (n != G.node_idx[e]) return false;
                printf("        %ld: %d - %d\n", (long) e, (int) from, (int) n);
                from = n;
                if (--cutoff == 0) break;
            }
            return true;
        });
    return app.exec(argc, argv);
}
