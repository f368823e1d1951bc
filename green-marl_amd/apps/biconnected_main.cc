// biconnected_main.cc -- bridges, articulation points and biconnected components, driver on the common protocol:
// `<graph> <threads> <nfs>`.  The kernel is the biconnected procedure.  The report is the five lines `num_blocks = <n>`,
// `num_bridges = <undirected edges>`, `num_articulation_points = <n>`, `num_2edge_components = <n>` and
// `largest_block_edges = <distinct undirected edges of the largest block>`.
#include "common_main.h"
#include "biconnected.h"

int main(int argc, char** argv) {
    std::vector<int32_t> block;
    int64_t num_blocks = 0, num_bridges = 0, num_artic = 0, num_tecc = 0;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) {
            block.assign((size_t) G.num_edges() + 1, -1);
            return true;
        })
        .kernel([&](gm_graph& G) {
            num_blocks = biconnected(G, NULL, NULL, block.data(), NULL, num_bridges, num_artic, num_tecc);
            return true;
        })
        .report([&](gm_graph& G) {
            // one (block, edge) key per slot; the repeats and the other orientation of an edge fall together
            const int64_t V = (int64_t) G.num_nodes();
            std::vector<std::pair<int32_t, int64_t>> keys;
            for (int64_t u = 0; u < V; u++)
                for (edge_t e = G.begin[u]; e < G.begin[u + 1]; e++) {
                    const int64_t w = (int64_t) G.node_idx[e];
                    if (block[(size_t) e] >= 0) keys.push_back({block[(size_t) e], std::min(u, w) * V + std::max(u, w)});
                }
            std::sort(keys.begin(), keys.end());
            keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
            std::vector<int64_t> size((size_t) num_blocks, 0);
            for (const auto& k : keys) size[(size_t) k.first]++;
            int64_t largest = 0;
            for (int64_t s : size) largest = std::max(largest, s);
            printf("num_blocks = %lld\n", (long long) num_blocks);
            printf("num_bridges = %lld\n", (long long) num_bridges);
            printf("num_articulation_points = %lld\n", (long long) num_artic);
            printf("num_2edge_components = %lld\n", (long long) num_tecc);
            printf("largest_block_edges = %lld\n", (long long) largest);
            return true;
        });
    return app.exec(argc, argv);
}
