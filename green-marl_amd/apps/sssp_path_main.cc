// sssp_path_main.cc -- shortest path between two vertices; inputs and output of
// /root/reference/apps/output_cpp/src/sssp_path_main.cc (edge lengths (rand % 100) + 1 drawn from gm_rand32 in slot order :33-35;
// root = rand() % N, then end = rand() % N, from the C library's unseeded rand() :40-42; `shortest path from <root> to <end>`
// and the path `a -> b -> ... -> z` on one line, no path line when end was not reached :51-61).
// The two values come from a private copy of that generator (glibc's random_r from seed 1 is the stream of an unseeded
// rand()): the process-wide rand() state is shared with every library in the process, and the device runtime draws from it.
#include "common_main.h"
#include "sssp_path.h"
#include "gm_rand.h"

int main(int argc, char** argv) {
    node_t root = 0, end = 0;
    std::vector<int32_t> length, dist;
    std::vector<node_t> prev;
    gm_node_seq Q;
    struct random_data unseeded;
    char unseeded_state[128];
    memset(&unseeded, 0, sizeof(unseeded));
    initstate_r(1, unseeded_state, sizeof(unseeded_state), &unseeded);
    gm_app app;
    app.setup([&](gm_graph& G) {
            gm_rand32 rng;
            dist.assign((size_t) G.num_nodes(), 0);
            prev.assign((size_t) G.num_nodes(), (node_t) gm_graph::NIL_NODE);
            length.resize((size_t) G.num_edges());
            for (int32_t& l : length) l = (rng.rand() % 100) + 1;   // 1 .. 100
            return true;
        })
        .kernel([&](gm_graph& G) {
            int32_t r0 = 0, r1 = 0;
            random_r(&unseeded, &r0);
            random_r(&unseeded, &r1);
            root = r0 % G.num_nodes();
            end = r1 % G.num_nodes();
            sssp_path(G, dist.data(), length.data(), root, prev.data());
            get_path(G, root, end, prev.data(), Q);
            return true;
        })
        .report([&](gm_graph&) {
            printf("shortest path from %d to %d\n", (int) root, (int) end);
            gm_node_seq::seq_iter it = Q.prepare_seq_iteration();
            while (it.has_next()) {
                const node_t n = it.get_next();
                printf("%d%s", (int) n, it.has_next() ? " -> " : "\n");
            }
            return true;
        });
    return app.exec(argc, argv);
}
