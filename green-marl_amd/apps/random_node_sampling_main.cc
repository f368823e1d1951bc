// random_node_sampling_main.cc -- driver of random_node_sampling on the command line of the others.  The reference's passes a
// libc rand() vertex id as N; this one takes N as an argument (default 16).
#include "common_main.h"
#include "random_node_sampling.h"

int main(int argc, char** argv) {
    int32_t N = 16;
    gm_node_set* set = NULL;
    gm_app app;
    app.usage("[N=16]")
        .args([&](const std::vector<std::string>& a) {
            if (a.size() > 0) N = atoi(a[0].c_str());
            return true;
        })
        .setup([&](gm_graph& G) { set = new gm_node_set(G.num_nodes()); return true; })
        .kernel([&](gm_graph& G) { random_node_sampling(G, N, *set); return true; })
        .report([&](gm_graph&) {
            printf("selected = %lld, rounds = 1\n", (long long) set->get_size());
            printf("set size = %lld\n", (long long) set->get_size());
            return true;
        });
    const int rc = app.exec(argc, argv);
    delete set;
    return rc;
}
