// random_walk_sampling_with_random_jump_main.cc -- driver of the single walker (a host loop: generated/random_walk_sampling_with_random_jump.cc) on the
// command line of the others.  The reference's passes a libc rand() vertex id as N; this one takes N (default 1024) and c.
#include "common_main.h"
#include "random_walk_sampling_with_random_jump.h"

int main(int argc, char** argv) {
    int32_t N = 1024;
    double c = 0.15;
    gm_node_set* set = NULL;
    gm_app app;
    app.usage("[N=1024] [c=0.15]")
        .args([&](const std::vector<std::string>& a) {
            if (a.size() > 0) N = atoi(a[0].c_str());
            if (a.size() > 1) c = atof(a[1].c_str());
            return true;
        })
        .setup([&](gm_graph& G) { set = new gm_node_set(G.num_nodes()); return true; })
        .kernel([&](gm_graph& G) { random_walk_sampling_with_random_jump(G, N, c, *set); return true; })
        .report([&](gm_graph&) {
            printf("selected = %lld, rounds = %d\n", (long long) set->get_size(), N);
            printf("set size = %lld\n", (long long) set->get_size());
            return true;
        });
    const int rc = app.exec(argc, argv);
    delete set;
    return rc;
}
