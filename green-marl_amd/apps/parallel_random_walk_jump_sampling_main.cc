// parallel_random_walk_jump_sampling_main.cc -- many-walker random-walk sampling driver.  The reference ships no driver for
// apps/src/parallel_random_walk_jump_sampling.gm: this one is this tree's own, on the command line of the others.  It calls
// the device entry directly, because the generated signature returns neither the count nor the rounds.
#include "common_main.h"
#include "parallel_random_walk_jump_sampling.h"
#include "gmx.h"

int main(int argc, char** argv) {
    float p_size = 0.1f, p_jump = 0.15f;
    int32_t tokens = 1024, max_rounds = INT32_MAX, rounds = 0;
    int64_t count = 0;
    bool* selected = NULL;
    gm_app app;
    app.usage("[p_size=0.1] [p_jump=0.15] [num_tokens=1024] [max_rounds]")
        .args([&](const std::vector<std::string>& a) {
            if (a.size() > 0) p_size = (float) atof(a[0].c_str());
            if (a.size() > 1) p_jump = (float) atof(a[1].c_str());
            if (a.size() > 2) tokens = atoi(a[2].c_str());
            if (a.size() > 3) max_rounds = atoi(a[3].c_str());
            return true;
        })
        .setup([&](gm_graph& G) {
            selected = new bool[(size_t) G.num_nodes() + 1];
            if (tokens > G.num_nodes()) tokens = G.num_nodes();
            return true;
        })
        .kernel([&](gm_graph& G) {
            gmx_graph_t* dev = G.device_mirror();
            gmx_stats_t st;
            if (dev == NULL || gmx_random_walk_sampling(dev, p_size, p_jump, tokens, max_rounds, gm_rt_rand_state(0), (uint8_t*) selected, NULL, &count,
                                                        &rounds, &st) != GMX_OK) {
                fprintf(stderr, "parallel_random_walk_jump_sampling: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            int64_t members = 0;
            for (node_t v = 0; v < G.num_nodes(); v++) members += selected[v] ? 1 : 0;
            printf("selected = %lld, rounds = %d\n", (long long) count, rounds);
            printf("set size = %lld\n", (long long) members);
            return true;
        });
    const int rc = app.exec(argc, argv);
    delete[] selected;
    return rc;
}
