// sampling_check.cc -- the host side of the sampling programs, printed for tests/test_sampling_host.py:
//   sampling_check streams <n>            gm_rt_set_num_threads(n): every thread's state, then five draws of thread 0 and its state
//   sampling_check walk <ring64|star64> <N> <c>
//                                         set_num_threads(1); three pick_random_out_neighbor(0), then the single-walker drop-in:
//                                         the picks, the members of S and the state of thread 0
//   sampling_check dropin <ring64|star64> <p_size> <p_jump> <tokens> <N>      (needs a GPU)
//                                         the three device drop-ins one after the other on thread 0's stream: the selected
//                                         vertices of each and the state behind it
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gm.h"
#include "random_walk_sampling_with_random_jump.h"
#include "parallel_random_walk_jump_sampling.h"
#include "random_node_sampling.h"
#include "random_degree_node_sampling.h"

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "streams")) {
        const int n = atoi(argv[2]);
        gm_rt_set_num_threads(n);
        for (int t = 0; t < n; t++) printf("state %d %012llx\n", t, (unsigned long long) *gm_rt_rand_state(t));
        for (int i = 0; i < 5; i++) printf("draw %a\n", gm_rt_uniform(0));
        printf("after %012llx\n", (unsigned long long) *gm_rt_rand_state(0));
        const int r = gm_rt_rand(10, 20, 0);   // (two statements: the order of evaluation of arguments is not fixed)
        const long rl = gm_rt_rand_long(1000000L, 0);
        printf("rand %d %ld\n", r, rl);
        printf("end %012llx\n", (unsigned long long) *gm_rt_rand_state(0));
        return 0;
    }
    const bool dropin = argc >= 7 && !strcmp(argv[1], "dropin");
    if (dropin || (argc >= 5 && !strcmp(argv[1], "walk"))) {
        gm_graph G;
        for (int i = 0; i < 64; i++) G.add_node();
        if (!strcmp(argv[2], "ring64")) {
            for (int v = 0; v < 64; v++) G.add_edge(v, (v + 1) % 64);
        } else {
            for (int t = 1; t < 48; t++) G.add_edge(0, t);
            for (int v = 1; v < 48; v++) G.add_edge(v, 0);
        }
        G.freeze();
        gm_rt_set_num_threads(1);
        if (dropin) {
            bool* sel = new bool[64];
            parallel_random_walk_jump_sampling(G, (float) atof(argv[3]), (float) atof(argv[4]), atoi(argv[5]), sel);
            printf("walk");
            for (int v = 0; v < 64; v++)
                if (sel[v]) printf(" %d", v);
            printf("\nstate %012llx\n", (unsigned long long) *gm_rt_rand_state(0));
            delete[] sel;
            for (int mode = 0; mode < 2; mode++) {
                gm_node_set S(G.num_nodes());
                if (mode) random_degree_node_sampling(G, atoi(argv[6]), S); else random_node_sampling(G, atoi(argv[6]), S);
                printf("nodes%d", mode);
                gm_node_set::seq_iter it = S.prepare_seq_iteration();
                while (it.has_next()) printf(" %d", (int) it.get_next());
                printf("\nstate %012llx\n", (unsigned long long) *gm_rt_rand_state(0));
            }
            return 0;
        }
        printf("picks");
        for (int i = 0; i < 3; i++) printf(" %d", (int) G.pick_random_out_neighbor(0));
        printf("\n");
        gm_node_set S(G.num_nodes());
        random_walk_sampling_with_random_jump(G, atoi(argv[3]), atof(argv[4]), S);
        printf("members");
        gm_node_set::seq_iter it = S.prepare_seq_iteration();
        while (it.has_next()) printf(" %d", (int) it.get_next());
        printf("\nstate %012llx\n", (unsigned long long) *gm_rt_rand_state(0));
        return 0;
    }
    return 2;
}
