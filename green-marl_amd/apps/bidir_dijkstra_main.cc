// bidir_dijkstra_main.cc -- route queries between pairs of vertices with Int edge weights.  The reference's driver
// (apps/output_cpp/src/bidir_dijkstra_main.cc) reads an adjacency-list file with weights, which the host library here does
// not load: this driver is this tree's own, on the command line of the others,
//     bidir_dijkstra <graph_name> <num_threads> <nfspath> <src> <dst> [<pairs_file> <num_pairs>]
// with weights (rand() % 100) + 1 drawn from gm_rand32 in slot order, as sssp_path_main.cc draws its lengths.  With a
// pairs file (lines `src dst`) the first <num_pairs> lines are answered instead of <src> <dst>.  ONE route object
// (gmx.h, gmx_route_create) serves all pairs: the weights are uploaded once.  Per query it prints the reference driver's
// line (:50-70) with vertex ids for node keys,
//     weight %4d ,hops %3d, time %7.2lf path=v<src>=>v<n1>=>v<n2>=>v<n3>=>      (the first four vertices; hops = vertices)
//     weight   -1 ,hops  -1, time %7.2lf path=NO_PATH_EXISTS
// each behind `TEST [ %2d ] ` in the pairs-file mode.  time is the query in milliseconds.
#include "common_main.h"
#include "bidir_dijkstra.h"
#include "gm_rand.h"
#include "gmx.h"

#include <utility>

static double wall_ms() {
    struct timeval t;
    gettimeofday(&t, NULL);
    return t.tv_sec * 1000.0 + t.tv_usec * 0.001;
}

int main(int argc, char** argv) {
    std::vector<std::pair<node_t, node_t> > pairs;
    std::vector<int32_t> weight;
    std::string pairs_file;
    long num_pairs = 0;
    gm_app app;
    app.usage(" <src> <dst> [<pairs_file> <num_pairs>]")
        .args([&](const std::vector<std::string>& a) {
            if (a.size() != 2 && a.size() != 4) return false;
            pairs.push_back(std::make_pair((node_t) atol(a[0].c_str()), (node_t) atol(a[1].c_str())));
            if (a.size() == 4) {
                pairs_file = a[2];
                num_pairs = atol(a[3].c_str());
            }
            return true;
        })
        .setup([&](gm_graph& G) {
            if (!pairs_file.empty()) {
                FILE* f = fopen(pairs_file.c_str(), "r");
                if (!f) {
                    printf("cannot open %s\n", pairs_file.c_str());
                    return false;
                }
                pairs.clear();
                long s = 0, d = 0;
                while ((long) pairs.size() < num_pairs && fscanf(f, "%ld %ld", &s, &d) == 2) pairs.push_back(std::make_pair((node_t) s, (node_t) d));
                fclose(f);
            }
            for (const std::pair<node_t, node_t>& p : pairs)
                if (p.first < 0 || p.first >= G.num_nodes() || p.second < 0 || p.second >= G.num_nodes()) {
                    printf("src and dst must be vertices of [0, %ld)\n", (long) G.num_nodes());
                    return false;
                }
            gm_rand32 rng;
            weight.resize((size_t) G.num_edges() + 1);
            for (size_t e = 0; e < (size_t) G.num_edges(); e++) weight[e] = (rng.rand() % 100) + 1;   // 1 .. 100
            return true;
        })
        .kernel([&](gm_graph& G) {
            gmx_graph_t* dev = G.device_mirror();
            gmx_route_t* route = NULL;
            if (dev == NULL || gmx_route_create(dev, weight.data(), &route) != GMX_OK) {
                fprintf(stderr, "bidir_dijkstra: %s\n", gmx_last_error());
                return false;
            }
            for (size_t i = 0; i < pairs.size(); i++) {
                gmx_node_t first[3];
                int32_t found = 0;
                int64_t cost = 0, hops = 0;
                const double t0 = wall_ms();
                if (gmx_route_query(route, pairs[i].first, pairs[i].second, &found, &cost, first, NULL, 3, &hops, NULL) != GMX_OK) {
                    fprintf(stderr, "bidir_dijkstra: %s\n", gmx_last_error());
                    gmx_route_free(route);
                    return false;
                }
                const double ms = wall_ms() - t0;
                if (!pairs_file.empty()) printf("TEST [ %2d ] ", (int) i + 1);
                if (!found) {
                    printf("weight %4d ,hops %3d, time %7.2lf path=%s\n", -1, -1, ms, "NO_PATH_EXISTS");
                    continue;
                }
                printf("weight %4d ,hops %3d, time %7.2lf path=v%d=>", (int) cost, (int) hops + 1, ms, (int) pairs[i].first);
                for (int64_t k = 0; k < hops && k < 3; k++) printf("v%d=>", (int) first[k]);
                printf("\n");
            }
            gmx_route_free(route);
            return true;
        });
    return app.exec(argc, argv);
}
