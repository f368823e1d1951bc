// squares_main.cc -- 4-cycle (square) counting driver on the common protocol: `<graph> <threads> <nfs>`.  The kernel is
// gmx_squares on the graph's device mirror (the squares procedure's call, with the statistics).  The report is the three
// lines `squares = <squares of the graph>`, `max_count = <the largest number of them through one vertex>` and
// `top = <the lowest vertex id with that count>`.
#include "common_main.h"
#include "squares.h"
#include "gmx.h"

int main(int argc, char** argv) {
    std::vector<int64_t> count;
    int64_t squares = 0;
    gmx_stats_t st;
    gm_app app;
    app.setup([&](gm_graph& G) {
            count.assign((size_t) G.num_nodes() + 1, 0);
            return true;
        })
        .kernel([&](gm_graph& G) {
            G.freeze();
            gmx_graph_t* dev = G.device_mirror();
            if (dev == NULL || gmx_squares(dev, count.data(), &squares, &st) != GMX_OK) {
                fprintf(stderr, "squares: %s\n", gmx_last_error());
                return false;
            }
            return true;
        })
        .report([&](gm_graph& G) {
            const int64_t V = (int64_t) G.num_nodes();
            int64_t top = 0;
            for (int64_t v = 1; v < V; v++)
                if (count[(size_t) v] > count[(size_t) top]) top = v;
            printf("squares = %lld\n", (long long) squares);
            printf("max_count = %lld\n", (long long) (V ? count[(size_t) top] : 0));
            printf("top = %lld\n", (long long) top);
            return true;
        });
    return app.exec(argc, argv);
}
