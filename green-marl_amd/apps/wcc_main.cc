// wcc_main.cc -- weakly connected components driver on the common protocol: the component array is the app's, run() is
// the wcc call, and the report is the two lines `num_components = <count>` and `largest_component = <vertices>`.
#include "common_main.h"
#include "wcc.h"

int main(int argc, char** argv) {
    std::vector<node_t> comp;
    int32_t num_components = 0;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) { comp.assign((size_t) G.num_nodes(), 0); num_components = 0; return true; })
        .kernel([&](gm_graph& G) { num_components = wcc(G, comp.data()); return true; })
        .report([&](gm_graph& G) {
            std::vector<int64_t> size((size_t) num_components, 0);
            for (node_t c : comp) size[(size_t) c]++;
            int64_t largest = 0;
            for (int64_t s : size) largest = std::max(largest, s);
            printf("num_components = %d\n", (int) num_components);
            printf("largest_component = %lld\n", (long long) largest);
            return true;
        });
    return app.exec(argc, argv);
}
