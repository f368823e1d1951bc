// v_cover_main.cc -- greedy vertex cover driver; command line and output of the reference's
// apps/output_cpp/src/v_cover_main.cc: the edge property is the app's, run() is the v_cover call, and the report is the
// number of covered vertices (the reference's wording: its parallel arg-max is not deterministic, the device is).
#include "common_main.h"
#include "v_cover.h"

int main(int argc, char** argv) {
    bool* selected = NULL;
    int covered = 0;
    gm_app app;
    app.usage("")
        .setup([&](gm_graph& G) { selected = new bool[(size_t) G.num_edges() + 1]; return true; })
        .kernel([&](gm_graph& G) { covered = v_cover(G, selected); return true; })
        .report([&](gm_graph&) {
            printf("covered (may be non-deterministic) = %d\n", covered);
            return true;
        });
    const int rc = app.exec(argc, argv);
    delete[] selected;
    return rc;
}
