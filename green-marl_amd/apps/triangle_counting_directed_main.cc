// triangle_counting_directed_main.cc -- driver of triangle_counting_directed.  The reference ships none for this
// application; the output line follows the undirected driver's (`number of triangles:`), with the full 64-bit count.
#include "common_main.h"
#include "triangle_counting_directed.h"

int main(int argc, char** argv) {
    int64_t triangles = 0;
    gm_app app;
    app.kernel([&](gm_graph& G) { triangles = triangle_counting_directed(G); return true; })
        .report([&](gm_graph&) {
            printf("number of triangles: %lld\n", (long long) triangles);
            return true;
        });
    return app.exec(argc, argv);
}
