// potential_friends_main.cc -- potential-friends benchmark driver; command line and output of the reference's
// apps/output_cpp/src/potential_friends_main.cc: the property of node sets is created inside run(), which is the
// potential_friends call, and the report is the header line followed, for each of the vertices 0 .. 9 whose
// set is not empty, by `node #v: {a, b, ...}` with at most ten entries and `...` after the tenth.
#include <memory>
#include "common_main.h"
#include "potential_friends.h"

int main(int argc, char** argv) {
    std::unique_ptr<gm_property_of_collection_impl<gm_node_set, false> > coll;
    gm_app app;
    app.usage("")
        .kernel([&](gm_graph& G) {
            coll.reset(new gm_property_of_collection_impl<gm_node_set, false>(G.num_nodes()));
            potential_friends(G, *coll);
            return true;
        })
        .report([&](gm_graph& G) {
            printf("potential friends for the first 10 nodes (max. 10 entries per node shown):\n");
            for (node_t v = 0; v < 10 && v < G.num_nodes(); v++) {
                gm_node_set::seq_iter it = (*coll)[v].prepare_seq_iteration();
                if (!it.has_next()) continue;
                printf("node #%d: {", (int) v);
                for (int shown = 0; it.has_next();) {
                    printf("%d", (int) it.get_next());
                    if (++shown == 10) {
                        printf("...");
                        break;
                    }
                    if (it.has_next()) printf(", ");
                }
                printf("}\n");
            }
            return true;
        });
    return app.exec(argc, argv);
}
