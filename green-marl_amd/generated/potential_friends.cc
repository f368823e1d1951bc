// potential_friends.cc -- body of the generated `potential_friends` procedure, MI355X build.
// Emitted prologue: gm_rt_initialize(); G.freeze();   The sets come from the device (gmx_potential_friends) over vertex
// ranges: one sizing call over all vertices gives every set's size, the ranges are then cut so that a range's host
// buffer stays under POTENTIAL_FRIENDS_RANGE_BYTES (a set above the bound is a range of its own), and every range is
// filled by one call and handed to the sets with assign_sorted.
#include <vector>
#include "potential_friends.h"
#include "gmx.h"

#define POTENTIAL_FRIENDS_RANGE_BYTES (256ll << 20)

static void potential_friends_fail() {
    fprintf(stderr, "potential_friends: %s\n", gmx_last_error());
    abort();
}

void potential_friends(gm_graph& G, gm_property_of_collection<gm_node_set>& G_potFriend) {
    gm_rt_initialize();
    G.freeze();
    gmx_graph_t* dev = G.device_mirror();
    const node_t V = G.num_nodes();
    std::vector<int64_t> begin((size_t) V + 1, 0), part;
    if (dev == NULL || gmx_potential_friends(dev, 0, V, begin.data(), NULL, 0, NULL, NULL) != GMX_OK) potential_friends_fail();
    const int64_t bound = POTENTIAL_FRIENDS_RANGE_BYTES / (int64_t) sizeof(node_t);
    std::vector<node_t> items;
    for (node_t lo = 0; lo < V;) {
        node_t hi = lo + 1;
        while (hi < V && begin[(size_t) hi + 1] - begin[(size_t) lo] <= bound) hi++;
        const int64_t want = begin[(size_t) hi] - begin[(size_t) lo];
        int64_t total = 0;
        items.resize((size_t) std::max<int64_t>(want, 1));
        part.assign((size_t) (hi - lo) + 1, 0);
        if (gmx_potential_friends(dev, lo, hi, part.data(), items.data(), want, &total, NULL) != GMX_OK) potential_friends_fail();
        if (total != want) {
            fprintf(stderr, "potential_friends: range [%d, %d) holds %lld items, sized as %lld\n", (int) lo, (int) hi, (long long) total, (long long) want);
            abort();
        }
        #pragma omp parallel for schedule(dynamic, 1024)
        for (node_t v = lo; v < hi; v++)
            G_potFriend[v].assign_sorted(items.data() + part[(size_t) (v - lo)], (size_t) (part[(size_t) (v - lo) + 1] - part[(size_t) (v - lo)]));
        lo = hi;
    }
    gm_rt_cleanup();
}
