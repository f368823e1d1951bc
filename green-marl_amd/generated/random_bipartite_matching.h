// random_bipartite_matching.h -- signature of the generated `random_bipartite_matching` procedure
// (apps/src/random_bipartite_matching.gm).
#ifndef GM_GENERATED_CPP_RANDOM_BIPARTITE_MATCHING_H
#define GM_GENERATED_CPP_RANDOM_BIPARTITE_MATCHING_H

#include "gm.h"

int32_t random_bipartite_matching(gm_graph& G, bool* G_isLeft, node_t* G_Match);

#endif
