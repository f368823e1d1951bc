// random_walk_sampling_with_random_jump.h -- signature of the gm_comp-generated header for apps/src/random_walk_sampling_with_random_jump.gm
#ifndef GM_GENERATED_CPP_RANDOM_WALK_SAMPLING_WITH_RANDOM_JUMP_H
#define GM_GENERATED_CPP_RANDOM_WALK_SAMPLING_WITH_RANDOM_JUMP_H
#include "gm.h"

void random_walk_sampling_with_random_jump(gm_graph& G, int32_t N, double c, gm_node_set& S);

#endif
