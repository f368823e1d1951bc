// parallel_random_walk_jump_sampling.h -- signature of the gm_comp-generated header for apps/src/parallel_random_walk_jump_sampling.gm
#ifndef GM_GENERATED_CPP_PARALLEL_RANDOM_WALK_JUMP_SAMPLING_H
#define GM_GENERATED_CPP_PARALLEL_RANDOM_WALK_JUMP_SAMPLING_H
#include "gm.h"

void parallel_random_walk_jump_sampling(gm_graph& G, float p_size, float p_jump, int32_t num_tokens, bool* G_Selected);

#endif
