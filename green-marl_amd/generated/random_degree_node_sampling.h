// random_degree_node_sampling.h -- signature of the gm_comp-generated header for apps/src/random_degree_node_sampling.gm
#ifndef GM_GENERATED_CPP_RANDOM_DEGREE_NODE_SAMPLING_H
#define GM_GENERATED_CPP_RANDOM_DEGREE_NODE_SAMPLING_H
#include "gm.h"

void random_degree_node_sampling(gm_graph& G, int32_t N, gm_node_set& S);

#endif
