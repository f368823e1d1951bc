// potential_friends.h -- entry point with the signature gm_comp emits for apps/src/potential_friends.gm
// (call site apps/output_cpp/src/potential_friends_main.cc:18 of the reference; N_P<Node_Set> ->
// gm_property_of_collection<gm_node_set>&, gm_cpp_gen.cc:1001).
// G_potFriend[v] receives the out-neighbours of v's out-neighbours that are neither v nor out-neighbours of v (see
// gmx_potential_friends in gmx.h); whatever it held before is replaced.
#ifndef GM_GENERATED_CPP_POTENTIAL_FRIENDS_H
#define GM_GENERATED_CPP_POTENTIAL_FRIENDS_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

void potential_friends(gm_graph& G, gm_property_of_collection<gm_node_set>& G_potFriend);

#endif
