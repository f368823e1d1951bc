// communities.h -- entry point with the signature gm_comp emits for apps/src/communities.gm
// (call site apps/output_cpp/src/communities_main.cc:19 of the reference; N_P<Node> -> node_t*).
// G_Comm[v] receives the community label of v: a vertex id.  Tie rule, vertices without out-edges and the schedule are
// canonical (see gmx_communities in gmx.h); the result is a fixpoint of the reference's rule unless the round bound cut it.
#ifndef GM_GENERATED_CPP_COMMUNITIES_H
#define GM_GENERATED_CPP_COMMUNITIES_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

void communities(gm_graph& G, node_t* G_Comm);

#endif
