// louvain.h -- Louvain modularity communities as a procedure in the generated style: what gm_comp would emit for
//   Procedure louvain(G: Graph, weight: E_P<Int>, comm: N_P<Node>) : Double
// (E_P<Int> -> int32_t* by forward edge slot, N_P<Node> -> node_t* by node id, Double return -> double).  The reference has no
// such program: every edge slot u -> w is an undirected edge of weight G_weight[slot] >= 1 (NULL: every weight is 1), the
// levels and half-rounds of gmx_louvain in gmx.h run with at most 32 levels of at most 64 rounds, G_comm[v] receives the
// community of v, numbered by ascending smallest member, and the modularity of that partition is returned.
#ifndef GM_GENERATED_CPP_LOUVAIN_H
#define GM_GENERATED_CPP_LOUVAIN_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

double louvain(gm_graph& G, int32_t* G_weight, node_t* G_comm);

#endif
