// wcc.h -- weakly connected components as a procedure in the generated style: what gm_comp would emit for
//   Procedure wcc(G: Graph, comp: N_P<Node>) : Int
// (N_P<Node> -> node_t*, Int return -> int32_t).  The reference has no such program; the result follows kosaraju's
// conventions here: G_comp[v] receives the component of v, ids dense over 0 .. count-1 in increasing order of each
// component's smallest vertex id, and the count is returned (see gmx_wcc in gmx.h).
#ifndef GM_GENERATED_CPP_WCC_H
#define GM_GENERATED_CPP_WCC_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int32_t wcc(gm_graph& G, node_t* G_comp);

#endif
