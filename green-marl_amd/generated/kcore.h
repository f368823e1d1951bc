// kcore.h -- k-core decomposition as a procedure in the generated style: what gm_comp would emit for
//   Procedure kcore(G: Graph, core: N_P<Int>) : Int
// (N_P<Int> -> int32_t*, Int return -> int32_t).  The reference has no such program: G_core[v] receives the core number of
// v with the in-slots as its degree (GMX_KCORE_IN in gmx.h; on a symmetric graph the k-core number of the undirected
// graph), and the largest core number is returned.
#ifndef GM_GENERATED_CPP_KCORE_H
#define GM_GENERATED_CPP_KCORE_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int32_t kcore(gm_graph& G, int32_t* G_core);

#endif
