// msf.h -- the minimum spanning forest as a procedure in the generated style: what gm_comp would emit for
//   Procedure msf(G: Graph, weight: E_P<Int>, in_forest: E_P<Bool>) : Long
// (E_P<Int> -> int32_t*, E_P<Bool> -> bool*, Long return -> int64_t).  The reference has no such program: every edge slot
// u -> w with u != w is an undirected edge of weight G_weight[slot], the edges are ordered by (weight, slot), G_in_forest[slot]
// receives whether Kruskal's algorithm selects the slot in that order (gmx_msf in gmx.h), and the forest's weight is returned.
#ifndef GM_GENERATED_CPP_MSF_H
#define GM_GENERATED_CPP_MSF_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int64_t msf(gm_graph& G, int32_t* G_weight, bool* G_in_forest);

#endif
