// ktruss.h -- k-truss decomposition and per-edge triangle support as a procedure in the generated style: what gm_comp would
// emit for
//   Procedure ktruss(G: Graph, truss: E_P<Int>, support: E_P<Int>) : Int
// (E_P<Int> -> int32_t* by forward edge slot, Int -> int32_t).  The reference has no such program: with the stored slots read
// as an undirected simple graph (gmx_ktruss in gmx.h), G_support[e] is the number of triangles through the slot's edge and
// G_truss[e] the largest k such that the edge lies in a subgraph whose every edge is in at least k - 2 triangles of that
// subgraph (at least 2; 0 at a self loop).  The largest truss number is returned.  Either array may be NULL; without
// G_truss nothing is peeled and 0 is returned.
#ifndef GM_GENERATED_CPP_KTRUSS_H
#define GM_GENERATED_CPP_KTRUSS_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int32_t ktruss(gm_graph& G, int32_t* G_truss, int32_t* G_support);

#endif
