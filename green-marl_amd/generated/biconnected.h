// biconnected.h -- bridges, articulation points, biconnected components and 2-edge-connected components as a procedure in
// the generated style: what gm_comp would emit for
//   Procedure biconnected(G: Graph, bridge: E_P<Bool>, artic: N_P<Bool>, block: E_P<Int>, tecc: N_P<Int>;
//                         num_bridges: Long, num_artic: Long, num_tecc: Long) : Long
// (E_P<Bool> -> bool* by forward edge slot, N_P<Bool> -> bool*, E_P<Int> / N_P<Int> -> int32_t*, Long -> int64_t).  The
// reference has no such program: with the stored slots read as an undirected simple graph (gmx_biconnected in gmx.h),
// G_bridge[e] says whether the slot's edge is a bridge, G_artic[v] whether v is an articulation point, G_block[e] names
// the biconnected component of the slot's edge (-1 at a self loop, ids by smallest slot), G_tecc[v] the 2-edge-connected
// component of v (ids by smallest vertex); the three counts come back by reference and the number of blocks is returned.
// Any of the four arrays may be NULL.
#ifndef GM_GENERATED_CPP_BICONNECTED_H
#define GM_GENERATED_CPP_BICONNECTED_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int64_t biconnected(gm_graph& G, bool* G_bridge, bool* G_artic, int32_t* G_block, int32_t* G_tecc, int64_t& num_bridges, int64_t& num_artic,
                    int64_t& num_tecc);

#endif
