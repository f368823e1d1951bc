// squares.h -- 4-cycle (square) counting as a procedure in the generated style: what gm_comp would emit for
//   Procedure squares(G: Graph, cnt: N_P<Long>) : Long
// (N_P<Long> -> int64_t* by node id, Long -> int64_t).  The reference has no such program: with the stored slots read as an
// undirected simple graph (gmx_squares in gmx.h), the number of cycles a - b - c - d - a on four distinct vertices is returned
// (chords allowed; the butterflies of a bipartite graph), and G_cnt[v] is the number of them through v.  G_cnt may be NULL:
// only the total is computed.
#ifndef GM_GENERATED_CPP_SQUARES_H
#define GM_GENERATED_CPP_SQUARES_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int64_t squares(gm_graph& G, int64_t* G_cnt);

#endif
