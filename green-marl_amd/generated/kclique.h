// kclique.h -- k-clique counting as a procedure in the generated style: what gm_comp would emit for
//   Procedure kclique(G: Graph, k: Int, cnt: N_P<Long>) : Long
// (N_P<Long> -> int64_t* by node id, Int -> int32_t, Long -> int64_t).  The reference has no such program: with the stored
// slots read as an undirected simple graph (gmx_kclique in gmx.h), the number of k-element vertex sets that are pairwise
// adjacent is returned, 3 <= k <= 8, and G_cnt[v] is the number of those sets that contain v.  G_cnt may be NULL: only the
// total is computed.
#ifndef GM_GENERATED_CPP_KCLIQUE_H
#define GM_GENERATED_CPP_KCLIQUE_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int64_t kclique(gm_graph& G, int32_t k, int64_t* G_cnt);

#endif
