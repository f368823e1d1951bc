// graphlets.h -- the 4-node graphlet census as a procedure in the generated style: what gm_comp would emit for
//   Procedure graphlets(G: Graph, gdv: N_P<Long>[15], totals: Long[9])
// (the node property is row-major by node id, fifteen int64 a node).  The reference has no such program: with the stored slots
// read as an undirected simple graph (gmx_graphlets in gmx.h), G_gdv[v * 15 + k] is the number of induced connected subgraphs
// on 2, 3 and 4 vertices in which v sits at orbit k (ORCA's numbering) and totals[j] the number of induced graphlets G0 .. G8.
// G_gdv may be NULL: only the totals are computed.
#ifndef GM_GENERATED_CPP_GRAPHLETS_H
#define GM_GENERATED_CPP_GRAPHLETS_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

void graphlets(gm_graph& G, int64_t* G_gdv, int64_t* totals);

#endif
