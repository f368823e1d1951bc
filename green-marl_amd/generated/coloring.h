// coloring.h -- greedy vertex colouring as procedures in the generated style: what gm_comp would emit for
//   Procedure coloring(G: Graph, color: N_P<Int>) : Int
//   Procedure coloring(G: Graph, prio: N_P<Int>, color: N_P<Int>) : Int
// (N_P<Int> -> int32_t*, Int return -> int32_t).  The reference has no such program: G_color[v] receives the first-fit
// colour of v in the order "larger priority first, ties to the lower id" (gmx_coloring in gmx.h), the first form with
// outdeg + indeg as the priority (largest degree first), and the number of colours is returned.  The vertices of colour
// 0 are the greedy maximal independent set of the order.
#ifndef GM_GENERATED_CPP_COLORING_H
#define GM_GENERATED_CPP_COLORING_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int32_t coloring(gm_graph& G, int32_t* G_color);
int32_t coloring(gm_graph& G, int32_t* G_prio, int32_t* G_color);

#endif
