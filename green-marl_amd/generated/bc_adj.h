// bc_adj.h -- entry point with the signature gm_comp emits for apps/src/bc_adj.gm:5
//   Procedure comp_BC(G: Graph, BC: N_P<Float>)
// (call site /root/reference/apps/output_cpp/src/bc_adj_main.cc:101).  An overload of bc.h's comp_BC(G, BC, Seeds):
// both headers may be included in one translation unit.
#ifndef GM_GENERATED_CPP_BC_ADJ_H
#define GM_GENERATED_CPP_BC_ADJ_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

void comp_BC(gm_graph& G, float* G_BC);

#endif
