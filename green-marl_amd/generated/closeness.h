// closeness.h -- distance centralities as procedures in the generated style: what gm_comp would emit for
//   Procedure closeness(G: Graph, mode: Int, closeness: N_P<Double>, harmonic: N_P<Double>, ecc: N_P<Int>)
//   Procedure closeness(G: Graph, mode: Int, Pivots: Node_Seq, closeness: N_P<Double>, harmonic: N_P<Double>, ecc: N_P<Int>)
// (N_P<Double> -> double*, N_P<Int> -> int32_t*, Node_Seq -> gm_node_seq&).  The reference has no such program.  mode is
// GMX_CLOSE_OUT (distances from v along out-edges), GMX_CLOSE_IN (distances to v) or GMX_CLOSE_BOTH (slots as undirected
// edges).  Over the sources s -- every vertex, or the pivots, a repeated pivot counting again -- at hop distance
// 0 < D(v, s) < infinity:  G_closeness[v] = reach / sum of D (0 when nothing is reached), G_harmonic[v] = sum of 1 / D (from
// below by less than reach * 2^-32: gmx_closeness's fixed point over 2^32) and G_ecc[v] = max of D.  Any of the three
// arrays may be NULL.  The device returns exact integers (gmx_closeness in gmx.h); the doubles are derived here.
#ifndef GM_GENERATED_CPP_CLOSENESS_H
#define GM_GENERATED_CPP_CLOSENESS_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <vector>
#include <omp.h>
#include "gm.h"

void closeness(gm_graph& G, int mode, double* G_closeness, double* G_harmonic, int32_t* G_ecc);
void closeness(gm_graph& G, int mode, gm_node_seq& Pivots, double* G_closeness, double* G_harmonic, int32_t* G_ecc);
void closeness(gm_graph& G, int mode, const std::vector<node_t>& pivots, double* G_closeness, double* G_harmonic, int32_t* G_ecc);

#endif
