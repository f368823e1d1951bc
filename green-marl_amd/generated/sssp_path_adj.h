// sssp_path_adj.h -- entry points with the signatures gm_comp emits for apps/src/sssp_path_adj.gm (call sites
// apps/output_cpp/src/sssp_path_adj_main.cc:107-109; N_P<Double> / E_P<Double> -> double*, N_P<Node> -> node_t*,
// N_P<Edge> -> edge_t*, Node in-arg -> node_t&, Node_Seq -> gm_node_seq&).  Both are overloads of the names in sssp_path.h.
#ifndef GM_GENERATED_CPP_SSSP_PATH_ADJ_H
#define GM_GENERATED_CPP_SSSP_PATH_ADJ_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

void sssp_path(gm_graph& G, double* G_dist,
    double* G_edge_cost, node_t& root,
    node_t& end, node_t* G_prev_node,
    edge_t* G_prev_edge);
double get_path(gm_graph& G, node_t& begin,
    node_t& end, node_t* G_prev_node,
    edge_t* G_prev_edge, double* G_edge_cost,
    gm_node_seq& Q);

#endif
