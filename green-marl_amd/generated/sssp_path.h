// sssp_path.h -- entry points with the signatures gm_comp emits for apps/src/sssp_path.gm
// (call sites /root/reference/apps/output_cpp/src/sssp_path_main.cc:44-46; N_P<Int> / E_P<Int> -> int32_t*, N_P<Node> -> node_t*,
// Node in-arg -> node_t&, Node_Seq -> gm_node_seq&).
#ifndef GM_GENERATED_CPP_SSSP_PATH_H
#define GM_GENERATED_CPP_SSSP_PATH_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

void sssp_path(gm_graph& G, int32_t* G_dist,
    int32_t* G_len, node_t& root,
    node_t* G_prev);
void get_path(gm_graph& G, node_t& begin,
    node_t& end, node_t* G_prev,
    gm_node_seq& Q);

#endif
