// sssp_dijkstra.h -- entry points with the signatures gm_comp emits for apps/src/sssp_dijkstra.gm (call sites
// apps/output_cpp/src/sssp_dijkstra_main.cc:37-42; E_P<Int> -> int32_t*, N_P<Node> -> node_t*, N_P<Edge> -> edge_t*,
// Node in-arg -> node_t&, Node_Seq -> gm_node_seq&, Bool / Int results).  get_path is the one of bidir_dijkstra.gm too:
// route_get_path.h declares it once for both headers.
#ifndef GM_GENERATED_CPP_SSSP_DIJKSTRA_H
#define GM_GENERATED_CPP_SSSP_DIJKSTRA_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"
#include "route_get_path.h"

bool dijkstra(gm_graph& G, int32_t* G_Len,
    node_t& root, node_t& dest,
    node_t* G_Parent, edge_t* G_ParentEdge);

#endif
