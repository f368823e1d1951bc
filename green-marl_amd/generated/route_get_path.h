// route_get_path.h -- the Int get_path that bidir_dijkstra.gm and sssp_dijkstra.gm both define, word for word the same
// procedure: declared once here so that bidir_dijkstra.h and sssp_dijkstra.h can be included by one program.  It is an
// overload of the get_path of sssp_path.h and of sssp_path_adj.h (Double costs).
#ifndef GM_GENERATED_CPP_ROUTE_GET_PATH_H
#define GM_GENERATED_CPP_ROUTE_GET_PATH_H

#include <stdint.h>
#include "gm.h"

int32_t get_path(gm_graph& G, node_t& begin,
    node_t& end, node_t* G_prev_node,
    edge_t* G_prev_edge, int32_t* G_edge_cost,
    gm_node_seq& Q);

#endif
