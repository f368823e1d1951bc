// clustering.h -- per-vertex triangle counts and clustering coefficients as a procedure in the generated style: what gm_comp
// would emit for
//   Procedure clustering(G: Graph, tri: N_P<Long>, lcc: N_P<Double>; wedges: Long) : Long
// (N_P<Long> -> int64_t*, N_P<Double> -> double*, Long -> int64_t).  The reference has no such program: with the stored
// slots read as an undirected simple graph (gmx_clustering in gmx.h), G_tri[v] receives the triangles through v, G_lcc[v]
// its local clustering coefficient 2 tri / (deg (deg - 1)) (0 below degree 2), wedges the number of paths of length two,
// and the number of triangles is returned.  G_tri or G_lcc may be NULL.
#ifndef GM_GENERATED_CPP_CLUSTERING_H
#define GM_GENERATED_CPP_CLUSTERING_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int64_t clustering(gm_graph& G, int64_t* G_tri, double* G_lcc, int64_t& wedges);

#endif
