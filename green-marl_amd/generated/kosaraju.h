// kosaraju.h -- entry point with the signature gm_comp emits for apps/src/kosaraju.gm
// (call site /root/reference/apps/output_cpp/src/kosaraju_main.cc:26; N_P<Int> -> int32_t*, Int return -> int32_t).
// G_mem[v] receives the component of v.  The partition and the returned count are the reference's; the component ids
// are canonical (dense 0 .. count-1 in increasing order of each component's smallest vertex id) rather than the
// reference's DFS finish order, which is inherently sequential (see gmx_scc in gmx.h).
#ifndef GM_GENERATED_CPP_KOSARAJU_H
#define GM_GENERATED_CPP_KOSARAJU_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int32_t kosaraju(gm_graph& G, int32_t* G_mem);

#endif
