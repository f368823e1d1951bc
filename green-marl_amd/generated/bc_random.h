// bc_random.h -- entry point with the signature gm_comp emits for apps/src/bc_random.gm:4
//   Procedure bc_random(G: Graph, BC: N_P<Float>, K: Int)
// (call site: the reference's apps/output_cpp/src/bc_random_main.cc:23; property -> float*, Int -> int32_t,
// src/backend_cpp/gm_cpp_gen.cc:520-608).
#ifndef GM_GENERATED_CPP_BC_RANDOM_H
#define GM_GENERATED_CPP_BC_RANDOM_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

void bc_random(gm_graph& G, float* G_BC,
    int32_t K);

#endif
