// triangle_counting_directed.h -- entry point with the signature gm_comp emits for apps/src/triangle_counting_directed.gm
// (Procedure triangle_counting_directed(G: Graph): Long; Long return -> int64_t).
#ifndef GM_GENERATED_CPP_TRIANGLE_COUNTING_DIRECTED_H
#define GM_GENERATED_CPP_TRIANGLE_COUNTING_DIRECTED_H

#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <cmath>
#include <algorithm>
#include <omp.h>
#include "gm.h"

int64_t triangle_counting_directed(gm_graph& G);

#endif
