// adamicAdar.h -- signature of the generated `adamicAdar` procedure (apps/src/adamicAdar.gm).
#ifndef GM_GENERATED_CPP_ADAMICADAR_H
#define GM_GENERATED_CPP_ADAMICADAR_H

#include "gm.h"

void adamicAdar(gm_graph& G, double* G_aa);

#endif
