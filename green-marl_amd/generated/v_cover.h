// v_cover.h -- signature of the generated `v_cover` procedure (apps/src/v_cover.gm).
#ifndef GM_GENERATED_CPP_V_COVER_H
#define GM_GENERATED_CPP_V_COVER_H

#include "gm.h"

int32_t v_cover(gm_graph& G, bool* G_select);

#endif
