// pick_random_check.cc -- gm_graph::pick_random_node() is one libc rand() draw modulo the vertex count: prints ten picks on
// a 256-vertex graph after srand(1) (tests/test_bc_random_host.py draws the same ten through libc itself).
#include <stdio.h>
#include <stdlib.h>
#include "gm.h"

int main() {
    gm_graph G;
    for (int i = 0; i < 256; i++) G.add_node();
    if (G.num_nodes() != 256) return 1;
    srand(1);
    for (int i = 0; i < 10; i++) printf("%d ", (int) G.pick_random_node());
    printf("\n");
    return 0;
}
