// gm_runtime.cc -- thread-count shim and the per-thread random streams (contract: ../inc/gm_runtime.h).
#include "gm_runtime.h"

#include <assert.h>
#include <stddef.h>
#include <vector>

static int g_threads = 0;
static bool g_init = false;
static std::vector<uint64_t> g_rand;   // one 48-bit state per thread

static double rand_draw(uint64_t& x) {
    x = (0x5DEECE66DULL * x + 0xBULL) & ((1ULL << 48) - 1);
    return (double) x / 281474976710656.0;
}
// the states of threads [old, n): seeded with n, then one warm-up draw each
static void rand_expand(int n) {
    const size_t old = g_rand.size();
    if ((size_t) n <= old) return;
    g_rand.resize((size_t) n);
    for (size_t i = old; i < (size_t) n; i++) {
        g_rand[i] = ((uint64_t) ((n >> 16) & 0xFFFF) << 32) | ((uint64_t) (n & 0xFFFF) << 16) | 0x330EULL;
        rand_draw(g_rand[i]);
    }
}

void gm_rt_initialize() {
    if (g_init) return;
    g_init = true;
    if (g_threads <= 0) g_threads = omp_get_max_threads();
}
bool gm_rt_is_initialized() { return g_init; }
int gm_rt_get_num_threads() { return g_threads > 0 ? g_threads : omp_get_max_threads(); }
void gm_rt_set_num_threads(int n) {
    if (n <= 0) return;
    rand_expand(n);
    g_threads = n;
    omp_set_num_threads(n);
}
int gm_rt_thread_id() { return omp_get_thread_num(); }
void gm_rt_cleanup() {}

uint64_t* gm_rt_rand_state(int tid) {
    assert(tid >= 0);
    if ((size_t) tid >= g_rand.size()) rand_expand(tid + 1 > gm_rt_get_num_threads() ? tid + 1 : gm_rt_get_num_threads());
    return &g_rand[(size_t) tid];
}
double gm_rt_uniform(int tid) { return rand_draw(*gm_rt_rand_state(tid)); }
int gm_rt_rand(int min, int max, int tid) {
    const int range = max - min;
    assert(range > 0);
    return (int) (gm_rt_uniform(tid) * range) + min;
}
long gm_rt_rand_long(long max, int tid) { return (long) (gm_rt_uniform(tid) * max); }
