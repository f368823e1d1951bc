// gm_runtime.h -- the slice of the reference's runtime API the drivers and generated entries call
// (/root/reference/apps/output_cpp/gm_graph/inc/gm_runtime.h:50-60): a thread-count holder and the per-thread random streams.
// On the GPU build the count only sizes the host-side OpenMP loops of gm_graph; kernels run on the device.
//
// The streams (gm_runtime.cc:60-123 of the reference): thread t owns a 48-bit state x; a draw is
// x = (0x5DEECE66D x + 0xB) mod 2^48 and yields x / 2^48, which is what erand48 returns.  The first
// gm_rt_set_num_threads(n) (and every later one that raises the count, for the new threads) seeds a state with the shorts
// {0x330E, n & 0xFFFF, n >> 16} and draws once: for n = 1 that is 0x00000001330E advanced to 0x0AA849495101.  The sampling
// entries of the device library continue thread 0's stream through gm_rt_rand_state(0) (include/gmx.h: the stream).
#ifndef GM_RUNTIME_H_
#define GM_RUNTIME_H_
#include <omp.h>
#include <stdint.h>

void gm_rt_initialize();
bool gm_rt_is_initialized();
int gm_rt_get_num_threads();
void gm_rt_set_num_threads(int n);
int gm_rt_thread_id();
void gm_rt_cleanup();
double gm_rt_uniform(int tid = 0);                  // one draw of thread tid's stream, in [0, 1)
int gm_rt_rand(int min, int max, int tid = 0);      // (int) (uniform * (max - min)) + min
long gm_rt_rand_long(long max, int tid = 0);        // (long) (uniform * max)
uint64_t* gm_rt_rand_state(int tid = 0);            // this tree's addition: the 48-bit state itself, for the device entries

#endif
