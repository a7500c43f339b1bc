// dog_step.hpp — the bookkeeping kernel between two steps of a walk run as ordinary batches (pawsome_dog.hip: chains of
// several clips; pawsome_clips.hip: clips grouped by fill).  Included by both units: the kernel uses no dynamic LDS, so
// nothing is keyed on its address and a private copy per unit is harmless (pdog_host.hpp, WHERE KERNELS LIVE).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdog {

// After the batches of step k: slot p's answer is filed under out[clip][k] and becomes its next guess.  order = NULL: slot p
// is clip p.  len = NULL: every slot takes part; otherwise a slot whose len[p] steps are done stores nothing and keeps its
// last guess.
static __global__ void dog_step_kernel(const int32_t *__restrict__ order, const int32_t *__restrict__ len, int n_slots, int n_steps,
                                       int k, const int32_t *__restrict__ step, int32_t *__restrict__ guess, int32_t *__restrict__ out)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n_slots || (len && len[p] <= k)) return;
    const int i = step[2 * p], j = step[2 * p + 1];
    const long long o = 2ll * ((long long)(order ? order[p] : p) * n_steps + k);
    out[o] = i;
    out[o + 1] = j;
    guess[2 * p] = i;
    guess[2 * p + 1] = j;
}

} // namespace pdog
