/*
 * pawsome_prune.h — kept ranges on the batch path of the rolling-accumulator kernels: what the bounding pre-pass left to
 * compute, and the batch's FP32 maxima for tests.  Part of the C ABI of pawsome_dog.h, which includes this file at its end
 * (include that one; the types and status codes are declared there).
 */
#ifndef PAWSOME_PRUNE_H
#define PAWSOME_PRUNE_H

#include "pawsome_dog.h" /* types and status codes (it includes this file at its end) */

#ifdef __cplusplus
extern "C" {
#endif

/* Batches on the rolling-accumulator kernels first bound, per window, which 8-row blocks of which 64-column strips can hold
 * the peak or a near-tie of it, and compute only those (positions and exact mode's decisions are unchanged by construction).
 * out[0] / out[1]: (strip, 8-row sub-chunk) pairs kept by the first-stage hull / present, summed over the batches that ran the bounding pass
 * since the tracker was created (batches that ask for the response map, pdog_set_exact(t, 2), "no_prune" and batches the
 * library found not worth bounding run dense and count nothing).  Drains the stream. */
int pdog_get_prune_counts(pdog_tracker *t, uint64_t out[2]);
/* TEST HOOK, not part of the stable ABI: it may change or go without a change of pdog_abi_version, and a host has no use for
 * it.  The FP32 maximum of each of the n windows of the LAST batch that ran on the tracker's strip kernels (the largest of the
 * window's partial peaks, before exact mode's re-evaluation), to HOST memory: for tests that compare two code paths bit for
 * bit.  PDOG_E_ARG when that batch had another size or ran on another kernel family.  Drains the stream. */
int pdog_get_batch_maxima(pdog_tracker *t, int n, float *h_out);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_PRUNE_H */
