/*
 * pawsome_refine.h — the ranges the pruned strips of the rolling-accumulator kernels run.  The bounding pre-pass works in two
 * stages: the first keeps, per 64-column strip, a range of 8-row blocks from one inequality per block (what
 * pdog_get_prune_counts counts); the second narrows each such range, possibly to nothing, with a bound per 8 x 8 output cell
 * (pdog_set_tuning "no_refine" pins it off).  Positions and exact mode's decisions are unchanged by construction either way.
 * Part of the C ABI of pawsome_dog.h, which includes this file at its end (include that one).
 */
#ifndef PAWSOME_REFINE_H
#define PAWSOME_REFINE_H

#include "pawsome_dog.h" /* types and status codes (it includes this file at its end) */

#ifdef __cplusplus
extern "C" {
#endif

/* TEST HOOK, not part of the stable ABI: it may change or go without a change of pdog_abi_version, and a host has no use for
 * it.  The strips that the LAST batch which ran the bounding pass left to compute, to HOST memory: *count receives their
 * number and h_out the first min(*count, capacity) of them as four int32 each — window, strip, first 8-row block, one past
 * the last block — in the order the pre-pass filed them, which differs from run to run.  It reads what the pre-pass wrote
 * for the strips; nothing is recorded for it.  PDOG_E_ARG when no batch of the tracker ran the bounding pass.  Drains the
 * stream. */
int pdog_get_prune_jobs(pdog_tracker *t, int capacity, int32_t *h_out, int *count);

#ifdef __cplusplus
}
#endif

#endif /* PAWSOME_REFINE_H */
