// pawsome_exclusive.hip — host side of the exclusive step and walk (include/pawsome_exclusive.h): the assignment kernel
// (dog_assign.hpp), its geometry and its init kernel; the walk's checks, scratch, staged table and loop are pdog_walk.hpp's.
// No kernel of the tracker is named here; what these calls keep on a tracker is the GroupWalkState that pawsome_dog.hip
// hands out (exclusive_state).
#include "../../include/pawsome_exclusive.h"
#include "pdog_walk.hpp"
#include "dog_assign.hpp"

using pdog::fail;
using namespace pdog::exclusive;
static_assert(kMaxTargets == PDOG_EXCLUSIVE_MAX_TARGETS, "a group is half a wave, as the header says");

namespace {

int launch_assign(hipStream_t stream, const AssignGeo &a, int n_groups)
{
    hipLaunchKernelGGL(dog_assign_kernel, dim3(n_groups), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

} // namespace

extern "C" int pdog_assign_exclusive(pdog_tracker *t, int n_groups, int n_targets, int k, int min_distance, double min_ratio,
                                     const int32_t *d_prev, const int32_t *d_ij, const float *d_peak, const int32_t *d_count,
                                     int32_t *d_out_ij, int32_t *d_out_state)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_assign_exclusive: null tracker");
    if (!d_prev || !d_ij || !d_peak || !d_count || !d_out_ij || !d_out_state) return fail(PDOG_E_ARG, "pdog_assign_exclusive: null pointer");
    if (int rc = pdog::check_exclusive("pdog_assign_exclusive", n_groups, n_targets, k, min_ratio)) return rc;
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    pdog::GroupWalkState *es = pdog::exclusive_state(t);
    hipStream_t stream = nullptr;
    if (int rc = pdog::stream_on_device(t, es, &stream)) return rc;
    AssignGeo a;
    a.prev = d_prev; a.ij = d_ij; a.peak = d_peak; a.count = d_count;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.next = nullptr; a.len = nullptr;
    a.out_stride = 1; a.d = pdog::distance_or_default(min_distance, info);
    a.step = 0; a.T = n_targets; a.k = k; a.rho = (float)min_ratio;
    ++es->steps;
    return launch_assign(stream, a, n_groups);
}

extern "C" int pdog_detect_chains_exclusive(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                            int n_frames, const int32_t *h_table, int n_steps, int n_groups, int n_targets,
                                            int first, int k, int min_distance, double min_ratio, const int32_t *d_start,
                                            int32_t *d_out_ij, int32_t *d_out_state)
{
    const char *who = "pdog_detect_chains_exclusive";
    if (!t) return fail(PDOG_E_ARG, std::string(who) + ": null tracker");
    if (!d_frames || !h_table || !d_start || !d_out_ij || !d_out_state) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    k = pdog::k_or_default(k, n_targets);
    if (int rc = pdog::check_exclusive(who, n_groups, n_targets, k, min_ratio)) return rc;
    pdog::GroupWalkState *es = pdog::exclusive_state(t);
    pdog::GroupWalk w{d_frames, frame_stride, row_stride, n_frames, h_table, n_steps, n_groups, n_targets, first, k, min_distance};
    if (int rc = pdog::begin_group_walk(who, t, es, 2, w)) return rc;
    if (w.max_len == 0) return PDOG_OK; // no group has a step

    int32_t *cur = w.carry; // [n][2] the current guesses
    hipLaunchKernelGGL(dog_assign_init_kernel, dim3((w.n + 255) / 256), dim3(256), 0, w.stream, d_start, w.d_len, cur, d_out_ij, d_out_state, w.n,
                       n_targets, (long long)n_steps, first);
    HIP_TRY(hipGetLastError());
    AssignGeo a;
    a.prev = cur; a.ij = w.picks; a.peak = w.peak; a.count = w.counts;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.next = cur; a.len = w.d_len;
    a.out_stride = n_steps; a.d = w.d;
    a.T = n_targets; a.k = k; a.rho = (float)min_ratio;
    return pdog::walk_groups(t, es, w, cur, [&](int s) { a.step = s; return launch_assign(w.stream, a, n_groups); });
}

extern "C" int pdog_get_exclusive_counts(pdog_tracker *t, uint64_t out[2])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_exclusive_counts: null pointer");
    const pdog::GroupWalkState *es = pdog::exclusive_state(t);
    out[0] = es->steps;
    out[1] = es->grown;
    return PDOG_OK;
}
