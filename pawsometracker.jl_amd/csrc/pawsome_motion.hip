// pawsome_motion.hip — host side of the motion step and walk (include/pawsome_motion.h): the motion kernel (dog_motion.hpp), its
// geometry and its init kernel; the walk's checks, scratch, staged table and loop are pdog_walk.hpp's, with the windows at the
// predictions.  No kernel of the tracker is named here; what these calls keep on a tracker is the GroupWalkState that
// pawsome_dog.hip hands out (motion_state), and the kernel's switch beside it (motion_lds).
#include "../../include/pawsome_motion.h"
#include "pdog_walk.hpp"
#include "dog_motion.hpp"

using pdog::fail;
using namespace pdog::motion;
static_assert(kMaxTargets == PDOG_MOTION_MAX_TARGETS, "a group is half a wave, as the header says");
static_assert(kLdsWords == PDOG_MOTION_MAX_TARGETS * PDOG_PEAKS_MAX_K, "the LDS image holds every lane's whole list");

namespace {

int launch_motion(hipStream_t stream, const MotionGeo &a, int n_groups, bool lds)
{
    if (lds) hipLaunchKernelGGL(dog_motion_kernel<true>, dim3(n_groups), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(dog_motion_kernel<false>, dim3(n_groups), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

void fill_geo(MotionGeo &a, const pdog_info &info, int n_targets, int k, int min_distance, double min_ratio, double min_response, int coast)
{
    a.d = pdog::distance_or_default(min_distance, info);
    a.T = n_targets; a.k = k; a.h = info.frame_h; a.w = info.frame_w; a.coast = coast;
    a.rho = (float)min_ratio; a.m = (float)min_response;
}

} // namespace

extern "C" int pdog_assign_motion(pdog_tracker *t, int n_groups, int n_targets, int k, int min_distance, double min_ratio,
                                  double min_response, int coast, const int32_t *d_prev, int32_t *d_mstate, const int32_t *d_ij,
                                  const float *d_peak, const int32_t *d_count, int32_t *d_out_ij, int32_t *d_out_state, int32_t *d_next)
{
    const char *who = "pdog_assign_motion";
    if (!t) return fail(PDOG_E_ARG, std::string(who) + ": null tracker");
    if (!d_prev || !d_mstate || !d_ij || !d_peak || !d_count || !d_out_ij || !d_out_state || !d_next) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    if (int rc = pdog::check_exclusive(who, n_groups, n_targets, k, min_ratio)) return rc;
    if (int rc = pdog::check_motion(who, min_response, coast)) return rc;
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    pdog::GroupWalkState *ms = pdog::motion_state(t);
    hipStream_t stream = nullptr;
    if (int rc = pdog::stream_on_device(t, ms, &stream)) return rc;
    MotionGeo a;
    a.prev = d_prev; a.mstate = d_mstate; a.ij = d_ij; a.peak = d_peak; a.count = d_count;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.pos = nullptr; a.next = d_next; a.len = nullptr;
    a.out_stride = 1; a.step = 0;
    fill_geo(a, info, n_targets, k, min_distance, min_ratio, min_response, coast);
    ++ms->steps;
    return launch_motion(stream, a, n_groups, pdog::motion_lds(t));
}

extern "C" int pdog_detect_chains_motion(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                         int n_frames, const int32_t *h_table, int n_steps, int n_groups, int n_targets, int first,
                                         int k, int min_distance, double min_ratio, double min_response, int coast,
                                         const int32_t *d_start, int32_t *d_out_ij, int32_t *d_out_state, int32_t *d_mstate)
{
    const char *who = "pdog_detect_chains_motion";
    if (!t) return fail(PDOG_E_ARG, std::string(who) + ": null tracker");
    if (!d_frames || !h_table || !d_start || !d_out_ij || !d_out_state) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    k = pdog::k_or_default(k, n_targets);
    if (int rc = pdog::check_exclusive(who, n_groups, n_targets, k, min_ratio)) return rc;
    if (int rc = pdog::check_motion(who, min_response, coast)) return rc;
    pdog::GroupWalkState *ms = pdog::motion_state(t);
    pdog::GroupWalk w{d_frames, frame_stride, row_stride, n_frames, h_table, n_steps, n_groups, n_targets, first, k, min_distance};
    if (int rc = pdog::begin_group_walk(who, t, ms, 8, w)) return rc;
    if (w.max_len == 0) return PDOG_OK; // no group has a step

    const size_t n = (size_t)w.n;
    int32_t *pos = w.carry, *guess = pos + 2 * n, *own = guess + 2 * n; // the positions [n][2], the guesses [n][2], the walk's own mstate [n][4]
    MotionGeo a;
    a.mstate = d_mstate ? d_mstate : own; // the caller's state is walked in place; a walk at rest keeps its own and drops it
    hipLaunchKernelGGL(dog_motion_init_kernel, dim3((w.n + 255) / 256), dim3(256), 0, w.stream, d_start, w.d_len, pos, guess, a.mstate,
                       d_mstate ? 0 : 1, d_out_ij, d_out_state, w.n, n_targets, (long long)n_steps, first, w.info.frame_h, w.info.frame_w);
    HIP_TRY(hipGetLastError());
    a.prev = pos; a.ij = w.picks; a.peak = w.peak; a.count = w.counts;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.pos = pos; a.next = guess; a.len = w.d_len;
    a.out_stride = n_steps;
    fill_geo(a, w.info, n_targets, k, min_distance, min_ratio, min_response, coast);
    const bool lds = pdog::motion_lds(t);
    return pdog::walk_groups(t, ms, w, guess, [&](int s) { a.step = s; return launch_motion(w.stream, a, n_groups, lds); });
}

extern "C" int pdog_get_motion_counts(pdog_tracker *t, uint64_t out[2])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_motion_counts: null pointer");
    const pdog::GroupWalkState *ms = pdog::motion_state(t);
    out[0] = ms->steps;
    out[1] = ms->grown;
    return PDOG_OK;
}
