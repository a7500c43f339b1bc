// pawsome_motion.hip — host side of the motion step and walk (include/pawsome_motion.h): per step pdog_detect_peaks for the G·T
// windows at the predictions, through its public entry point, and the motion kernel (dog_motion.hpp) behind it on the same
// stream.  No kernel of the tracker is named here; what these calls keep on a tracker (scratch, the staged table, the
// switch, the counters) is the MotionState that pawsome_dog.hip hands out.
#include "../../include/pawsome_motion.h"
#include "pdog_host.hpp"
#include "dog_motion.hpp"

#include <algorithm>
#include <cmath>

using pdog::fail;
using namespace pdog::motion;
static_assert(kMaxTargets == PDOG_MOTION_MAX_TARGETS, "a group is half a wave, as the header says");
static_assert(kLdsWords == PDOG_MOTION_MAX_TARGETS * PDOG_PEAKS_MAX_K, "the LDS image holds every lane's whole list");

namespace {

long long distance_or_default(int min_distance, const pdog_info &info)
{
    return min_distance > 0 ? min_distance : std::max(1LL, (long long)std::ceil(info.target_width)); // pawsome_peaks.h
}

int launch_motion(hipStream_t stream, const MotionGeo &a, int n_groups, bool lds)
{
    if (lds) hipLaunchKernelGGL(dog_motion_kernel<true>, dim3(n_groups), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(dog_motion_kernel<false>, dim3(n_groups), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

template <typename T>
int reserve_counted(pdog::MotionState *ms, pdog::DeviceBuffer<T> &b, size_t count, const hipStream_t &stream)
{
    if (count > b.capacity()) ++ms->grown;
    return b.reserve(count, &stream);
}

void fill_geo(MotionGeo &a, const pdog_info &info, int n_targets, int k, int min_distance, double min_ratio, double min_response, int coast)
{
    a.d = distance_or_default(min_distance, info);
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
    pdog::MotionState *ms = pdog::motion_state(t);
    void *sp = nullptr;
    if (int rc = pdog_get_stream(t, &sp)) return rc;
    HIP_TRY(hipSetDevice(ms->device));
    MotionGeo a;
    a.prev = d_prev; a.mstate = d_mstate; a.ij = d_ij; a.peak = d_peak; a.count = d_count;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.pos = nullptr; a.next = d_next; a.len = nullptr;
    a.out_stride = 1; a.step = 0;
    fill_geo(a, info, n_targets, k, min_distance, min_ratio, min_response, coast);
    ++ms->steps;
    return launch_motion((hipStream_t)sp, a, n_groups, ms->lds);
}

extern "C" int pdog_detect_chains_motion(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                         int n_frames, const int32_t *h_table, int n_steps, int n_groups, int n_targets, int first,
                                         int k, int min_distance, double min_ratio, double min_response, int coast,
                                         const int32_t *d_start, int32_t *d_out_ij, int32_t *d_out_state, int32_t *d_mstate)
{
    const char *who = "pdog_detect_chains_motion";
    if (!t) return fail(PDOG_E_ARG, std::string(who) + ": null tracker");
    if (!d_frames || !h_table || !d_start || !d_out_ij || !d_out_state) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    if (k <= 0 && n_targets >= 1) k = std::min(PDOG_PEAKS_MAX_K, 2 * std::min(n_targets, PDOG_PEAKS_MAX_K));
    if (int rc = pdog::check_exclusive(who, n_groups, n_targets, k, min_ratio)) return rc;
    if (int rc = pdog::check_motion(who, min_response, coast)) return rc;
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    const long long n_ll = (long long)n_groups * n_targets;
    if (int rc = pdog::check_stack(who, info.frame_w, n_frames, row_stride, frame_stride, n_steps > 0 && n_ll * n_steps <= 0x7fffffffLL)) return rc;
    if (n_ll * info.n_strips > 0x7ffffff0LL) return fail(PDOG_E_ARG, std::string(who) + ": batch too large"); // (pdog_detect_peaks' limit, judged before the first launch)
    if (first != 0 && first != 1) return fail(PDOG_E_ARG, std::string(who) + ": first must be 0 or 1");
    pdog::MotionState *ms = pdog::motion_state(t);
    if (ms->len.size() < (size_t)n_groups) ms->len.resize((size_t)n_groups);
    int max_len = 0;
    if (int rc = pdog::chain_table_lengths(who, h_table, n_steps, n_groups, n_frames, ms->len.data(), &max_len)) return rc;
    if (max_len == 0) return PDOG_OK; // no group has a step

    void *sp = nullptr;
    if (int rc = pdog_get_stream(t, &sp)) return rc;
    const hipStream_t stream = (hipStream_t)sp;
    HIP_TRY(hipSetDevice(ms->device));
    const int n = (int)n_ll, T = n_targets;
    if (int rc = reserve_counted(ms, ms->d_words, (size_t)n * (9 + 2 * (size_t)k), stream)) return rc;
    if (int rc = reserve_counted(ms, ms->d_peak, (size_t)n * k, stream)) return rc;
    int32_t *pos = ms->d_words.get(), *guess = pos + 2 * (size_t)n, *own = guess + 2 * (size_t)n, *picks = own + 4 * (size_t)n,
            *counts = picks + 2 * (size_t)n * k;

    // the table by step with a frame per window, then the lengths: as pdog_detect_chains_exclusive stages them
    const size_t cells = (size_t)max_len * n, words = cells + (size_t)n_groups;
    if (words > ms->table_words) { ++ms->grown; ms->table_words = words; }
    int32_t *hp = nullptr;
    if (int rc = ms->table.staging(words, stream, &hp)) return rc;
    for (int g = 0; g < n_groups; ++g) {
        const int32_t *row = h_table + (size_t)g * n_steps;
        const int len = ms->len[g];
        for (int s = 0; s < max_len; ++s) {
            const int32_t f = s < len ? row[s] : (len ? row[len - 1] : 0);
            std::fill_n(hp + (size_t)s * n + (size_t)g * T, T, f);
        }
    }
    std::copy_n(ms->len.data(), n_groups, hp + cells);
    if (int rc = ms->table.send(words, stream)) return rc;
    const int32_t *d_cols = ms->table.device(), *d_len = d_cols + cells;

    MotionGeo a;
    a.mstate = d_mstate ? d_mstate : own; // the caller's state is walked in place; a walk at rest keeps its own and drops it
    hipLaunchKernelGGL(dog_motion_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_start, d_len, pos, guess, a.mstate,
                       d_mstate ? 0 : 1, d_out_ij, d_out_state, n, T, (long long)n_steps, first, info.frame_h, info.frame_w);
    HIP_TRY(hipGetLastError());
    a.prev = pos; a.ij = picks; a.peak = ms->d_peak.get(); a.count = counts;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.pos = pos; a.next = guess; a.len = d_len;
    a.out_stride = n_steps;
    fill_geo(a, info, T, k, min_distance, min_ratio, min_response, coast);
    for (int s = first; s < max_len; ++s) {
        if (int rc = pdog_detect_peaks(t, d_frames, frame_stride, row_stride, n_frames, d_cols + (size_t)s * n, guess, n, k, (int)a.d, picks,
                                       ms->d_peak.get(), counts, nullptr))
            return rc;
        a.step = s;
        ++ms->steps;
        if (int rc = launch_motion(stream, a, n_groups, ms->lds)) return rc;
    }
    return PDOG_OK;
}

extern "C" int pdog_get_motion_counts(pdog_tracker *t, uint64_t out[2])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_motion_counts: null pointer");
    const pdog::MotionState *ms = pdog::motion_state(t);
    out[0] = ms->steps;
    out[1] = ms->grown;
    return PDOG_OK;
}
