// pawsome_exclusive.hip — host side of the exclusive step and walk (include/pawsome_exclusive.h): per step pdog_detect_peaks for
// the G·T windows, through its public entry point, and the assignment kernel (dog_assign.hpp) behind it on the same stream.
// No kernel of the tracker is named here; what these calls keep on a tracker (scratch, the staged table, the counters) is the
// ExclusiveState that pawsome_dog.hip hands out.
#include "../../include/pawsome_exclusive.h"
#include "pdog_host.hpp"
#include "dog_assign.hpp"

#include <algorithm>
#include <cmath>

using pdog::fail;
using namespace pdog::exclusive;
static_assert(kMaxTargets == PDOG_EXCLUSIVE_MAX_TARGETS, "a group is half a wave, as the header says");

namespace {

long long distance_or_default(int min_distance, const pdog_info &info)
{
    return min_distance > 0 ? min_distance : std::max(1LL, (long long)std::ceil(info.target_width)); // pawsome_peaks.h
}

int launch_assign(hipStream_t stream, const AssignGeo &a, int n_groups)
{
    hipLaunchKernelGGL(dog_assign_kernel, dim3(n_groups), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

template <typename T>
int reserve_counted(pdog::ExclusiveState *es, pdog::DeviceBuffer<T> &b, size_t count, const hipStream_t &stream)
{
    if (count > b.capacity()) ++es->grown;
    return b.reserve(count, &stream);
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
    pdog::ExclusiveState *es = pdog::exclusive_state(t);
    void *sp = nullptr;
    if (int rc = pdog_get_stream(t, &sp)) return rc;
    HIP_TRY(hipSetDevice(es->device));
    AssignGeo a;
    a.prev = d_prev; a.ij = d_ij; a.peak = d_peak; a.count = d_count;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.next = nullptr; a.len = nullptr;
    a.out_stride = 1; a.d = distance_or_default(min_distance, info);
    a.step = 0; a.T = n_targets; a.k = k; a.rho = (float)min_ratio;
    ++es->steps;
    return launch_assign((hipStream_t)sp, a, n_groups);
}

extern "C" int pdog_detect_chains_exclusive(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                            int n_frames, const int32_t *h_table, int n_steps, int n_groups, int n_targets,
                                            int first, int k, int min_distance, double min_ratio, const int32_t *d_start,
                                            int32_t *d_out_ij, int32_t *d_out_state)
{
    const char *who = "pdog_detect_chains_exclusive";
    if (!t) return fail(PDOG_E_ARG, std::string(who) + ": null tracker");
    if (!d_frames || !h_table || !d_start || !d_out_ij || !d_out_state) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    if (k <= 0 && n_targets >= 1) k = std::min(PDOG_PEAKS_MAX_K, 2 * std::min(n_targets, PDOG_PEAKS_MAX_K));
    if (int rc = pdog::check_exclusive(who, n_groups, n_targets, k, min_ratio)) return rc;
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    const long long n_ll = (long long)n_groups * n_targets;
    if (int rc = pdog::check_stack(who, info.frame_w, n_frames, row_stride, frame_stride, n_steps > 0 && n_ll * n_steps <= 0x7fffffffLL)) return rc;
    if (n_ll * info.n_strips > 0x7ffffff0LL) return fail(PDOG_E_ARG, std::string(who) + ": batch too large"); // (pdog_detect_peaks' limit, judged before the first launch)
    if (first != 0 && first != 1) return fail(PDOG_E_ARG, std::string(who) + ": first must be 0 or 1");
    pdog::ExclusiveState *es = pdog::exclusive_state(t);
    if (es->len.size() < (size_t)n_groups) es->len.resize((size_t)n_groups);
    int max_len = 0;
    if (int rc = pdog::chain_table_lengths(who, h_table, n_steps, n_groups, n_frames, es->len.data(), &max_len)) return rc;
    if (max_len == 0) return PDOG_OK; // no group has a step

    void *sp = nullptr;
    if (int rc = pdog_get_stream(t, &sp)) return rc;
    const hipStream_t stream = (hipStream_t)sp;
    HIP_TRY(hipSetDevice(es->device));
    const int n = (int)n_ll, T = n_targets;
    if (int rc = reserve_counted(es, es->d_words, (size_t)n * (3 + 2 * (size_t)k), stream)) return rc;
    if (int rc = reserve_counted(es, es->d_peak, (size_t)n * k, stream)) return rc;
    int32_t *cur = es->d_words.get(), *picks = cur + 2 * (size_t)n, *counts = picks + 2 * (size_t)n * k;

    // the table by step with a frame per window (step s's row is that batch's frame index), a group that has ended repeating
    // its last frame (frame 0 if it has none); then the lengths
    const size_t cells = (size_t)max_len * n, words = cells + (size_t)n_groups;
    if (words > es->table_words) { ++es->grown; es->table_words = words; }
    int32_t *hp = nullptr;
    if (int rc = es->table.staging(words, stream, &hp)) return rc;
    for (int g = 0; g < n_groups; ++g) {
        const int32_t *row = h_table + (size_t)g * n_steps;
        const int len = es->len[g];
        for (int s = 0; s < max_len; ++s) {
            const int32_t f = s < len ? row[s] : (len ? row[len - 1] : 0);
            std::fill_n(hp + (size_t)s * n + (size_t)g * T, T, f);
        }
    }
    std::copy_n(es->len.data(), n_groups, hp + cells);
    if (int rc = es->table.send(words, stream)) return rc;
    const int32_t *d_cols = es->table.device(), *d_len = d_cols + cells;

    hipLaunchKernelGGL(dog_assign_init_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_start, d_len, cur, d_out_ij, d_out_state, n, T,
                       (long long)n_steps, first);
    HIP_TRY(hipGetLastError());
    AssignGeo a;
    a.prev = cur; a.ij = picks; a.peak = es->d_peak.get(); a.count = counts;
    a.out_ij = d_out_ij; a.out_state = d_out_state; a.next = cur; a.len = d_len;
    a.out_stride = n_steps; a.d = distance_or_default(min_distance, info);
    a.T = T; a.k = k; a.rho = (float)min_ratio;
    for (int s = first; s < max_len; ++s) {
        if (int rc = pdog_detect_peaks(t, d_frames, frame_stride, row_stride, n_frames, d_cols + (size_t)s * n, cur, n, k, (int)a.d, picks,
                                       es->d_peak.get(), counts, nullptr))
            return rc;
        a.step = s;
        ++es->steps;
        if (int rc = launch_assign(stream, a, n_groups)) return rc;
    }
    return PDOG_OK;
}

extern "C" int pdog_get_exclusive_counts(pdog_tracker *t, uint64_t out[2])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_exclusive_counts: null pointer");
    const pdog::ExclusiveState *es = pdog::exclusive_state(t);
    out[0] = es->steps;
    out[1] = es->grown;
    return PDOG_OK;
}
