// pdog_walk.hpp — what the walks of GROUPS over a frame table share (pawsome_exclusive.hip, pawsome_motion.hip): the defaults of
// their arguments, the call's checks behind the rule's own, the scratch and the staged table on a GroupWalkState, and the loop
// that runs pdog_detect_peaks for a step's windows, through its public entry point, and the rule's kernel behind it on the
// same stream.  No kernel header is included here (pdog_host.hpp says why): the rule's launch comes in as a callable.
#pragma once
#include "../../include/pawsome_exclusive.h"
#include "pdog_host.hpp"

#include <algorithm>
#include <cmath>

#pragma GCC visibility push(hidden)
namespace pdog {

inline long long distance_or_default(int min_distance, const pdog_info &info)
{
    return min_distance > 0 ? min_distance : std::max(1LL, (long long)std::ceil(info.target_width)); // pawsome_peaks.h
}
inline int k_or_default(int k, int n_targets)
{
    return k <= 0 && n_targets >= 1 ? std::min(PDOG_PEAKS_MAX_K, 2 * std::min(n_targets, PDOG_PEAKS_MAX_K)) : k; // pawsome_exclusive.h
}

// The tracker's stream, with the state's device made current.
inline int stream_on_device(pdog_tracker *t, const GroupWalkState *st, hipStream_t *out)
{
    void *sp = nullptr;
    if (int rc = pdog_get_stream(t, &sp)) return rc;
    HIP_TRY(hipSetDevice(st->device));
    *out = (hipStream_t)sp;
    return PDOG_OK;
}

template <typename T>
int reserve_counted(GroupWalkState *st, DeviceBuffer<T> &b, size_t count, const hipStream_t &stream)
{
    if (count > b.capacity()) ++st->grown;
    return b.reserve(count, &stream);
}

struct GroupWalk {
    // the call as the entry point received it, k after k_or_default and the rule's own checks
    const uint8_t *d_frames;
    int64_t frame_stride, row_stride;
    int n_frames;
    const int32_t *h_table;
    int n_steps, n_groups, T, first, k, min_distance;
    // begin_group_walk's: max_len = 0 means that no group has a step, and nothing else is set
    int max_len, n;      // the longest row; n = n_groups * T windows
    pdog_info info;
    hipStream_t stream;
    long long d;         // the picks' distance
    int32_t *carry;      // the state's d_words: [n][carry_words] for the rule, then picks [n][k][2] and counts [n]
    int32_t *picks, *counts;
    float *peak;
    const int32_t *d_cols, *d_len; // the table by step with a frame per window, and the groups' lengths
};

// The call checked (check_table_walk, in `who`'s name), then the scratch, carry_words words per window for the rule among it,
// and the table staged on the tracker's stream.
inline int begin_group_walk(const char *who, pdog_tracker *t, GroupWalkState *st, int carry_words, GroupWalk &w)
{
    if (int rc = pdog_get_info(t, &w.info)) return rc;
    TableWalk tw{who, w.info.frame_w, w.n_frames, w.row_stride, w.frame_stride, w.h_table, w.n_steps, w.n_groups, w.T, w.first, w.info.n_strips, 0};
    if (int rc = check_table_walk(tw, st->table.len)) return rc;
    if (!(w.max_len = tw.max_len)) return PDOG_OK;
    if (int rc = stream_on_device(t, st, &w.stream)) return rc;
    w.n = w.n_groups * w.T;
    const size_t n = (size_t)w.n;
    if (int rc = reserve_counted(st, st->d_words, n * ((size_t)carry_words + 1 + 2 * (size_t)w.k), w.stream)) return rc;
    if (int rc = reserve_counted(st, st->d_peak, n * w.k, w.stream)) return rc;
    w.carry = st->d_words.get();
    w.picks = w.carry + n * carry_words;
    w.counts = w.picks + 2 * n * w.k;
    w.peak = st->d_peak.get();
    w.d = distance_or_default(w.min_distance, w.info);
    return st->table.upload(w.h_table, TableShape{w.n_steps, w.n_groups, w.max_len, w.T}, w.stream, &st->grown, &w.d_cols, &w.d_len);
}

// The steps first ... max_len - 1: the k best peaks of every window at `guess`, then the rule's launch(s) behind them.
template <typename Launch>
int walk_groups(pdog_tracker *t, GroupWalkState *st, const GroupWalk &w, const int32_t *guess, Launch launch)
{
    for (int s = w.first; s < w.max_len; ++s) {
        if (int rc = pdog_detect_peaks(t, w.d_frames, w.frame_stride, w.row_stride, w.n_frames, w.d_cols + (size_t)s * w.n, guess, w.n, w.k, (int)w.d,
                                       w.picks, w.peak, w.counts, nullptr))
            return rc;
        ++st->steps;
        if (int rc = launch(s)) return rc;
    }
    return PDOG_OK;
}

} // namespace pdog
#pragma GCC visibility pop
