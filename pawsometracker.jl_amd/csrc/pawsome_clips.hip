// pawsome_clips.hip — many clips tracked as the reference tracks each (include/pawsome_dog.h, pdog_clips_*): one `Tracker`
// per video means a fill per clip (mode of ITS first frame, src/PawsomeTracker.jl:47-48) and a bootstrap per clip (the first
// position is given, the loop starts at the second frame, :99-107, :161-167).
//
// A handle borrows a tracker and uses it through the public ABI only (pdog_get_info, pdog_get_stream, pdog_set_fill,
// pdog_reserve, pdog_detect_batch, pdog_detect_chains): no kernel of the tracker is launched, named or changed here.  The
// tracker reads its fill when it launches, so the fill may change between stream-ordered launches: clips are grouped by
// fill and walked frame by frame, one batch per group and frame.  The handle owns grow-only workspace (mode tables, plan,
// per-slot frame index, guesses and step results); a call whose sizes repeat allocates nothing.  Kernels: dog_clips.hpp.
#include "pdog_host.hpp"
#include "dog_clips.hpp"
#include "dog_step.hpp"
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace pdog;

struct pdog_clips {
    pdog_tracker *t = nullptr;
    int device = 0;
    int fh = 0, fw = 0;
    DeviceBuffer<unsigned> d_table;  // multi-workgroup modes: 512 words per entry
    StagedUpload<int32_t> plan;      // order[n_slots], slot_len[n_slots], len[n_clips], then a table's frames step-major
    DeviceBuffer<int32_t> d_work;    // fidx[n_slots], guess[2 n_slots], step[2 n_slots]
    std::vector<int32_t> order, group_fill, group_start, active;
    std::vector<int32_t> table_len;  // steps per clip of the frame table being served (pdog_clips_track_indexed)
    int reserved = 0;                // windows the tracker's workspace was reserved for through this handle
    uint64_t counters[4] = {0, 0, 0, 0}; // mode launches: one workgroup per frame, several per frame; per-frame batches; chain fast paths
    int mode_form = 0;               // 0 automatic, 1 one workgroup per frame, 2 several
};

namespace {

constexpr int kModeTargetWorkgroups = 2048; // 256 CUs x 8 workgroups of 4 waves
constexpr int kModeItemsPerWorkgroup = 2048; // at least 8 pieces per lane before a frame is split

int stream_of(pdog_clips *c, hipStream_t *s)
{
    void *p = nullptr;
    if (int rc = pdog_get_stream(c->t, &p)) return rc;
    *s = (hipStream_t)p;
    return PDOG_OK;
}

// The walk of pdog_clips_track and pdog_clips_track_indexed, arguments checked by them: n_clips clips of up to n_steps
// steps.  h_table null: clip c's step k is frame c*n_steps + k of d_frames.  Otherwise step k of clip c is frame
// h_table[c*n_steps + k] of a stack of n_stack frames (the table validated, h_len its rows' lengths).
int track_walk(pdog_clips *c, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_steps, int n_clips,
               const int32_t *h_fill, const int32_t *h_len, int first, const int32_t *d_start, int32_t *d_out_ij,
               const int32_t *h_table, int n_stack)
{
    const char *who = h_table ? "pdog_clips_track_indexed" : "pdog_clips_track";
    // 1. the plan (checks fills and lengths: nothing has been launched when it fails)
    const size_t max_groups = (size_t)std::min(n_clips, 256);
    if (c->order.size() < (size_t)n_clips) c->order.resize((size_t)n_clips);
    if (c->group_fill.size() < max_groups) { c->group_fill.resize(max_groups); c->group_start.resize(max_groups + 1); c->active.resize(max_groups); }
    int n_groups = 0;
    if (int rc = pdog_clips_plan(n_clips, n_steps, first, h_fill, h_len, c->order.data(), c->group_fill.data(), c->group_start.data(), &n_groups)) {
        if (h_table) return fail(rc, std::string(who) + ": " + pdog_last_error());
        return rc;
    }
    const int n_slots = c->group_start[n_groups];
    auto len_of = [&](int clip) { return h_len ? (int)h_len[clip] : n_steps; };
    pdog_info info;
    if (int rc = pdog_get_info(c->t, &info)) return rc;
    HIP_TRY(hipSetDevice(c->device));

    // the fast path.  Contiguous clips: one fill, full lengths and first = 0 is the persistent chain under that fill and nothing
    // else.  A table: one fill (or no clip with a step to compute) is the chain over the table, whatever the lengths and first.
    const bool fast = h_table ? n_groups <= 1
                              : first == 0 && n_groups == 1 && n_slots == n_clips && len_of(c->order[n_slots - 1]) == n_steps;
    if (fast) {
        if (n_groups == 1 && c->group_fill[0] >= 0)
            if (int rc = pdog_set_fill(c->t, c->group_fill[0])) return rc;
        const int rc = h_table ? pdog_detect_chains_indexed(c->t, d_frames, frame_stride, row_stride, n_stack, h_table, n_steps, n_clips, first, d_start, d_out_ij)
                               : pdog_detect_chains(c->t, d_frames, frame_stride, row_stride, n_steps, n_clips, d_start, d_out_ij);
        (void)pdog_set_fill(c->t, info.fill);
        if (rc == PDOG_OK) ++c->counters[3];
        return rc;
    }

    hipStream_t s = nullptr;
    if (int rc = stream_of(c, &s)) return rc;
    int largest = 0;
    for (int g = 0; g < n_groups; ++g) largest = std::max(largest, c->group_start[g + 1] - c->group_start[g]);
    if (largest > c->reserved) { // once per size: the batches below then find their workspace
        if (int rc = pdog_reserve(c->t, largest)) return rc;
        c->reserved = largest;
    }
    // 2. upload the plan: order and length per slot, (first = 1) the length per clip for the copied starts, and with a table
    // the frame of every slot at every step, step-major: a group's slice of a step is that batch's frame index
    const bool want_len = first == 1 && h_len;
    int max_len = 0;
    for (int p = 0; p < n_slots; ++p) max_len = std::max(max_len, len_of(c->order[p]));
    const size_t head_words = 2 * (size_t)n_slots + (want_len ? (size_t)n_clips : 0);
    const size_t plan_words = head_words + (h_table ? (size_t)max_len * n_slots : 0);
    int32_t *hp = nullptr;
    if (int rc = c->plan.staging(plan_words, s, &hp)) return rc;
    if (int rc = c->d_work.reserve(5 * (size_t)std::max(n_slots, 1), &s)) return rc;
    for (int p = 0; p < n_slots; ++p) {
        hp[p] = c->order[p];
        hp[n_slots + p] = len_of(c->order[p]);
    }
    if (want_len) std::memcpy(hp + 2 * (size_t)n_slots, h_len, sizeof(int32_t) * (size_t)n_clips);
    if (h_table)
        for (int p = 0; p < n_slots; ++p) {
            const int32_t *row = h_table + (size_t)c->order[p] * n_steps;
            const int len = len_of(c->order[p]);
            for (int k = 0; k < max_len; ++k) hp[head_words + (size_t)k * n_slots + p] = row[std::min(k, len - 1)]; // (a slot takes part: len > first)
        }
    if (plan_words)
        if (int rc = c->plan.send(plan_words, s)) return rc;
    const int32_t *d_order = c->plan.device(), *d_slot_len = d_order + n_slots;
    const int32_t *d_len = want_len ? d_slot_len + n_slots : nullptr;
    const int32_t *d_steps = d_order + head_words;
    int32_t *d_fidx = c->d_work.get(), *d_guess = d_fidx + n_slots, *d_step = d_guess + 2 * (size_t)n_slots;
    const int n_init = std::max(n_slots, first ? n_clips : 0);
    if (n_init == 0) return PDOG_OK; // no clip has a frame to compute or a start to copy
    hipLaunchKernelGGL(clips_init_kernel, dim3((n_init + 255) / 256), dim3(256), 0, s, d_order, n_slots, n_clips, n_steps, first, d_len,
                       d_start, d_fidx, d_guess, d_out_ij);
    HIP_TRY(hipGetLastError());
    // 3. the walk: per frame and fill group one batch over the group's active prefix, then one step kernel for all groups
    for (int g = 0; g < n_groups; ++g) c->active[g] = c->group_start[g + 1] - c->group_start[g];
    int rc = PDOG_OK;
    for (int k = first; k < n_steps && rc == PDOG_OK; ++k) {
        bool any = false;
        for (int g = 0; g < n_groups && rc == PDOG_OK; ++g) {
            const int p0 = c->group_start[g];
            int &na = c->active[g];
            while (na > 0 && hp[n_slots + p0 + na - 1] <= k) --na; // lengths descend inside a group
            if (na == 0) continue;
            if (c->group_fill[g] >= 0) rc = pdog_set_fill(c->t, c->group_fill[g]);
            if (rc == PDOG_OK)
                rc = h_table ? pdog_detect_batch(c->t, d_frames, frame_stride, row_stride, n_stack, d_steps + (size_t)k * n_slots + p0,
                                                 d_guess + 2 * (size_t)p0, na, d_step + 2 * (size_t)p0, nullptr)
                             : pdog_detect_batch(c->t, d_frames + (int64_t)k * frame_stride, frame_stride, row_stride, n_clips * n_steps - k,
                                                 d_fidx + p0, d_guess + 2 * (size_t)p0, na, d_step + 2 * (size_t)p0, nullptr);
            if (rc == PDOG_OK) ++c->counters[2];
            any = true;
        }
        if (rc != PDOG_OK || !any) break;
        hipLaunchKernelGGL(dog_step_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, s, d_order, d_slot_len, n_slots, n_steps, k,
                           (const int32_t *)d_step, d_guess, d_out_ij);
        if (hipGetLastError() != hipSuccess) rc = fail(PDOG_E_HIP, std::string(who) + ": the step kernel did not launch");
    }
    (void)pdog_set_fill(c->t, info.fill);
    return rc;
}

} // namespace

extern "C" {

int pdog_clips_create(pdog_tracker *t, pdog_clips **out)
{
    if (!out) return fail(PDOG_E_ARG, "pdog_clips_create: out is null");
    *out = nullptr;
    if (!t) return fail(PDOG_E_ARG, "pdog_clips_create: null tracker");
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    if (int rc = pdog_reserve(t, 1)) return rc; // makes the tracker's device the current one
    pdog_clips *c = new pdog_clips;
    c->t = t;
    c->fh = info.frame_h;
    c->fw = info.frame_w;
    c->reserved = 1;
    const hipError_t e = hipGetDevice(&c->device);
    if (e != hipSuccess) {
        delete c;
        return fail(PDOG_E_HIP, std::string("pdog_clips_create: ") + hipGetErrorString(e));
    }
    *out = c;
    return PDOG_OK;
}

int pdog_clips_destroy(pdog_clips *c)
{
    if (!c) return PDOG_OK;
    (void)hipSetDevice(c->device);
    hipStream_t s = nullptr;
    if (stream_of(c, &s) == PDOG_OK) (void)hipStreamSynchronize(s); // kernels queued there may still use the workspace
    delete c;
    return PDOG_OK;
}

int pdog_clips_get_counters(const pdog_clips *c, uint64_t out[4])
{
    if (!c || !out) return fail(PDOG_E_ARG, "pdog_clips_get_counters: null pointer");
    std::memcpy(out, c->counters, sizeof c->counters);
    return PDOG_OK;
}

int pdog_clips_set_tuning(pdog_clips *c, const char *key, int value)
{
    if (!c || !key) return fail(PDOG_E_ARG, "pdog_clips_set_tuning: null pointer");
    const std::string k(key);
    if (k == "mode_form" && value >= 0 && value <= 2) c->mode_form = value;
    else return fail(PDOG_E_ARG, "pdog_clips_set_tuning: unknown key or value");
    return PDOG_OK;
}

int pdog_clips_modes(pdog_clips *c, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                     const int32_t *d_frame_index, int n, int32_t *d_out_mode)
{
    if (!c) return fail(PDOG_E_ARG, "pdog_clips_modes: null handle");
    if (int rc = check_stack("pdog_clips_modes", c->fw, n_frames, row_stride, frame_stride, n >= 0)) return rc;
    if (!d_frame_index && n > n_frames) return fail(PDOG_E_ARG, "pdog_clips_modes: more entries than frames and no frame index");
    if ((long long)c->fh * c->fw >= 0xffffffffLL) return fail(PDOG_E_ARG, "pdog_clips_modes: frame too large for 32-bit positions");
    if (n == 0) return PDOG_OK;
    if (!d_frames || !d_out_mode) return fail(PDOG_E_ARG, "pdog_clips_modes: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = nullptr;
    if (int rc = stream_of(c, &s)) return rc;
    ClipsModeGeo g;
    g.frames = d_frames;
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.frame_index = d_frame_index;
    g.n_frames = n_frames;
    g.h = c->fh;
    g.w = c->fw;
    g.cpr = 1 + (int)(((long long)c->fw + 15) / 16);
    const long long items = (long long)g.h * g.cpr;
    // One workgroup per frame when there are enough frames to fill the chip (or the frame is too small to split);
    // otherwise as many workgroups per frame as give every lane a few pieces and the chip its share of workgroups.
    long long parts = 1;
    if (c->mode_form == 2 || (c->mode_form == 0 && n < kModeTargetWorkgroups))
        parts = std::min((items + kModeItemsPerWorkgroup - 1) / kModeItemsPerWorkgroup, (long long)(kModeTargetWorkgroups + n - 1) / n);
    if (c->mode_form == 2) parts = std::max(parts, 2ll);
    // HIP takes fewer than 2^32 threads per grid dimension
    if ((long long)n * parts * kClipsModeThreads >= (1ll << 32)) return fail(PDOG_E_ARG, "pdog_clips_modes: too many entries for one launch");
    if (parts < 2) {
        g.parts = 1;
        hipLaunchKernelGGL(clips_mode_frame_kernel, dim3(n), dim3(kClipsModeThreads), 0, s, g, d_out_mode);
        HIP_TRY(hipGetLastError());
        ++c->counters[0];
        return PDOG_OK;
    }
    g.parts = (int)parts;
    if (int rc = c->d_table.reserve(512 * (size_t)n, &s)) return rc;
    HIP_TRY(hipMemsetAsync(c->d_table.get(), 0, sizeof(unsigned) * 512 * (size_t)n, s));
    hipLaunchKernelGGL(clips_mode_part_kernel, dim3(n * g.parts), dim3(kClipsModeThreads), 0, s, g, c->d_table.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(clips_mode_resolve_kernel, dim3(n), dim3(kClipsModeThreads), 0, s, g, (const unsigned *)c->d_table.get(), d_out_mode);
    HIP_TRY(hipGetLastError());
    ++c->counters[1];
    return PDOG_OK;
}

int pdog_clips_track(pdog_clips *c, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                     int n_clips, const int32_t *h_fill, const int32_t *h_len, int first, const int32_t *d_start,
                     int32_t *d_out_ij)
{
    if (!c) return fail(PDOG_E_ARG, "pdog_clips_track: null handle");
    if (!d_frames || !d_start || !d_out_ij) return fail(PDOG_E_ARG, "pdog_clips_track: null pointer");
    if (int rc = check_stack("pdog_clips_track", c->fw, n_frames, row_stride, frame_stride, n_clips > 0 && (long long)n_clips * n_frames <= 0x7fffffffLL)) return rc;
    if (first != 0 && first != 1) return fail(PDOG_E_ARG, "pdog_clips_track: first must be 0 or 1");
    return track_walk(c, d_frames, frame_stride, row_stride, n_frames, n_clips, h_fill, h_len, first, d_start, d_out_ij, nullptr, 0);
}

int pdog_clips_track_indexed(pdog_clips *c, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                             const int32_t *h_table, int n_steps, int n_clips, const int32_t *h_fill, int first,
                             const int32_t *d_start, int32_t *d_out_ij)
{
    if (!c) return fail(PDOG_E_ARG, "pdog_clips_track_indexed: null handle");
    if (!d_frames || !h_table || !d_start || !d_out_ij) return fail(PDOG_E_ARG, "pdog_clips_track_indexed: null pointer");
    // the lengths come from the table's negative tails; it is checked before anything is launched
    TableWalk w{"pdog_clips_track_indexed", c->fw, n_frames, row_stride, frame_stride, h_table, n_steps, n_clips, 1, first, 0, 0};
    if (int rc = check_table_walk(w, c->table_len)) return rc;
    return track_walk(c, d_frames, frame_stride, row_stride, n_steps, n_clips, h_fill, c->table_len.data(), first, d_start, d_out_ij,
                      h_table, n_frames);
}

} // extern "C"
