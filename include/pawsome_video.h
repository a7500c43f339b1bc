/*
 * pawsome_video.h — chains over a FRAME TABLE: start, stop, fps and several targets per video on a stack of frames
 * that already lives in device memory.  Part of the C ABI of pawsome_dog.h, which includes this file at its end (include
 * that one; the types and status codes are declared there).
 *
 * The reference's public call is track(file; start, stop, target_width, start_location, window_size, darker_target,
 * fps, diagnostic_file) (src/PawsomeTracker.jl:130-146).  It turns start, stop and fps into an ffmpeg command line
 * (:155) that hands over the selected frames one by one, and returns the time stamps ts beside the positions
 * (:150-153, :173).  With the video in HBM at its native rate there is nothing to decode: the selection is a table of
 * frame indices, and a chain (:163-169) walks the table instead of a contiguous stack.  Several rows may name the same
 * frames — several targets in one arena, several start/stop windows of one video — without a copy of the video each.
 */
#ifndef PAWSOME_VIDEO_H
#define PAWSOME_VIDEO_H

#include "pawsome_dog.h" /* types and status codes (it includes this file at its end) */

#ifdef __cplusplus
extern "C" {
#endif

#define PDOG_DEFAULT_STOP 86399.999 /* DEFAULT_MAX_DURATION_SECONDS, src/PawsomeTracker.jl:19 */

/* ---- host arithmetic (no GPU) ---- */
/* The time stamps of src/PawsomeTracker.jl:150-152: t = stop - start, n = round(Int, fps * t) (ties to even),
 * ts = range(start, stop, n), restated as out_ts[j] = start + j * ((stop - start) / (n - 1)) in Float64, each operation
 * rounded on its own; n == 1 gives {start}.  out_ts == NULL only reports n in *out_n.  UNPINNED: Julia builds such a
 * range in TwicePrecision arithmetic, and no Julia was at hand to compare last bits; the restatement may differ from it
 * by an ulp at interior points (both give start at j = 0).  PDOG_E_ARG, outputs untouched, for stop <= start, fps <= 0,
 * n < 1, cap < n or a null out_n. */
int pdog_time_axis(double start, double stop, double fps, double *out_ts, int cap, int *out_n);
/* Which frames of a stack `ffmpeg -ss start -i f -t t -vf fps=fps` (:155) selects: the stack holds n_frames frames at
 * `rate` frames per second, frame i at time i / rate.  i0 = ceil(start * rate) is the first frame at or after start;
 * input frame i0 + i belongs to output slot o(i) = floor((i * fps) / rate + 0.5), evaluated in that order in Float64;
 * output j takes frame i0 + max{ i : o(i) <= j } — of several frames in one slot the later one wins, and an empty slot
 * repeats the previous frame.  Outputs exist for j = 0 ... min(n, o(n_frames - 1 - i0) + 1) - 1 with n from the time
 * axis above; *out_n reports how many, which is the reference's last_frame (:173), and out_index (room for cap entries;
 * NULL: only the count) receives them.
 * UNPINNED, like the five recollections listed for the overlay in pawsome_dog.h: this rule is a RECOLLECTION of
 * libavfilter's fps filter (round = near; of frames with equal output time stamp the earlier one is dropped), and of -ss
 * in front of -i starting at the first frame at or after `start`.  Neither ffmpeg nor Julia was at hand to check it.  A
 * caller who knows better passes their own table to the entry points below: nothing else depends on this rule.
 * PDOG_E_ARG, outputs untouched, for rate <= 0, n_frames <= 0, start < 0, the time axis' errors, a stack with no frame
 * at or after start, cap below the count or a null out_n. */
int pdog_fps_table(double rate, int n_frames, double start, double stop, double fps, int32_t *out_index, int cap,
                   int *out_n);

/* ---- the chain over a frame table (src/PawsomeTracker.jl:163-169 on selected frames) ----
 * d_frames is ONE stack of n_frames frames (device; frame i at d_frames + i*frame_stride, rows row_stride bytes apart).
 * h_table is a HOST array, n_clips rows of n_steps int32, consumed before the call returns: step k of clip c looks at
 * frame h_table[c*n_steps + k].  A clip ends where its row turns negative: len[c] is the count of leading non-negative
 * entries.  d_start is n_clips x 2 and d_out_ij n_clips x n_steps x 2 (device, 1-based (row, col)).
 *   first = 0: out[c][0] = functor(frame table[c][0], start[c]); out[c][k] = functor(frame table[c][k], out[c][k-1]), k < len[c]
 *   first = 1: out[c][0] = start[c] exactly as given when len[c] >= 1 (:104, :161); then the same loop for 1 <= k < len[c]
 * under the tracker's fill (:163-167).  Rows k >= len[c] are not written.
 * The library validates the table before anything is launched: every entry must be < n_frames, and negative entries may
 * only form the tail of a row.  No table can therefore make a kernel read outside d_frames.  PDOG_E_ARG, with nothing
 * launched, for that, a null pointer, first other than 0 or 1, a non-positive size, row_stride < frame_w, a negative
 * frame_stride or n_clips * n_steps beyond int32.  PDOG_E_RANGE for a device-resident guess arrives through pdog_sync.
 * Asynchronous on the tracker's stream (the call may wait for the PREVIOUS call's table upload, and drains the stream
 * when the table workspace grows); apart from that workspace nothing is allocated once sizes repeat.
 * Paths: chosen as for the chains entry point of pawsome_dog.h.  The kernels that walk a clip themselves — one workgroup
 * per clip, the persistent roll chain, the cooperative launch for a few clips of large windows — read the table on the
 * device, one scalar load per clip and step, in instances of their own (the existing launches are compiled as before);
 * otherwise one clip is a launch per step whose frame the host names, and several clips are a batch per step whose
 * frame index is a column of the table (clips that have ended keep their last guess and store nothing).  A table of a
 * single step always runs that way. */
int pdog_detect_chains_indexed(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                               int n_frames, const int32_t *h_table, int n_steps, int n_clips, int first,
                               const int32_t *d_start, int32_t *d_out_ij);

/* ---- the same with a fill per clip (src/PawsomeTracker.jl:47-48: every video's PaddedView has its own) ----
 * The walk of the clips track entry point of pawsome_dog.h — per step and fill group one detect-batch launch under that
 * group's fill, plan and ordering those of its plan function — with every slot's frame taken from the table instead of
 * counted up; arguments as for the chain over a table above, h_fill (HOST, consumed before the call returns) as there:
 * a fill per clip, or NULL = the tracker's fill for all.  The lengths are the table's: len[c] is the count of leading
 * non-negative entries of row c.  Clips of ONE fill (or no clip with a step to compute) are handed to the chain over a
 * table above under that fill, whatever their lengths and `first`: that is the fast-path counter out[3] of the handle,
 * as for contiguous clips.  The tracker's fill on return is what it was before.  PDOG_E_ARG, with nothing launched, for
 * everything the chain over a table refuses and for a fill outside 0 ... 255. */
int pdog_clips_track_indexed(pdog_clips *c, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                             int n_frames, const int32_t *h_table, int n_steps, int n_clips, const int32_t *h_fill,
                             int first, const int32_t *d_start, int32_t *d_out_ij);

#ifdef __cplusplus
}
#endif
#endif /* PAWSOME_VIDEO_H */
