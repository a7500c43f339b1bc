// pawsome_frame_blobs.hip — every connected blob of a whole frame, behind include/pawsome_frame_blobs.h (pdog_fb_*,
// pdog_frame_blobs).
//
// A handle holds the scratch of `in_flight` steps — a label and an area word per pixel, the blocks' counts — and ONE
// StagedUpload through which a call's frame table goes up on the call's stream, as pdog_bg does.  A call clears its outputs,
// then runs the seven kernels of dog_frame_blobs.hpp once per round of at most `in_flight` steps; everything is queued on the
// one stream, so a round's scratch is the previous round's, reused in stream order.  This file uses nothing else of the library.
#include "pdog_host.hpp"
#include "dog_frame_blobs.hpp"
#include "../../include/pawsome_frame_blobs.h"
#include <algorithm>
#include <string>

using namespace pdog;

struct pdog_fb {
    int device = 0, h = 0, w = 0, in_flight = 0, n_blocks = 0;
    DeviceBuffer<int32_t> d_labels, d_area, d_block_counts;
    StagedUpload<int32_t> words; // the frame table of the last call
    hipStream_t last = nullptr;
    bool launched = false;
    hipEvent_t ev = nullptr;
};

namespace {

static_assert(fblobs::kMaxWidth == PDOG_MAX_ROW_STRIDE, "size_refusal's width limit is the row stride's");

// The device made current and `s` ordered behind the stream that used the scratch last.
int begin(pdog_fb *fb, hipStream_t s)
{
    HIP_TRY(hipSetDevice(fb->device));
    if (fb->launched && s != fb->last) {
        HIP_TRY(hipEventRecord(fb->ev, fb->last));
        HIP_TRY(hipStreamWaitEvent(s, fb->ev, 0));
    }
    return PDOG_OK;
}

std::string num(int64_t v) { return std::to_string((long long)v); }

} // namespace

extern "C" {

int pdog_fb_create(int device, int frame_h, int frame_w, int steps_in_flight, pdog_fb **out)
{
    if (!out) return fail(PDOG_E_ARG, "pdog_fb_create: out is null");
    *out = nullptr;
    if (const char *why = fblobs::size_refusal(frame_h, frame_w))
        return fail(PDOG_E_ARG, "pdog_fb_create: bad frame size " + num(frame_h) + " x " + num(frame_w) + ": " + why);
    if (steps_in_flight < 1 || steps_in_flight > PDOG_FB_MAX_IN_FLIGHT)
        return fail(PDOG_E_ARG, "pdog_fb_create: steps_in_flight " + num(steps_in_flight) + " outside 1 ... " + num(PDOG_FB_MAX_IN_FLIGHT));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDOG_E_NODEV, "pdog_fb_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(PDOG_E_ARG, "pdog_fb_create: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    pdog_fb *fb = new pdog_fb;
    fb->device = device;
    fb->h = frame_h;
    fb->w = frame_w;
    fb->in_flight = steps_in_flight;
    const size_t n_pix = (size_t)frame_h * frame_w;
    fb->n_blocks = (int)((n_pix + fblobs::kThreads - 1) / fblobs::kThreads);
    hipError_t e = fb->d_labels.try_reserve(n_pix * steps_in_flight, nullptr);
    if (e == hipSuccess) e = fb->d_area.try_reserve(n_pix * steps_in_flight, nullptr);
    if (e == hipSuccess) e = fb->d_block_counts.try_reserve((size_t)fb->n_blocks * steps_in_flight, nullptr);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&fb->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        pdog_fb_destroy(fb);
        return fail(e == hipErrorOutOfMemory ? PDOG_E_ALLOC : PDOG_E_HIP, std::string("pdog_fb_create: ") + hipGetErrorString(e));
    }
    *out = fb;
    return PDOG_OK;
}

int pdog_fb_destroy(pdog_fb *fb)
{
    if (!fb) return PDOG_OK;
    (void)hipSetDevice(fb->device);
    if (fb->launched) (void)hipStreamSynchronize(fb->last);
    if (fb->ev) (void)hipEventDestroy(fb->ev);
    delete fb;
    return PDOG_OK;
}

int pdog_frame_blobs(pdog_fb *fb, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                     const int32_t *h_table, int n_steps, int level, int darker, int min_contrast, int connectivity, int64_t min_area,
                     int64_t max_area, int cap, int64_t *d_out_words, int32_t *d_out_count)
{
    const std::string who = "pdog_frame_blobs";
    if (!fb) return fail(PDOG_E_ARG, who + ": null handle");
    if (n_frames <= 0) return fail(PDOG_E_ARG, who + ": n_frames " + num(n_frames) + " is not positive");
    if (n_steps < 0) return fail(PDOG_E_ARG, who + ": n_steps " + num(n_steps) + " is negative");
    if (level < 0 || level > 255) return fail(PDOG_E_ARG, who + ": level " + num(level) + " outside 0 ... 255");
    if (min_contrast < 1 || min_contrast > 255) return fail(PDOG_E_ARG, who + ": min_contrast " + num(min_contrast) + " outside 1 ... 255");
    if (connectivity != 4 && connectivity != 8) return fail(PDOG_E_ARG, who + ": connectivity " + num(connectivity) + " is neither 4 nor 8");
    if (min_area < 1) return fail(PDOG_E_ARG, who + ": min_area " + num(min_area) + " is below 1");
    if (max_area < min_area) return fail(PDOG_E_ARG, who + ": max_area " + num(max_area) + " is below min_area " + num(min_area));
    if (cap < 1) return fail(PDOG_E_ARG, who + ": cap " + num(cap) + " is below 1");
    if (row_stride < fb->w || row_stride > PDOG_MAX_ROW_STRIDE)
        return fail(PDOG_E_ARG, who + ": bad stride (row_stride " + num(row_stride) + " outside frame width " + num(fb->w) + " ... " + num(PDOG_MAX_ROW_STRIDE) + ")");
    if (frame_stride < 0) return fail(PDOG_E_ARG, who + ": bad stride (frame_stride " + num(frame_stride) + " is negative)");
    if (n_steps == 0) return PDOG_OK;
    if (!d_frames || !h_table || !d_out_words || !d_out_count)
        return fail(PDOG_E_ARG, who + ": null pointer (" + (!d_frames ? "d_frames" : !h_table ? "h_table" : !d_out_words ? "d_out_words" : "d_out_count") + ")");
    for (int k = 0; k < n_steps; ++k)
        if (h_table[k] < 0 || h_table[k] >= n_frames)
            return fail(PDOG_E_ARG, who + ": table entry " + num(k) + " is " + num(h_table[k]) + ", outside 0 ... n_frames-1");
    const hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = begin(fb, s)) return rc;
    int32_t *st = nullptr;
    if (int rc = fb->words.staging((size_t)n_steps, s, &st)) return rc;
    std::copy(h_table, h_table + n_steps, st);
    if (int rc = fb->words.send((size_t)n_steps, s)) return rc;
    fb->last = s; // (also where a launch fails: the stream has the upload)
    fb->launched = true;
    HIP_TRY(hipMemsetAsync(d_out_words, 0, sizeof(int64_t) * fblobs::kWords * (size_t)cap * (size_t)n_steps, s));
    HIP_TRY(hipMemsetAsync(d_out_count, 0, sizeof(int32_t) * 2 * (size_t)n_steps, s));
    fblobs::Geo g;
    g.frames = d_frames;
    g.labels = fb->d_labels.get();
    g.area = fb->d_area.get();
    g.block_counts = fb->d_block_counts.get();
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.min_area = min_area;
    g.max_area = max_area;
    g.h = fb->h;
    g.w = fb->w;
    g.n_pix = fb->h * fb->w;
    g.n_blocks = fb->n_blocks;
    g.level = level;
    g.darker = darker != 0;
    g.min_contrast = min_contrast;
    g.conn8 = connectivity == 8;
    g.cap = cap;
    const unsigned tiles_x = (unsigned)(g.w + fblobs::kTile - 1) / fblobs::kTile, tiles_y = (unsigned)(g.h + fblobs::kTile - 1) / fblobs::kTile;
    const unsigned n_hb = (unsigned)(g.h - 1) / fblobs::kTile, n_vb = (unsigned)(g.w - 1) / fblobs::kTile;
    const unsigned borders = n_hb * (unsigned)g.w + n_vb * (unsigned)g.h * (g.conn8 ? 2u : 1u);
    const unsigned row_words = (unsigned)g.h * ((unsigned)(g.w + 63) / 64);
    const dim3 block(fblobs::kThreads);
    for (int k0 = 0; k0 < n_steps; k0 += fb->in_flight) {
        const unsigned nk = (unsigned)std::min(fb->in_flight, n_steps - k0);
        g.table = fb->words.device() + k0;
        g.out_words = d_out_words + (int64_t)k0 * cap * fblobs::kWords;
        g.out_count = d_out_count + 2 * (int64_t)k0;
        HIP_TRY(hipMemsetAsync(g.area, 0, sizeof(int32_t) * (size_t)g.n_pix * nk, s));
        hipLaunchKernelGGL(fblobs::fb_label_kernel, dim3(tiles_x, tiles_y, nk), dim3(fblobs::kLabelThreads), 0, s, g);
        if (borders) hipLaunchKernelGGL(fblobs::fb_merge_kernel, dim3((borders + fblobs::kThreads - 1) / fblobs::kThreads, nk), block, 0, s, g);
        hipLaunchKernelGGL(fblobs::fb_flatten_kernel, dim3((unsigned)g.n_blocks, nk), block, 0, s, g);
        hipLaunchKernelGGL(fblobs::fb_count_kernel, dim3((unsigned)g.n_blocks, nk), block, 0, s, g);
        hipLaunchKernelGGL(fblobs::fb_scan_kernel, dim3(nk), dim3(fblobs::kScanThreads), 0, s, g);
        hipLaunchKernelGGL(fblobs::fb_rank_kernel, dim3((unsigned)g.n_blocks, nk), block, 0, s, g);
        hipLaunchKernelGGL(fblobs::fb_sums_kernel, dim3((row_words + fblobs::kThreads / 64 - 1) / (fblobs::kThreads / 64), nk), block, 0, s, g);
        HIP_TRY(hipGetLastError());
    }
    return PDOG_OK;
}

} // extern "C"
