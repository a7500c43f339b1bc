// pawsome_background.hip — the static background model behind include/pawsome_background.h (pdog_bg_*): the per-pixel lower
// median of some frames of a stack, and frames of the stack with that model subtracted.
//
// A handle holds the model (frame_h x frame_w bytes, dense, on its device) and ONE StagedUpload through which a call's host
// words — the sample list of an estimate, the frame table of a subtract — go up on the call's stream.  The host keeps only
// whether a model exists and which stream touched it last, so a call needs no host synchronisation beyond the staging's own.
// The kernels are in dog_background.hpp; this file uses nothing else of the library.
#include "pdog_host.hpp"
#include "dog_background.hpp"
#include <algorithm>
#include <string>

using namespace pdog;

struct pdog_bg {
    int device = 0, h = 0, w = 0;
    DeviceBuffer<uint8_t> d_model;
    StagedUpload<int32_t> words; // the sample list or the frame table of the last call
    bool has_model = false;
    hipStream_t last = nullptr;
    bool launched = false;
    hipEvent_t ev = nullptr;
};

namespace {

constexpr int kMaxStepsPerLaunch = 1 << 15; // grid.y

// The device made current and `s` ordered behind the stream that touched the model last.
int begin(pdog_bg *bg, hipStream_t s)
{
    HIP_TRY(hipSetDevice(bg->device));
    if (bg->launched && s != bg->last) {
        HIP_TRY(hipEventRecord(bg->ev, bg->last));
        HIP_TRY(hipStreamWaitEvent(s, bg->ev, 0));
    }
    return PDOG_OK;
}
void done(pdog_bg *bg, hipStream_t s)
{
    bg->last = s;
    bg->launched = true;
}

// n host words on their way to the device, on s
int stage(pdog_bg *bg, hipStream_t s, const int32_t *h_words, int n)
{
    int32_t *st = nullptr;
    if (int rc = bg->words.staging((size_t)n, s, &st)) return rc;
    std::copy(h_words, h_words + n, st);
    return bg->words.send((size_t)n, s);
}

int check_entries(const std::string &who, const char *what, const int32_t *v, int n, int n_frames)
{
    for (int k = 0; k < n; ++k)
        if (v[k] < 0 || v[k] >= n_frames)
            return fail(PDOG_E_ARG, who + ": " + what + " entry " + std::to_string(k) + " is " + std::to_string(v[k]) + ", outside 0 ... n_frames-1");
    return PDOG_OK;
}

template <int KMAX>
void launch_median(const BgMedianGeo &g, hipStream_t s)
{
    const dim3 grid(((unsigned)g.h * (unsigned)g.wpr + kBgThreads - 1) / kBgThreads), block(kBgThreads);
    if (g.w >= 4) hipLaunchKernelGGL((bg_median_kernel<KMAX, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((bg_median_kernel<KMAX, false>), grid, block, 0, s, g);
}

} // namespace

extern "C" {

int pdog_bg_samples(const int32_t *h_table, int m, int k, int32_t *out_index, int cap, int *out_n)
{
    if (!h_table || !out_n || m < 1 || k < 1 || k > PDOG_BG_MAX_SAMPLES || cap < 0 || (cap > 0 && !out_index))
        return fail(PDOG_E_ARG, "pdog_bg_samples: bad argument");
    const int n = std::min(k, m);
    *out_n = n;
    if (!out_index) return PDOG_OK; // (cap is 0: the count alone was asked for)
    if (cap < n) return fail(PDOG_E_RANGE, "pdog_bg_samples: room for " + std::to_string(cap) + " of " + std::to_string(n) + " samples");
    for (int i = 0; i < n; ++i) out_index[i] = h_table[(int64_t)i * m / n];
    return PDOG_OK;
}

int pdog_bg_create(int device, int frame_h, int frame_w, pdog_bg **out)
{
    if (!out) return fail(PDOG_E_ARG, "pdog_bg_create: out is null");
    *out = nullptr;
    if (frame_h <= 0 || frame_w <= 0 || ((int64_t)frame_h * ((frame_w + 3) / 4)) > 0x7fff0000LL)
        return fail(PDOG_E_ARG, "pdog_bg_create: bad frame size");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDOG_E_NODEV, "pdog_bg_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(PDOG_E_ARG, "pdog_bg_create: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    pdog_bg *bg = new pdog_bg;
    bg->device = device;
    bg->h = frame_h;
    bg->w = frame_w;
    hipError_t e = bg->d_model.try_reserve((size_t)frame_h * frame_w, nullptr);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&bg->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        pdog_bg_destroy(bg);
        return fail(e == hipErrorOutOfMemory ? PDOG_E_ALLOC : PDOG_E_HIP, std::string("pdog_bg_create: ") + hipGetErrorString(e));
    }
    *out = bg;
    return PDOG_OK;
}

int pdog_bg_destroy(pdog_bg *bg)
{
    if (!bg) return PDOG_OK;
    (void)hipSetDevice(bg->device);
    if (bg->launched) (void)hipStreamSynchronize(bg->last);
    if (bg->ev) (void)hipEventDestroy(bg->ev);
    delete bg;
    return PDOG_OK;
}

int pdog_bg_estimate(pdog_bg *bg, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                     const int32_t *h_samples, int n_samples)
{
    const std::string who = "pdog_bg_estimate";
    if (!bg) return fail(PDOG_E_ARG, who + ": null handle");
    if (!d_frames || !h_samples) return fail(PDOG_E_ARG, who + ": null pointer");
    if (n_samples < 1 || n_samples > PDOG_BG_MAX_SAMPLES)
        return fail(PDOG_E_ARG, who + ": n_samples outside 1 ... " + std::to_string(PDOG_BG_MAX_SAMPLES));
    if (n_frames <= 0 || row_stride < bg->w || frame_stride < 0) return fail(PDOG_E_ARG, who + ": bad size/stride");
    if (int rc = check_entries(who, "sample", h_samples, n_samples, n_frames)) return rc;
    const hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = begin(bg, s)) return rc;
    const int tier = bw_tier(n_samples);
    int32_t padded[BW_MAX_SAMPLES]; // the kernel loads a whole tier without a condition: the last sample repeated behind the list
    for (int k = 0; k < tier; ++k) padded[k] = h_samples[std::min(k, n_samples - 1)];
    if (int rc = stage(bg, s, padded, tier)) return rc;
    BgMedianGeo g;
    g.frames = d_frames;
    g.samples = bg->words.device();
    g.model = bg->d_model.get();
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.h = bg->h;
    g.w = bg->w;
    g.wpr = (bg->w + 3) / 4;
    g.k = n_samples;
    switch (tier) {
    case 8: launch_median<8>(g, s); break;
    case 16: launch_median<16>(g, s); break;
    case 32: launch_median<32>(g, s); break;
    default: launch_median<64>(g, s); break;
    }
    done(bg, s); // (also where the launch failed: the stream has the upload)
    HIP_TRY(hipGetLastError());
    bg->has_model = true;
    return PDOG_OK;
}

int pdog_bg_set(pdog_bg *bg, void *hip_stream, const uint8_t *d_image, int64_t row_stride)
{
    if (!bg) return fail(PDOG_E_ARG, "pdog_bg_set: null handle");
    if (!d_image) return fail(PDOG_E_ARG, "pdog_bg_set: null pointer");
    if (row_stride < bg->w) return fail(PDOG_E_ARG, "pdog_bg_set: bad stride (row_stride < frame width)");
    const hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = begin(bg, s)) return rc;
    HIP_TRY(hipMemcpy2DAsync(bg->d_model.get(), (size_t)bg->w, d_image, (size_t)row_stride, (size_t)bg->w, (size_t)bg->h, hipMemcpyDeviceToDevice, s));
    done(bg, s);
    bg->has_model = true;
    return PDOG_OK;
}

int pdog_bg_get(pdog_bg *bg, void *hip_stream, uint8_t *d_out, int64_t row_stride)
{
    if (!bg) return fail(PDOG_E_ARG, "pdog_bg_get: null handle");
    if (!d_out) return fail(PDOG_E_ARG, "pdog_bg_get: null pointer");
    if (row_stride < bg->w) return fail(PDOG_E_ARG, "pdog_bg_get: bad stride (row_stride < frame width)");
    if (!bg->has_model) return fail(PDOG_E_ARG, "pdog_bg_get: the handle has no model yet (pdog_bg_estimate or pdog_bg_set makes one)");
    const hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = begin(bg, s)) return rc;
    HIP_TRY(hipMemcpy2DAsync(d_out, (size_t)row_stride, bg->d_model.get(), (size_t)bg->w, (size_t)bg->w, (size_t)bg->h, hipMemcpyDeviceToDevice, s));
    done(bg, s);
    return PDOG_OK;
}

int pdog_bg_subtract_indexed(pdog_bg *bg, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                             const int32_t *h_table, int n_steps, uint8_t *d_out, int64_t out_frame_stride, int64_t out_row_stride)
{
    const std::string who = "pdog_bg_subtract_indexed";
    if (!bg) return fail(PDOG_E_ARG, who + ": null handle");
    if (n_frames <= 0 || n_steps < 0) return fail(PDOG_E_ARG, who + ": bad size");
    if (!bg->has_model) return fail(PDOG_E_ARG, who + ": the handle has no model yet (pdog_bg_estimate or pdog_bg_set makes one)");
    if (n_steps == 0) return PDOG_OK;
    if (!d_frames || !h_table || !d_out) return fail(PDOG_E_ARG, who + ": null pointer");
    if (row_stride < bg->w || frame_stride < 0 || out_row_stride < bg->w
        || (n_steps > 1 && out_frame_stride < (int64_t)(bg->h - 1) * out_row_stride + bg->w))
        return fail(PDOG_E_ARG, who + ": bad stride");
    if (int rc = check_entries(who, "table", h_table, n_steps, n_frames)) return rc;
    const hipStream_t s = (hipStream_t)hip_stream;
    if (int rc = begin(bg, s)) return rc;
    if (int rc = stage(bg, s, h_table, n_steps)) return rc;
    BgSubtractGeo g;
    g.frames = d_frames;
    g.model = bg->d_model.get();
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.out_frame_stride = out_frame_stride;
    g.out_row_stride = out_row_stride;
    g.h = bg->h;
    g.w = bg->w;
    g.ppr = (bg->w + 15) / 16;
    const unsigned items = (unsigned)g.h * (unsigned)g.ppr;
    done(bg, s);
    for (int k0 = 0; k0 < n_steps; k0 += kMaxStepsPerLaunch) {
        const int nk = std::min(kMaxStepsPerLaunch, n_steps - k0);
        g.table = bg->words.device() + k0;
        g.out = d_out + (int64_t)k0 * out_frame_stride;
        hipLaunchKernelGGL(bg_subtract_kernel, dim3((items + kBgThreads - 1) / kBgThreads, nk), dim3(kBgThreads), 0, s, g);
        HIP_TRY(hipGetLastError());
    }
    return PDOG_OK;
}

} // extern "C"
