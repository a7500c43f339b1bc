// pawsome_diag.hip — the diagnostic overlay behind include/pawsome_dog.h (pdog_diag_*): the reference's `Diagnose`
// (src/diagnose.jl:5-38) minus label and video writer, on frames that already live in HBM.
//
// A handle holds what `Diagnose` carries from frame to frame: the colour (:17) and the trace (:20), here the last
// ≤ 99 scaled points before the next call, on the device in two buffers that alternate per call (the overlay kernel of
// a call reads one and writes the other).  The host keeps only their count and which one is current, so a call needs
// no host synchronisation; the ratio (:26-28) is computed per call from its frame size, as update_ratio! does per file.
// With several targets (include/pawsome_overlay.h) each buffer holds one such trace per target; every call adds the same
// number of points to all of them, so one count serves.  A frame table goes up through the handle's StagedUpload.
// The kernels are in dog_diag.hpp; this file uses nothing else of the library.
#include "pdog_host.hpp"
#include "dog_diag.hpp"
#include <algorithm>
#include <cmath>
#include <string>

#pragma clang fp contract(off)

using namespace pdog;

struct pdog_diag {
    int device = 0;
    int color = 255;
    int n_targets = 1;
    DeviceBuffer<int2> d_hist;   // 2 x n_targets x kDiagHist scaled points
    StagedUpload<int32_t> table; // the frame table of the last indexed render
    DeviceBuffer<double> d_lut;  // raw / 255.0 for raw = 0 ... 255
    int cur = 0, hcnt = 0;     // current history buffer, points in each of its traces
    hipStream_t last = nullptr;
    bool launched = false;
    hipEvent_t ev = nullptr;
};

namespace {

constexpr int kMaxFramesPerLaunch = 1 << 15; // resize grid: 57 workgroups per frame

// The launches of a render whose arguments the entry point has checked: n outputs, resize first, then the overlay on top
// (stream order).  h_table == nullptr: output k is frame k and ij one row of positions (pdog_diag_render: the launches it
// always made).  Otherwise output k is frame h_table[k], and ij holds a row per target of the handle, ij_stride positions apart.
int render(pdog_diag *d, hipStream_t s, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int frame_h, int frame_w,
           const int32_t *h_table, int n, const int32_t *d_ij, int64_t ij_stride, uint8_t *d_out)
{
    HIP_TRY(hipSetDevice(d->device));
    if (d->launched && s != d->last) { // the trace state was last touched on another stream: order behind it
        HIP_TRY(hipEventRecord(d->ev, d->last));
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    }
    if (h_table) { // (behind the ordering above: where the device copy grows, draining s also drains its last readers)
        int32_t *stage = nullptr;
        if (int rc = d->table.staging((size_t)n, s, &stage)) return rc;
        std::copy(h_table, h_table + n, stage);
        if (int rc = d->table.send((size_t)n, s)) return rc;
    }
    DiagResizeTableGeo rg;
    rg.frame_stride = frame_stride;
    rg.row_stride = row_stride;
    rg.h = frame_h;
    rg.w = frame_w;
    rg.clamp = frame_h < kDiagH || frame_w < kDiagW; // either axis upsamples
    rg.sy = (double)frame_h / kDiagH;
    rg.offy = 0.5 - rg.sy * 0.5;
    rg.sx = (double)frame_w / kDiagW;
    rg.offx = 0.5 - rg.sx * 0.5;
    DiagOverlayTargetsGeo og;
    og.ij = d_ij;
    og.hist_in = d->d_hist.get() + (size_t)d->cur * d->n_targets * kDiagHist;
    og.hist_out = d->d_hist.get() + (size_t)(d->cur ^ 1) * d->n_targets * kDiagHist;
    og.out = d_out;
    og.n = n;
    og.hcnt = d->hcnt;
    og.h = frame_h;
    og.w = frame_w;
    og.ry = (double)kDiagH / frame_h;
    og.rx = (double)kDiagW / frame_w;
    og.color = d->color;
    og.ij_stride = ij_stride;
    const bool aligned = ((uintptr_t)d_out & 15) == 0;
    const dim3 rt(kDiagResizeThreads);
    const double *lut = d->d_lut.get();
    for (int k0 = 0; k0 < n; k0 += kMaxFramesPerLaunch) {
        const int nk = std::min(kMaxFramesPerLaunch, n - k0);
        const dim3 grid(nk * kDiagBlocksPerFrame);
        rg.out = d_out + (int64_t)k0 * kDiagFrameBytes;
        og.k0 = k0;
        og.write_hist = k0 + nk == n; // once, in the call's last launch
        if (h_table) {
            rg.frames = d_frames;
            rg.table = d->table.device() + k0;
            if (aligned)
                hipLaunchKernelGGL((dog_diag_resize_kernel<true, true>), grid, rt, 0, s, rg, lut);
            else
                hipLaunchKernelGGL((dog_diag_resize_kernel<false, true>), grid, rt, 0, s, rg, lut);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(dog_diag_overlay_targets_kernel, dim3(nk, d->n_targets), dim3(kDiagOverlayThreads), 0, s, og);
        } else {
            rg.frames = d_frames + (int64_t)k0 * frame_stride;
            if (aligned)
                hipLaunchKernelGGL(dog_diag_resize_kernel<true>, grid, rt, 0, s, (const DiagResizeGeo &)rg, lut);
            else
                hipLaunchKernelGGL(dog_diag_resize_kernel<false>, grid, rt, 0, s, (const DiagResizeGeo &)rg, lut);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(dog_diag_overlay_kernel, dim3(nk), dim3(kDiagOverlayThreads), 0, s, (const DiagOverlayGeo &)og);
        }
        HIP_TRY(hipGetLastError());
    }
    d->cur ^= 1;
    d->hcnt = std::min(kDiagHist, d->hcnt + n);
    d->last = s;
    d->launched = true;
    return PDOG_OK;
}

} // namespace

extern "C" {

int pdog_diag_point(int frame_h, int frame_w, const int32_t ij[2], int32_t out[2])
{
    if (!ij || !out || frame_h <= 0 || frame_w <= 0) return fail(PDOG_E_ARG, "pdog_diag_point: bad argument");
    const int i = std::min(std::max((int)ij[0], 1), frame_h), j = std::min(std::max((int)ij[1], 1), frame_w);
    const double ry = (double)kDiagH / frame_h, rx = (double)kDiagW / frame_w; // ratio first (:27), then the product (:31)
    out[0] = (int32_t)std::nearbyint(i * ry);
    out[1] = (int32_t)std::nearbyint(j * rx);
    return PDOG_OK;
}

int pdog_diag_create(int device, int darker_target, pdog_diag **out)
{
    if (!out) return fail(PDOG_E_ARG, "pdog_diag_create: out is null");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PDOG_E_NODEV, "pdog_diag_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(PDOG_E_ARG, "pdog_diag_create: device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    pdog_diag *d = new pdog_diag;
    d->device = device;
    d->color = darker_target ? 255 : 0; // :17
    double lut[256];
    for (int r = 0; r < 256; ++r) lut[r] = r / 255.0;
    hipError_t e = d->d_hist.try_reserve(2 * kDiagHist, nullptr); // one target
    if (e == hipSuccess) e = d->d_lut.try_reserve(256, nullptr);
    if (e == hipSuccess) e = hipMemcpy(d->d_lut.get(), lut, sizeof lut, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&d->ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        pdog_diag_destroy(d);
        return fail(e == hipErrorOutOfMemory ? PDOG_E_ALLOC : PDOG_E_HIP, std::string("pdog_diag_create: ") + hipGetErrorString(e));
    }
    *out = d;
    return PDOG_OK;
}

int pdog_diag_destroy(pdog_diag *d)
{
    if (!d) return PDOG_OK;
    (void)hipSetDevice(d->device);
    if (d->launched) (void)hipStreamSynchronize(d->last);
    if (d->ev) (void)hipEventDestroy(d->ev);
    delete d;
    return PDOG_OK;
}

int pdog_diag_render(pdog_diag *d, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                     int frame_h, int frame_w, int n_frames, const int32_t *d_ij, uint8_t *d_out)
{
    if (!d) return fail(PDOG_E_ARG, "pdog_diag_render: null handle");
    if (d->n_targets != 1) return fail(PDOG_E_ARG, "pdog_diag_render: the handle carries several targets (pdog_diag_render_indexed draws them)");
    if (frame_h <= 0 || frame_w <= 0 || n_frames < 0) return fail(PDOG_E_ARG, "pdog_diag_render: bad size");
    if (n_frames == 0) return PDOG_OK;
    if (!d_frames || !d_ij || !d_out) return fail(PDOG_E_ARG, "pdog_diag_render: null pointer");
    if (row_stride < frame_w || frame_stride < 0) return fail(PDOG_E_ARG, "pdog_diag_render: bad stride");
    return render(d, (hipStream_t)hip_stream, d_frames, frame_stride, row_stride, frame_h, frame_w, nullptr, n_frames, d_ij, 0, d_out);
}

int pdog_diag_set_targets(pdog_diag *d, int n_targets)
{
    if (!d) return fail(PDOG_E_ARG, "pdog_diag_set_targets: null handle");
    if (n_targets < 1 || n_targets > PDOG_DIAG_MAX_TARGETS)
        return fail(PDOG_E_ARG, "pdog_diag_set_targets: n_targets outside 1 ... " + std::to_string(PDOG_DIAG_MAX_TARGETS));
    HIP_TRY(hipSetDevice(d->device));
    // renders queued on the last stream may still use the old state: it is drained before that memory goes
    const int rc = d->d_hist.reserve((size_t)2 * n_targets * kDiagHist, d->launched ? &d->last : nullptr);
    d->n_targets = rc ? 0 : n_targets; // (a failed allocation left no state: every render is refused until a later call succeeds)
    d->hcnt = 0; // nothing inherited: the next render reads no state, and it is ordered behind the last one as every render is
    return rc;
}

int pdog_diag_get_targets(const pdog_diag *d, int *out_n_targets)
{
    if (!d || !out_n_targets) return fail(PDOG_E_ARG, "pdog_diag_get_targets: null argument");
    *out_n_targets = d->n_targets;
    return PDOG_OK;
}

int pdog_diag_render_indexed(pdog_diag *d, void *hip_stream, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                             int frame_h, int frame_w, int n_frames, const int32_t *h_table, int n_steps, const int32_t *d_ij,
                             int64_t ij_target_stride, int n_targets, uint8_t *d_out)
{
    const char *who = "pdog_diag_render_indexed";
    if (!d) return fail(PDOG_E_ARG, std::string(who) + ": null handle");
    if (frame_h <= 0 || frame_w <= 0 || n_frames <= 0 || n_steps < 0) return fail(PDOG_E_ARG, std::string(who) + ": bad size");
    if (n_targets != d->n_targets || n_targets < 1)
        return fail(PDOG_E_ARG, std::string(who) + ": " + std::to_string(n_targets) + " targets, but the handle carries " + std::to_string(d->n_targets));
    if (n_steps == 0) return PDOG_OK;
    if (!d_frames || !h_table || !d_ij || !d_out) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    if (row_stride < frame_w || frame_stride < 0 || ij_target_stride < n_steps) return fail(PDOG_E_ARG, std::string(who) + ": bad stride");
    for (int k = 0; k < n_steps; ++k)
        if (h_table[k] < 0 || h_table[k] >= n_frames)
            return fail(PDOG_E_ARG, std::string(who) + ": table entry " + std::to_string(k) + " is " + std::to_string(h_table[k]) + ", outside 0 ... n_frames-1");
    return render(d, (hipStream_t)hip_stream, d_frames, frame_stride, row_stride, frame_h, frame_w, h_table, n_steps, d_ij, ij_target_stride, d_out);
}

} // extern "C"
