// pawsome_diag.hip — the diagnostic overlay behind include/pawsome_dog.h (pdog_diag_*): the reference's `Diagnose`
// (src/diagnose.jl:5-38) minus label and video writer, on frames that already live in HBM.
//
// A handle holds what `Diagnose` carries from frame to frame: the colour (:17) and the trace (:20), here the last
// ≤ 99 scaled points before the next call, on the device in two buffers that alternate per call (the overlay kernel of
// a call reads one and writes the other).  The host keeps only their count and which one is current, so a call needs
// no host synchronisation; the ratio (:26-28) is computed per call from its frame size, as update_ratio! does per file.
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
    DeviceBuffer<int2> d_hist;   // 2 x kDiagHist scaled points
    DeviceBuffer<double> d_lut;  // raw / 255.0 for raw = 0 ... 255
    int cur = 0, hcnt = 0;     // current history buffer, points in it
    hipStream_t last = nullptr;
    bool launched = false;
    hipEvent_t ev = nullptr;
};

namespace {

constexpr int kMaxFramesPerLaunch = 1 << 15; // resize grid: 57 workgroups per frame

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
    hipError_t e = d->d_hist.try_reserve(2 * kDiagHist, nullptr);
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
    if (frame_h <= 0 || frame_w <= 0 || n_frames < 0) return fail(PDOG_E_ARG, "pdog_diag_render: bad size");
    if (n_frames == 0) return PDOG_OK;
    if (!d_frames || !d_ij || !d_out) return fail(PDOG_E_ARG, "pdog_diag_render: null pointer");
    if (row_stride < frame_w || frame_stride < 0) return fail(PDOG_E_ARG, "pdog_diag_render: bad stride");
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(d->device));
    if (d->launched && s != d->last) { // the trace state was last touched on another stream: order behind it
        HIP_TRY(hipEventRecord(d->ev, d->last));
        HIP_TRY(hipStreamWaitEvent(s, d->ev, 0));
    }
    DiagResizeGeo rg;
    rg.frame_stride = frame_stride;
    rg.row_stride = row_stride;
    rg.h = frame_h;
    rg.w = frame_w;
    rg.clamp = frame_h < kDiagH || frame_w < kDiagW; // either axis upsamples
    rg.sy = (double)frame_h / kDiagH;
    rg.offy = 0.5 - rg.sy * 0.5;
    rg.sx = (double)frame_w / kDiagW;
    rg.offx = 0.5 - rg.sx * 0.5;
    DiagOverlayGeo og;
    og.ij = d_ij;
    og.hist_in = d->d_hist.get() + d->cur * kDiagHist;
    og.hist_out = d->d_hist.get() + (d->cur ^ 1) * kDiagHist;
    og.out = d_out;
    og.n = n_frames;
    og.hcnt = d->hcnt;
    og.h = frame_h;
    og.w = frame_w;
    og.ry = (double)kDiagH / frame_h;
    og.rx = (double)kDiagW / frame_w;
    og.color = d->color;
    const bool aligned = ((uintptr_t)d_out & 15) == 0;
    for (int k0 = 0; k0 < n_frames; k0 += kMaxFramesPerLaunch) { // resize first, then the overlay on top (stream order)
        const int nk = std::min(kMaxFramesPerLaunch, n_frames - k0);
        rg.frames = d_frames + (int64_t)k0 * frame_stride;
        rg.out = d_out + (int64_t)k0 * kDiagFrameBytes;
        if (aligned)
            hipLaunchKernelGGL(dog_diag_resize_kernel<true>, dim3(nk * kDiagBlocksPerFrame), dim3(kDiagResizeThreads), 0, s, rg, (const double *)d->d_lut.get());
        else
            hipLaunchKernelGGL(dog_diag_resize_kernel<false>, dim3(nk * kDiagBlocksPerFrame), dim3(kDiagResizeThreads), 0, s, rg, (const double *)d->d_lut.get());
        HIP_TRY(hipGetLastError());
        og.k0 = k0;
        og.write_hist = k0 + nk == n_frames;
        hipLaunchKernelGGL(dog_diag_overlay_kernel, dim3(nk), dim3(kDiagOverlayThreads), 0, s, og);
        HIP_TRY(hipGetLastError());
    }
    d->cur ^= 1;
    d->hcnt = std::min(kDiagHist, d->hcnt + n_frames);
    d->last = s;
    d->launched = true;
    return PDOG_OK;
}

} // extern "C"
