// pawsome_shape.hip — pdog_shape (include/pawsome_shape.h): how a target lies at tracked positions.  The kernel is in
// dog_shape.hpp; this file uses nothing else of the library but the tracker's public getters (frame size, fill,
// darker_target, target_width, stream) and its device (peaks_state, pdog_host.hpp): no workspace, no counter, no variant.
// The two host-only entry points of the header, pdog_shape_derive and pdog_shape_headings, are pdog_math.cpp's.
#include "pdog_host.hpp"
#include "dog_shape.hpp"
#include "../../include/pawsome_shape.h"
#include <cmath>
#include <map>
#include <mutex>
#include <string>

using namespace pdog;

namespace {

// the disc's pixel count for every radius, once: N depends on R only
int disc_pixels(int R)
{
    int n = 0;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) n += dy * dy + dx * dx <= R * R;
    return n;
}

// the kernel's dynamic LDS beyond the default limit, raised once per device
int raise_shape_lds(size_t bytes)
{
    static std::mutex mu;
    static std::map<int, size_t> limit;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = limit[dev];
    if (bytes <= cur) return PDOG_OK;
    HIP_TRY(hipFuncSetAttribute((const void *)shape_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    cur = bytes;
    return PDOG_OK;
}

} // namespace

extern "C" int pdog_shape(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                          const int32_t *d_frame_index, const int32_t *d_ij, int n, int radius, int min_contrast,
                          int32_t *d_out_sums, double *d_out_shape)
{
    const char *who = "pdog_shape";
    if (!t) return fail(PDOG_E_ARG, "pdog_shape: null tracker");
    if (!d_frames || !d_ij) return fail(PDOG_E_ARG, "pdog_shape: null pointer");
    if (!d_out_sums && !d_out_shape) return fail(PDOG_E_ARG, "pdog_shape: both outputs are null");
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    if (int rc = check_stack(who, info.frame_w, n_frames, row_stride, frame_stride, n >= 0)) return rc;
    if (!d_frame_index && n > n_frames) return fail(PDOG_E_ARG, "pdog_shape: more positions than frames and no frame index");
    if (radius != 0 && (radius < 2 || radius > PDOG_SHAPE_MAX_RADIUS))
        return fail(PDOG_E_ARG, "pdog_shape: radius " + std::to_string(radius) + " is neither 0 nor in 2 ... " + std::to_string(PDOG_SHAPE_MAX_RADIUS));
    if (min_contrast < 1 || min_contrast > 255)
        return fail(PDOG_E_ARG, "pdog_shape: min_contrast " + std::to_string(min_contrast) + " lies outside 1 ... 255");
    if (n == 0) return PDOG_OK;
    void *stream = nullptr;
    if (int rc = pdog_get_stream(t, &stream)) return rc;
    HIP_TRY(hipSetDevice(peaks_state(t)->device));
    ShapeGeo g;
    g.frames = d_frames;
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.frame_index = d_frame_index;
    g.ij = d_ij;
    g.n = n;
    g.fh = info.frame_h;
    g.fw = info.frame_w;
    g.fill = info.fill;
    g.darker = info.darker_target;
    g.R = radius;
    if (radius == 0) { // the default: ceil(target_width), within the rule's range
        const double tw = std::ceil(info.target_width);
        g.R = tw >= PDOG_SHAPE_MAX_RADIUS ? PDOG_SHAPE_MAX_RADIUS : tw <= 2 ? 2 : (int)tw;
    }
    g.min_contrast = min_contrast;
    const int D = 2 * g.R + 1;
    g.colbits = 3;
    while ((1 << g.colbits) < D) ++g.colbits;
    g.rank = (disc_pixels(g.R) - 1) / 2;
    g.out_sums = d_out_sums;
    g.out_shape = d_out_shape;
    const size_t lds = sizeof(uint32_t) * (size_t)shape_tile_words(g.R);
    if (lds > 48 * 1024)
        if (int rc = raise_shape_lds(lds)) return rc;
    hipLaunchKernelGGL(shape_kernel, dim3((unsigned)n), dim3(kShapeThreads), lds, (hipStream_t)stream, g);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}
