// pawsome_blob.hip — pdog_blob (include/pawsome_blob.h): the shape of the connected blob under tracked positions.  The kernel
// is in dog_blob.hpp (its first four steps are dog_shape.hpp's); like pawsome_shape.hip this file uses nothing else of the
// library but the tracker's public getters and its device: no workspace, no counter, no variant.
#include "pdog_host.hpp"
#include "dog_blob.hpp"
#include "../../include/pawsome_blob.h"
#include <cmath>
#include <map>
#include <mutex>
#include <string>

using namespace pdog;

namespace {

// the disc's pixel count: N depends on R only
int blob_disc_pixels(int R)
{
    int n = 0;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) n += dy * dy + dx * dx <= R * R;
    return n;
}

// the workgroup tier's dynamic LDS beyond the default limit, raised once per device (the wave tier stays far below it)
int raise_blob_lds(size_t bytes)
{
    static std::mutex mu;
    static std::map<int, size_t> limit;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = limit[dev];
    if (bytes <= cur) return PDOG_OK;
    HIP_TRY(hipFuncSetAttribute((const void *)blob_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    cur = bytes;
    return PDOG_OK;
}

#ifdef PDOG_ABLATIONS
uint32_t *g_blob_sweeps = nullptr;
#endif

} // namespace

#ifdef PDOG_ABLATIONS
// the ablation build's counter (tools/blob_bench.py): d_sweeps, device [n] uint32 or NULL, receives the sweeps of every
// position of the pdog_blob calls that follow
extern "C" int pdog_blob_debug_sweeps(uint32_t *d_sweeps)
{
    g_blob_sweeps = d_sweeps;
    return PDOG_OK;
}
#endif

extern "C" int pdog_blob(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                         const int32_t *d_frame_index, const int32_t *d_ij, int n, int radius, int min_contrast, int connectivity,
                         int32_t *d_out_sums, double *d_out_shape)
{
    const char *who = "pdog_blob";
    if (!t) return fail(PDOG_E_ARG, "pdog_blob: null tracker");
    if (!d_frames || !d_ij) return fail(PDOG_E_ARG, "pdog_blob: null pointer");
    if (!d_out_sums && !d_out_shape) return fail(PDOG_E_ARG, "pdog_blob: both outputs are null");
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    if (int rc = check_stack(who, info.frame_w, n_frames, row_stride, frame_stride, n >= 0)) return rc;
    if (!d_frame_index && n > n_frames) return fail(PDOG_E_ARG, "pdog_blob: more positions than frames and no frame index");
    if (radius != 0 && (radius < 2 || radius > PDOG_SHAPE_MAX_RADIUS))
        return fail(PDOG_E_ARG, "pdog_blob: radius " + std::to_string(radius) + " is neither 0 nor in 2 ... " + std::to_string(PDOG_SHAPE_MAX_RADIUS));
    if (min_contrast < 1 || min_contrast > 255)
        return fail(PDOG_E_ARG, "pdog_blob: min_contrast " + std::to_string(min_contrast) + " lies outside 1 ... 255");
    if (connectivity != 4 && connectivity != 8)
        return fail(PDOG_E_ARG, "pdog_blob: connectivity " + std::to_string(connectivity) + " is neither 4 nor 8");
    if (n == 0) return PDOG_OK;
    void *stream = nullptr;
    if (int rc = pdog_get_stream(t, &stream)) return rc;
    HIP_TRY(hipSetDevice(peaks_state(t)->device));
    BlobGeo bg;
    ShapeGeo &g = bg.s;
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
    g.rank = (blob_disc_pixels(g.R) - 1) / 2;
    g.out_sums = d_out_sums;
    g.out_shape = d_out_shape;
    bg.eight = connectivity == 8;
    bg.sweeps = nullptr;
#ifdef PDOG_ABLATIONS
    bg.sweeps = g_blob_sweeps;
#endif
    const size_t lds = blob_lds_bytes(g.R, g.colbits);
    if (g.R <= 31) { // a row is one u64: the wave tier
        hipLaunchKernelGGL(blob_kernel<1>, dim3((unsigned)n), dim3(kShapeThreads), lds, (hipStream_t)stream, bg);
    } else {
        if (lds > 48 * 1024)
            if (int rc = raise_blob_lds(lds)) return rc;
        hipLaunchKernelGGL(blob_kernel<2>, dim3((unsigned)n), dim3(kShapeThreads), lds, (hipStream_t)stream, bg);
    }
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}
