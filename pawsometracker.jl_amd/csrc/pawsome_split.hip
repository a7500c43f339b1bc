// pawsome_split.hip — pdog_blob_split (include/pawsome_split.h): the blob under every target of a set, cut to the target's
// nearest-centre cell.  The kernel is dog_blob.hpp's blob_kernel instantiated with SplitGeo (one copy of every step of the blob
// rule; the cell's row intervals are pdog_split_cell.hpp's); like pawsome_blob.hip this file uses nothing else of the library
// but the tracker's public getters and its device.
#include "pdog_host.hpp"
#include "dog_blob.hpp"
#include "../../include/pawsome_split.h"
#include <cmath>
#include <map>
#include <mutex>
#include <string>

using namespace pdog;

namespace {

int split_disc_pixels(int R)
{
    int n = 0;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) n += dy * dy + dx * dx <= R * R;
    return n;
}

// the workgroup tier's dynamic LDS beyond the default limit, raised once per device (split_lds_bytes, dog_blob.hpp)
int raise_split_lds(size_t bytes)
{
    static std::mutex mu;
    static std::map<int, size_t> limit;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = limit[dev];
    if (bytes <= cur) return PDOG_OK;
    HIP_TRY(hipFuncSetAttribute((const void *)blob_kernel<2, SplitGeo>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    cur = bytes;
    return PDOG_OK;
}

} // namespace

extern "C" int pdog_blob_split(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                               const int32_t *d_frame_index, const int32_t *d_ij, int n_sets, int n_targets, int64_t set_stride,
                               int64_t target_stride, int radius, int min_contrast, int connectivity, int32_t *d_out_sums,
                               double *d_out_shape)
{
    const char *who = "pdog_blob_split";
    const std::string w = who;
    if (!t) return fail(PDOG_E_ARG, w + ": null tracker");
    if (!d_frames || !d_ij) return fail(PDOG_E_ARG, w + ": null pointer");
    if (!d_out_sums && !d_out_shape) return fail(PDOG_E_ARG, w + ": both outputs are null");
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    if (int rc = check_stack(who, info.frame_w, n_frames, row_stride, frame_stride, n_sets >= 0)) return rc;
    if (n_targets < 1 || n_targets > kSplitMaxTargets)
        return fail(PDOG_E_ARG, w + ": n_targets " + std::to_string(n_targets) + " lies outside 1 ... " + std::to_string(kSplitMaxTargets));
    const bool set_major = set_stride == n_targets && target_stride == 1;
    const bool target_major = set_stride == 1 && target_stride == n_sets;
    if (!set_major && !target_major)
        return fail(PDOG_E_ARG, w + ": strides (" + std::to_string(set_stride) + ", " + std::to_string(target_stride) +
                                    ") are neither (n_targets, 1) nor (1, n_sets)");
    if ((long long)n_sets * n_targets > 0x7fffffffll)
        return fail(PDOG_E_ARG, w + ": " + std::to_string((long long)n_sets * n_targets) + " positions are more than 2^31 - 1");
    if (!d_frame_index && n_sets > n_frames)
        return fail(PDOG_E_ARG, w + ": n_sets " + std::to_string(n_sets) + " is more than the " + std::to_string(n_frames) + " frames and there is no frame index");
    if (radius != 0 && (radius < 2 || radius > PDOG_SHAPE_MAX_RADIUS))
        return fail(PDOG_E_ARG, w + ": radius " + std::to_string(radius) + " is neither 0 nor in 2 ... " + std::to_string(PDOG_SHAPE_MAX_RADIUS));
    if (min_contrast < 1 || min_contrast > 255)
        return fail(PDOG_E_ARG, w + ": min_contrast " + std::to_string(min_contrast) + " lies outside 1 ... 255");
    if (connectivity != 4 && connectivity != 8)
        return fail(PDOG_E_ARG, w + ": connectivity " + std::to_string(connectivity) + " is neither 4 nor 8");
    if (n_sets == 0) return PDOG_OK;
    void *stream = nullptr;
    if (int rc = pdog_get_stream(t, &stream)) return rc;
    HIP_TRY(hipSetDevice(peaks_state(t)->device));
    SplitGeo bg;
    ShapeGeo &g = bg.s;
    g.frames = d_frames;
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.frame_index = d_frame_index;
    g.ij = d_ij;
    g.n = n_sets * n_targets;
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
    g.rank = (split_disc_pixels(g.R) - 1) / 2;
    g.out_sums = d_out_sums;
    g.out_shape = d_out_shape;
    bg.eight = connectivity == 8;
    bg.sweeps = nullptr;
    bg.n_sets = n_sets;
    bg.n_targets = n_targets;
    bg.target_major = !set_major;      // (one target or one set: both spellings name the same elements)
    const size_t lds = split_lds_bytes(g.R, g.colbits);
    if (g.R <= 31) {
        hipLaunchKernelGGL((blob_kernel<1, SplitGeo>), dim3((unsigned)g.n), dim3(kShapeThreads), lds, (hipStream_t)stream, bg);
    } else {
        if (lds > 48 * 1024)
            if (int rc = raise_split_lds(lds)) return rc;
        hipLaunchKernelGGL((blob_kernel<2, SplitGeo>), dim3((unsigned)g.n), dim3(kShapeThreads), lds, (hipStream_t)stream, bg);
    }
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}
