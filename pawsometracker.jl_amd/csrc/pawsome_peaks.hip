// pawsome_peaks.hip — host side of pdog_detect_peaks (include/pawsome_peaks.h): the tracker's normal batch path with the
// response map, through its public entry point, and the selection kernel (dog_peaks.hpp) behind it on the same stream.  No
// kernel of the tracker is named here; what this call keeps on a tracker (scratch, the "peaks_no_list" switch, the counters)
// is the PeaksState that pawsome_dog.hip hands out.
#include "../../include/pawsome_peaks.h"
#include "pdog_host.hpp"
#include "dog_peaks.hpp"

#include <algorithm>
#include <cmath>

using pdog::fail;
using namespace pdog::peaks;
static_assert(PEAKS_MAX_K == PDOG_PEAKS_MAX_K, "the kernel's pick slots follow the header");

extern "C" int pdog_detect_peaks(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                                 const int32_t *d_frame_index, const int32_t *d_guesses, int n, int k, int min_distance,
                                 int32_t *d_out_ij, float *d_out_peak, int32_t *d_out_count, float *d_out_resp)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_detect_peaks: null tracker");
    if (k < 1 || k > PDOG_PEAKS_MAX_K) return fail(PDOG_E_ARG, "pdog_detect_peaks: k = " + std::to_string(k) + " lies outside 1 ... " + std::to_string(PDOG_PEAKS_MAX_K));
    if (n == 0) return PDOG_OK;
    if (!d_frames || !d_guesses || !d_out_ij) return fail(PDOG_E_ARG, "pdog_detect_peaks: null pointer");
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    if (int rc = pdog::check_stack("pdog_detect_peaks", info.frame_w, n_frames, row_stride, frame_stride, n >= 0)) return rc;
    if (!d_frame_index && n > n_frames) return fail(PDOG_E_ARG, "pdog_detect_peaks: more windows than frames and no frame index");
    if ((long long)n * info.n_strips > 0x7ffffff0LL) return fail(PDOG_E_ARG, "pdog_detect_peaks: batch too large");
    const long long md = min_distance > 0 ? min_distance : std::max(1LL, (long long)std::ceil(info.target_width));

    pdog::PeaksState *ps = pdog::peaks_state(t);
    void *sp = nullptr;
    if (int rc = pdog_get_stream(t, &sp)) return rc;
    const hipStream_t stream = (hipStream_t)sp;
    HIP_TRY(hipSetDevice(ps->device));
    const size_t per_win = (size_t)info.win_h * info.win_w;
    // the maps: the caller's buffer takes the whole batch; the tracker's scratch takes what PDOG_MAP_MB holds, one window at least
    const int chunk = d_out_resp ? n : (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ps->map_cap / (per_win * sizeof(float))));
    if (!d_out_resp)
        if (int rc = ps->d_map.reserve((size_t)chunk * per_win, &stream)) return rc;
    if (int rc = ps->d_ij1.reserve((size_t)2 * n, &stream)) return rc;
    if (int rc = ps->d_stat.reserve(2, &stream, true)) return rc;

    PeaksGeo g;
    g.md2 = md * md;
    g.n1 = info.win_h; g.n2 = info.win_w; g.r1 = info.radius_h; g.r2 = info.radius_w;
    g.fh = info.frame_h; g.fw = info.frame_w; g.k = k; g.no_list = ps->no_list ? 1 : 0;
    g.stat = ps->d_stat.get();
    for (int lo = 0; lo < n; lo += chunk) {
        const int m = std::min(chunk, n - lo);
        float *maps = d_out_resp ? d_out_resp + (size_t)lo * per_win : ps->d_map.get();
        // without a frame index window b looks at frame b: the chunk's frames start at frame lo
        const int rc = pdog_detect_batch(t, d_frame_index ? d_frames : d_frames + (int64_t)lo * frame_stride, frame_stride, row_stride,
                                         d_frame_index ? n_frames : n_frames - lo, d_frame_index ? d_frame_index + lo : nullptr,
                                         d_guesses + 2 * (size_t)lo, m, ps->d_ij1.get() + 2 * (size_t)lo, maps);
        if (rc) return rc;
        g.resp = maps;
        g.guesses = d_guesses + 2 * (size_t)lo;
        g.ij1 = ps->d_ij1.get() + 2 * (size_t)lo;
        g.out_ij = d_out_ij + 2 * (size_t)lo * k;
        g.out_peak = d_out_peak ? d_out_peak + (size_t)lo * k : nullptr;
        g.out_count = d_out_count ? d_out_count + lo : nullptr;
        hipLaunchKernelGGL(dog_peaks_kernel, dim3(m), dim3(PEAKS_NT), 0, stream, g);
        HIP_TRY(hipGetLastError());
    }
    return PDOG_OK;
}

extern "C" int pdog_get_peaks_counts(pdog_tracker *t, uint64_t out[2])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_peaks_counts: null pointer");
    if (int rc = pdog_sync(t)) return rc;
    pdog::PeaksState *ps = pdog::peaks_state(t);
    unsigned long long v[2] = {0, 0};
    if (ps->d_stat.get()) {
        HIP_TRY(hipSetDevice(ps->device));
        HIP_TRY(hipMemcpy(v, ps->d_stat.get(), sizeof v, hipMemcpyDeviceToHost));
    }
    out[0] = (uint64_t)v[0];
    out[1] = (uint64_t)v[1];
    return PDOG_OK;
}
