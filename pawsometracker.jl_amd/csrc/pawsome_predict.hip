// pawsome_predict.hip — host side of the predicted chain (include/pawsome_predict.h): the walk is validated here as
// pdog_detect_chains_indexed validates its own, then goes to ONE launch of a predicted instance of the tracker's chain kernels
// (launch_predicted, pawsome_dog.hip: those kernels are named and launched there alone, pdog_host.hpp says why) or, where the
// path choice does not end at such a kernel, to pdog_detect_chains_motion through its public entry point.  What these calls
// keep on a tracker is the PredictState that pawsome_dog.hip hands out.
#include "../../include/pawsome_predict.h"
#include "pdog_host.hpp"

using pdog::fail;

extern "C" int pdog_detect_chains_predicted(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                            int n_frames, const int32_t *h_table, int n_steps, int n_clips, int first,
                                            double min_response, int coast, const int32_t *d_start, int32_t *d_out_ij,
                                            int32_t *d_out_state, int32_t *d_mstate)
{
    const char *who = "pdog_detect_chains_predicted";
    if (!t) return fail(PDOG_E_ARG, std::string(who) + ": null tracker");
    if (!d_frames || !h_table || !d_start || !d_out_ij || !d_out_state) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    if (int rc = pdog::check_motion(who, min_response, coast)) return rc;
    pdog_info info;
    if (int rc = pdog_get_info(t, &info)) return rc;
    pdog::PredictState *ps = pdog::predict_state(t);
    pdog::PredictWalk w{{who, info.frame_w, n_frames, row_stride, frame_stride, h_table, n_steps, n_clips, 1, first, 0, 0}, d_frames,
                        (float)min_response, coast, d_start, d_out_ij, d_out_state, d_mstate};
    if (int rc = pdog::check_table_walk(w.walk, ps->table.len)) return rc;
    if (w.walk.max_len == 0) return PDOG_OK; // no clip has a step

    int taken = 0;
    if (int rc = pdog::launch_predicted(t, w, &taken)) return rc;
    if (taken) return PDOG_OK;
    // The tiled and the stepped geometries, and lengths without an instance: the motion walk with every clip a group of one
    // target and k = 1.  min_distance never matters to one target; min_ratio = 1 makes the ratio test v >= 1 * v, which
    // holds for every response that exceeds min_response.
    const int rc = pdog_detect_chains_motion(t, d_frames, frame_stride, row_stride, n_frames, h_table, n_steps, n_clips, 1, first, 1, 1, 1.0,
                                             min_response, coast, d_start, d_out_ij, d_out_state, d_mstate);
    if (rc == PDOG_OK) ++ps->fallback;
    return rc;
}

extern "C" int pdog_get_predict_counts(pdog_tracker *t, uint64_t out[4])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_predict_counts: null pointer");
    const pdog::PredictState *ps = pdog::predict_state(t);
    out[0] = ps->fused;
    out[1] = ps->persistent;
    out[2] = ps->fallback;
    out[3] = ps->grown;
    return PDOG_OK;
}
