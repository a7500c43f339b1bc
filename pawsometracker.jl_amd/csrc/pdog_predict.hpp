// pdog_predict.hpp — one step of the predicted chain (include/pawsome_predict.h states the rule): the motion rule of
// include/pawsome_motion.h for a group of ONE target with k = 1, where nothing is shared out and nothing is contested.  The
// clamp and the two carry updates are pdog_motion.hpp's, by inclusion, so the one-launch kernels (dog_fused.hpp, dog_roll.hpp)
// and the stepped motion walk they fall back to cannot drift apart.  Plain C++, no HIP, no tracker.
#pragma once
#include "pdog_motion.hpp"

namespace pdog {
namespace predict {

using motion::Carry;
using motion::predict; // clamp(p + v) into 1 ... n, the sum in 64 bits

// What a clip's walk carries from step to step: the position p filed last (the start, as given, before the first step) and
// the velocity and hold count.
struct Walk {
    int32_t pi, pj;
    Carry c;
};
// What a step files (position, state) and the next step's guess, clamp(p' + v').
struct Filed {
    int32_t i, j, state, gi, gj;
};

// Rule 3: the target is assigned iff the window's FP32 maximum EXCEEDS (float)min_response; a NaN fails.
PDOG_HD inline bool assigned(float R, float m_f) { return R > m_f; }

// Rules 3 - 5.  (ci, cj) is the prediction the window was centred on, (qi, qj) the functor's clamped position, which a held
// step does not look at.
PDOG_HD inline Filed step(Walk &w, bool hit, int ci, int cj, int qi, int qj, int coast, int h, int wd)
{
    Filed f;
    if (hit) {
        f.i = qi; f.j = qj; f.state = 1;
        w.c = motion::carry_assigned(w.c, false, w.pi, w.pj, qi, qj);
    } else {
        f.i = ci; f.j = cj; f.state = -1;
        w.c = motion::carry_held(w.c, coast);
    }
    w.pi = f.i; w.pj = f.j;
    f.gi = predict(f.i, w.c.vi, h);
    f.gj = predict(f.j, w.c.vj, wd);
    return f;
}

} // namespace predict
} // namespace pdog
