// pdog_motion.hpp — the pieces of the motion step's rule (include/pawsome_motion.h) that the kernel (dog_motion.hpp) and the
// host function (pdog_assign_motion_host, pdog_math.cpp) must agree on to the bit: which list entries are admissible, how far
// an entry lies from the prediction, where a prediction is clamped, and what an assigned and a held target carry to the next
// step.  When one position blocks another and the order among equal distances are pdog_exclusive.hpp's, by inclusion.  Plain
// C++, no HIP, no tracker: the host compiler takes it as it is (tests/motion_main.cpp), hipcc as host and device code.
#pragma once
#include "pdog_exclusive.hpp"

namespace pdog {
namespace motion {

using exclusive::blocks;
using exclusive::head_key;
using exclusive::key_target;
using exclusive::kMaxTargets; // PDOG_MOTION_MAX_TARGETS: the same half wave

constexpr uint32_t kFar = 0xffffffffu; // D of an entry 65536 or more rows or columns from the prediction, and the cap of every D

// Entry q of a list with `count` entries, value v, pick 1's value v0.  Pick 1 is NOT exempt from the two value tests (it is
// from the count: the functor's answer exists whatever the count says).  rho_f * v0 is ONE FP32 multiplication; a NaN on
// either side fails the comparisons.
PDOG_HD inline bool admissible(int q, int count, float v, float v0, float m_f, float rho_f)
{
    return (q == 0 || q < count) && v > m_f && v >= rho_f * v0;
}

// D: the squared integer distance from (i, j) to the prediction (ci, cj) as an unsigned 32-bit number, for any int32 input.
PDOG_HD inline uint32_t dist2(int i, int j, int ci, int cj)
{
    const long long di = (long long)i - ci, dj = (long long)j - cj;
    if (di >= 65536 || di <= -65536 || dj >= 65536 || dj <= -65536) return kFar;
    const unsigned long long s = (unsigned long long)(di * di) + (unsigned long long)(dj * dj); // each square < 2^32
    return s > kFar ? kFar : (uint32_t)s;
}

// clamp(p + v) into 1 ... n along one axis (n >= 1), the sum in 64 bits.
PDOG_HD inline int predict(int p, int v, int n)
{
    const long long x = (long long)p + v;
    return x < 1 ? 1 : x > n ? n : (int)x;
}

// What a target carries from step to step beside its position.
struct Carry {
    int32_t vi, vj, n_held;
};

// An assigned target: n_held' = 0; v' = p' - p unless the target is contested, in which case it keeps v.  (The difference
// wraps modulo 2^32: positions inside a frame never get there, and no input is undefined behaviour.)
PDOG_HD inline Carry carry_assigned(Carry c, bool contested, int pi, int pj, int ni, int nj)
{
    if (!contested) {
        c.vi = (int32_t)((uint32_t)ni - (uint32_t)pi);
        c.vj = (int32_t)((uint32_t)nj - (uint32_t)pj);
    }
    c.n_held = 0;
    return c;
}

// A held target: n_held' = n_held + 1 (it stays at INT32_MAX once there); v' = v while n_held' < coast, (0, 0) from then on.
PDOG_HD inline Carry carry_held(Carry c, int coast)
{
    c.n_held = c.n_held < 0x7fffffff ? c.n_held + 1 : 0x7fffffff;
    if (!(c.n_held < coast)) c.vi = c.vj = 0;
    return c;
}

} // namespace motion
} // namespace pdog
