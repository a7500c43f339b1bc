// pdog_shape.hpp — the Float64 part of the shape rule (include/pawsome_shape.h states it): the six derived values of a
// position from its eight integer sums (step 7), and the heading of a target over its steps (step 8).  ONE copy for the
// kernel (dog_shape.hpp), the host entry points (pdog_shape_derive, pdog_shape_headings in pdog_math.cpp) and the host
// compiler's test (tests/shape_rule_main.cpp).  Plain C++, no HIP, no tracker: hipcc takes it as host and device code.
//
// Every operation is rounded on its own: contraction is switched off per function (clang; gcc has nothing to contract to on
// the generic x86-64 target and does not know the pragma).  The numerators are exact in int64 and exact as doubles: with
// R <= 127 a disc holds N <= 50 949 pixels and n * Syy <= N * 4.1e8 < 2^53.  atan2, hypot, sin and cos are the math
// library's: the host's and the device's results may differ in their last bits, the integers never do.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef PDOG_HD
#ifdef __HIPCC__
#define PDOG_HD __host__ __device__
#else
#define PDOG_HD
#endif
#endif

namespace pdog {
namespace shape {

constexpr int kMaxRadius = 127; // PDOG_SHAPE_MAX_RADIUS
constexpr double kPi = 3.14159265358979323846;

// Step 7.  s = {n, Sy, Sx, Syy, Syx, Sxx, b, c}, (i, j) the clamped 1-based position; out = {row, col, theta, major, minor, width}.
PDOG_HD inline void derive(const int32_t s[8], int i, int j, double out[6])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const long long n = s[0], Sy = s[1], Sx = s[2], Syy = s[3], Syx = s[4], Sxx = s[5];
    if (n <= 0) {
        for (int k = 0; k < 6; ++k) out[k] = __builtin_nan("");
        return;
    }
    const double nd = (double)n, nn = (double)(n * n);
    const double A = (double)(n * Syy - Sy * Sy), B = (double)(n * Sxx - Sx * Sx), C = (double)(n * Syx - Sy * Sx);
    const double myy = A / nn + 1.0 / 12.0, mxx = B / nn + 1.0 / 12.0, myx = C / nn;
    const double two = 2.0 * myx, dif = mxx - myy, sum = mxx + myy;
    const double t = std::hypot(two, dif);
    const double lo = (sum - t) / 2.0;
    out[0] = (double)i + (double)Sy / nd;
    out[1] = (double)j + (double)Sx / nd;
    out[2] = 0.5 * std::atan2(two, dif);
    out[3] = 4.0 * std::sqrt((sum + t) / 2.0);
    out[4] = 4.0 * std::sqrt(lo > 0.0 ? lo : 0.0);
    out[5] = 2.0 * std::sqrt(nd / kPi);
}

// Step 8 for one step of one target: theta, whether the target moved at least min_step and by what (d_row, d_col), and the
// heading carried so far (has_prev false: none), which a NaN theta leaves alone.
struct Heading {
    bool has_prev = false;
    double prev = 0.0;
};
PDOG_HD inline double heading_step(Heading &h, double theta, bool moved, long long d_row, long long d_col)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    if (theta != theta) return theta;
    bool flip = false;
    if (moved) {
        flip = (double)d_row * std::sin(theta) + (double)d_col * std::cos(theta) < 0.0;
    } else if (h.has_prev) {
        double d = theta - h.prev; // theta in (-pi/2, pi/2], prev in (-pi, pi]: one turn brings d into (-pi, pi]
        if (d > kPi) d -= 2.0 * kPi;
        else if (d <= -kPi) d += 2.0 * kPi;
        flip = std::fabs(d) > kPi / 2.0;
    }
    double out = flip ? theta + kPi : theta;
    if (out > kPi) out -= 2.0 * kPi;
    h.has_prev = true;
    h.prev = out;
    return out;
}
inline void headings(const double *theta, const int32_t *ij, int n_steps, double min_step, double *out)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    Heading h;
    for (int k = 0; k < n_steps; ++k) {
        long long di = 0, dj = 0;
        bool moved = false;
        if (k > 0) {
            di = (long long)ij[2 * k] - ij[2 * k - 2];
            dj = (long long)ij[2 * k + 1] - ij[2 * k - 1];
            moved = (double)di * (double)di + (double)dj * (double)dj >= min_step * min_step;
        }
        out[k] = heading_step(h, theta[k], moved, di, dj);
    }
}

} // namespace shape
} // namespace pdog
