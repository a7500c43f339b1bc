// pdog_split_cell.hpp — the nearest-centre cell of the split rule (include/pawsome_split.h, step 5c) as ONE COLUMN INTERVAL PER
// BITMAP ROW, for the host and the device alike: no HIP header, nothing of the library.  dog_blob.hpp's split instances cut their
// mask rows with these and with nothing else; tests/split_cell_main.cpp holds them to the per-pixel inequality under the host
// compiler and its sanitizers.
//
// Everything is relative to the target's own clamped position p: a patch pixel is (dy, dx), -R <= dy, dx <= R, and a rival is
// e = q - p = (ei, ej), both clamped positions.  The pixel is the target's against that rival if
//      |x - p|^2 < |x - q|^2   <=>   ej (2 dx - ej) + ei (2 dy - ei) < 0,
// or if the two sides are equal and the target wins the tie (its index is the lower one).  On the row dy that is
//      2 ej dx <= T,   T = ej^2 - ei (2 dy - ei) - (wins ? 0 : 1),
// a half-line of columns: dx <= floor(T / 2ej) for ej > 0, dx >= -floor(T / (-2ej)) for ej < 0 (the ceiling of a quotient is
// minus the floor of its negative), and for ej = 0 the whole row (0 <= T) or none of it.  The cell is the intersection of these
// half-planes over the rivals, so a row holds one interval.  |ei|, |ej| <= 2R + 2 <= 256 and |dy|, |dx| <= 127 keep every
// product below 2^20: plain int.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDOG_SPLIT_HD __host__ __device__ inline
#else
#define PDOG_SPLIT_HD inline
#endif

namespace pdog {
namespace splitcell {

// floor(a / b) for b > 0 and any a (C++ division truncates towards zero)
PDOG_SPLIT_HD int floor_div(int a, int b)
{
    const int q = a / b;
    return q - (a % b < 0);
}

// Cuts the interval lo ... hi (inclusive, in dx; empty when lo > hi) of the row dy down to the rival's half-plane.
PDOG_SPLIT_HD void cut_row(int &lo, int &hi, int dy, int ei, int ej, bool wins_ties)
{
    const int T = ej * ej - ei * (2 * dy - ei) - (wins_ties ? 0 : 1);
    if (ej > 0) {
        const int v = floor_div(T, 2 * ej);
        hi = v < hi ? v : hi;
    } else if (ej < 0) {
        const int v = -floor_div(T, -2 * ej);
        lo = v > lo ? v : lo;
    } else if (T < 0) {
        lo = 1;
        hi = 0;
    }
}

// Word k of a row bitmap (bit x & 63 of word x >> 6 for column x) with the columns c0 ... c1 set; 0 <= c0, and nothing when
// c0 > c1.
PDOG_SPLIT_HD uint64_t span_word(int c0, int c1, int k)
{
    const int a = c0 - 64 * k, b = c1 - 64 * k;         // the span in this word's own bit numbers
    if (c0 > c1 || b < 0 || a > 63) return 0;
    const uint64_t from = a <= 0 ? ~0ull : ~0ull << a;
    const uint64_t to = b >= 63 ? ~0ull : (1ull << (b + 1)) - 1ull;
    return from & to;
}

} // namespace splitcell
} // namespace pdog
