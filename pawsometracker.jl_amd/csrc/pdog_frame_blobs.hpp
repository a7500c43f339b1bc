// pdog_frame_blobs.hpp — the arithmetic of the frame-blob rule (include/pawsome_frame_blobs.h states it) that needs no GPU:
// the operations on a 64-bit ROW WORD of the mask (bit c = column c of a tile's row), the closed sums of a run of pixels, the
// offsets of the compaction, and the Float64 values derived from a blob's twelve words.  ONE copy for the kernels
// (dog_frame_blobs.hpp), the host entry point (pdog_frame_blobs_derive in pdog_math.cpp) and the host compiler's test
// (tests/frame_blobs_main.cpp).  Plain C++, no HIP: hipcc takes it as host and device code.
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
namespace fblobs {

constexpr int kTile = 64;  // a tile is kTile x kTile pixels: a row of it is one word
constexpr int kWords = 12; // PDOG_FB_WORDS
enum Word { W_N, W_SY, W_SX, W_SYY, W_SYX, W_SXX, W_RMIN, W_RMAX, W_CMIN, W_CMAX, W_FIRST, W_SS };

// The pixel's contrast against the level; in the mask when it reaches min_contrast.
PDOG_HD inline int contrast(int p, int level, bool darker) { return darker ? level - p : p - level; }

// Column of the first pixel of the run of set bits that holds bit c (bit c of m is set).
PDOG_HD inline int run_start(uint64_t m, int c)
{
    const uint64_t below = ~m & ((1ull << c) - 1); // the unset bits below c
    return below ? 64 - __builtin_clzll(below) : 0;
}
// The first bits of the runs of m.
PDOG_HD inline uint64_t run_starts(uint64_t m) { return m & ~(m << 1); }

// THE LINKS BETWEEN A ROW AND THE ROW ABOVE IT that a labelling by runs needs (a run is one node: its pixels are joined
// already).  Bit c of the result is set where pixel (r, c) must be joined with a pixel of row r - 1:
//   links_up     with (r-1, c), at the first column of every stretch in which both rows are set — further columns of the
//                stretch join the same two runs again;
//   links_left   (connectivity 8) with (r-1, c-1), where neither (r-1, c) nor (r, c-1) is set: otherwise that pixel is joined
//                to (r-1, c-1) by a run and an up link;
//   links_right  (connectivity 8) with (r-1, c+1), where neither (r-1, c) nor (r, c+1) is set, alike.
// Neighbours outside the word (column -1 and column 64) belong to another tile: the border merge joins them.
PDOG_HD inline uint64_t links_up(uint64_t m, uint64_t up)
{
    const uint64_t both = m & up;
    return both & ~(both << 1);
}
PDOG_HD inline uint64_t links_left(uint64_t m, uint64_t up) { return m & (up << 1) & ~up & ~(m << 1); }
PDOG_HD inline uint64_t links_right(uint64_t m, uint64_t up) { return m & (up >> 1) & ~up & ~(m >> 1); }

// THE UNION-FIND (pawsome_frame_blobs.h, "how it ends").  load(x) reads x's parent, lower(x, v) stores min(parent of x, v) and
// returns what stood there: relaxed atomics in the kernels, plain memory in the host's test.  A parent never exceeds its node.
// On its way up find hangs every node it passes under its grandparent (path splitting, through `lower`: a parent is only ever
// lowered to an ancestor, and never a root's), so that no later find walks the same chain again.  (On the benchmark's ragged
// blobs it changed nothing measurable — DESIGN.md —: it bounds the chains, it is not what those cases wait for.)
template <class Load, class Lower>
PDOG_HD inline int uf_find(Load load, Lower lower, int x)
{
    int y = load(x);
    while (y < x) { // (y == x: a root.  y > x does not occur; read as a root, the loop still ends)
        const int z = load(y);
        if (z < y) lower(x, z);
        x = y;
        y = z;
    }
    return x;
}
template <class Load, class Lower>
PDOG_HD inline void uf_union(Load load, Lower lower, int a, int b)
{
    for (;;) {
        a = uf_find(load, lower, a);
        b = uf_find(load, lower, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = lower(b, a);
        if (old >= b) return; // b was a root and hangs under a now
        b = old;              // a label below b: on from there
    }
}

// The lowest set bit of `bounds` above bit `lane`, 64 if there is none: where the segment that starts at `lane` ends.
PDOG_HD inline int next_bound(uint64_t bounds, int lane)
{
    const uint64_t above = bounds & ~((2ull << lane) - 1); // (lane 63: 2 << 63 wraps to 0, the mask is all ones)
    return above ? __builtin_ctzll(above) : 64;
}

// The sums of 1, c and c*c over the columns a ... b (0 <= a <= b), closed: c = a + i, i = 0 ... n-1.  The largest product is
// n * a * a: a run of a wave's 64 lanes at column 2^21, the widest row an entry point accepts, stays below 2^49.
PDOG_HD inline void run_sums(int64_t a, int64_t b, int64_t *n, int64_t *sx, int64_t *sxx)
{
    const int64_t m = b - a + 1, t1 = m * (m - 1) / 2, t2 = (m - 1) * m * (2 * m - 1) / 6; // the sums of i and of i * i
    *n = m;
    *sx = m * a + t1;
    *sxx = m * a * a + 2 * a * t1 + t2;
}

// THE COMPACTION'S OFFSETS.  counts[i] kept roots in block i of the raster, blocks in raster order: offsets[i] = the rank of
// block i's first kept root, the return value the number of kept roots.  (The kernel's scan computes the same numbers.)
inline int64_t block_offsets(const int32_t *counts, int n_blocks, int32_t *offsets)
{
    int64_t run = 0;
    for (int i = 0; i < n_blocks; ++i) {
        offsets[i] = (int32_t)run;
        run += counts[i];
    }
    return run;
}

// THE ADMITTED FRAME SIZES (include/pawsome_frame_blobs.h, "Sizes"): nullptr for a size the rule admits, otherwise what of it
// does not fit — the text pdog_fb_create's refusal ends on.  The one blob of a full mask holds the largest words a frame can
// produce: Syy = w * S2(h), Sxx = h * S2(w) and Syx = T(h) * T(w), with S2(k) = (k-1)k(2k-1)/6 and T(k) = k(k-1)/2, and the
// device's 64-bit atomics would wrap without a sign where one of them passes 2^63 - 1.  The checks run in this order, and behind
// the pixel limit both sides are at most 2^30, so that the 128-bit products cannot wrap themselves.
constexpr int64_t kMaxPixels = 1ll << 30;
constexpr int64_t kMaxWidth = 1ll << 21; // PDOG_MAX_ROW_STRIDE: a call's row_stride is at least the frame's width
inline const char *size_refusal(int64_t h, int64_t w)
{
    if (h < 1 || w < 1) return "a side is not positive";
    if ((__int128)h * w > kMaxPixels) return "more than 2^30 pixels";
    if (w > kMaxWidth) return "frame_w exceeds PDOG_MAX_ROW_STRIDE";
    const __int128 most = INT64_MAX;
    const auto s2 = [](__int128 k) { return (k - 1) * k * (2 * k - 1) / 6; };
    const auto t = [](__int128 k) { return k * (k - 1) / 2; };
    if (w * s2(h) > most) return "Syy of a full frame leaves 63 bits";
    if (h * s2(w) > most) return "Sxx of a full frame leaves 63 bits";
    if (t(h) * t(w) > most) return "Syx of a full frame leaves 63 bits";
    return nullptr;
}

constexpr double kPi = 3.14159265358979323846;

// The rule's derived values: pdog_shape.hpp's step 7 on 64-bit sums, rows and columns 0-based in, 1-based out.
inline void derive(const int64_t s[kWords], double out[6])
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const __int128 n = s[W_N], Sy = s[W_SY], Sx = s[W_SX], Syy = s[W_SYY], Syx = s[W_SYX], Sxx = s[W_SXX];
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
    out[0] = 1.0 + (double)Sy / nd;
    out[1] = 1.0 + (double)Sx / nd;
    out[2] = 0.5 * std::atan2(two, dif);
    out[3] = 4.0 * std::sqrt((sum + t) / 2.0);
    out[4] = 4.0 * std::sqrt(lo > 0.0 ? lo : 0.0);
    out[5] = 2.0 * std::sqrt(nd / kPi);
}

} // namespace fblobs
} // namespace pdog
