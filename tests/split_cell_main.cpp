// split_cell_main.cpp — pdog_split_cell.hpp (the split rule's cell as one column interval per bitmap row) under the host
// compiler, held to the PER-PIXEL inequality of include/pawsome_split.h, step 5c, in frame coordinates:
//      own  <=>  |x - p|^2 < |x - q|^2, or equal and the target's index is the lower one.
// For R = 2, 3 and 12 every rival offset within +-(2R + 2), for R = 31, 32 and 127 sampled offsets and the axis cases (ej = 0,
// ei = 0, exactly 2R), each with both tie orders, at a position in the frame's corner (rows and columns of the patch outside the
// frame: they take part like any other) and at one inside; then several rivals at once (the intersection stays one interval),
// and span_word's bits against the interval for rows of 1, 2 and 4 words.  tests/test_split_cpu.py builds this plain and with
// -fsanitize=address,undefined and runs it.
#include "pdog_split_cell.hpp"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace pdog::splitcell;

static long long checks = 0, mismatches = 0;
static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;

static int rnd(int lo, int hi) // inclusive
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (int)((rng_state >> 33) % (unsigned long long)(hi - lo + 1));
}

// the header's text, per pixel, in frame coordinates (1-based; p may be a corner: x runs outside the frame)
static bool own_pixel(long long xi, long long xj, long long pi, long long pj, long long qi, long long qj, bool wins)
{
    const long long a = (xi - pi) * (xi - pi) + (xj - pj) * (xj - pj), b = (xi - qi) * (xi - qi) + (xj - qj) * (xj - qj);
    return a < b || (a == b && wins);
}

struct Rival {
    int ei, ej;
    bool wins;
};

static void check_rows(int R, int pi, int pj, const Rival *rv, int n)
{
    const int D = 2 * R + 1, nws = D <= 64 ? 1 : D <= 128 ? 2 : 4;
    for (int dy = -R; dy <= R; ++dy) {
        int lo = -R, hi = R;
        for (int k = 0; k < n; ++k) cut_row(lo, hi, dy, rv[k].ei, rv[k].ej, rv[k].wins);
        for (int dx = -R; dx <= R; ++dx) {
            bool want = true;
            for (int k = 0; k < n; ++k) want = want && own_pixel(pi + dy, pj + dx, pi, pj, pi + rv[k].ei, pj + rv[k].ej, rv[k].wins);
            const bool got = lo <= dx && dx <= hi;
            const int c = dx + R;
            const bool bit = (span_word(lo + R, hi + R, c >> 6) >> (c & 63)) & 1ull;
            ++checks;
            if (got != want || bit != want) {
                if (++mismatches <= 10)
                    std::printf("MISMATCH R %d dy %d dx %d rival0 (%d, %d, %d) of %d: interval %d ... %d, bit %d, want %d\n", R, dy, dx,
                                rv[0].ei, rv[0].ej, (int)rv[0].wins, n, lo, hi, (int)bit, (int)want);
            }
        }
        // nothing past column D - 1, nothing in the words a row does not have
        for (int k = 0; k < 4; ++k) {
            const uint64_t w = span_word(lo + R, hi + R, k);
            uint64_t allowed = 0;
            for (int c = 64 * k; c < 64 * k + 64 && c < D; ++c) allowed |= 1ull << (c - 64 * k);
            ++checks;
            if ((w & ~allowed) || (k >= nws && w)) {
                if (++mismatches <= 10) std::printf("MISMATCH R %d dy %d word %d: bits outside the row\n", R, dy, k);
            }
        }
    }
}

int main()
{
    // floor_div on both signs
    for (int a = -50; a <= 50; ++a)
        for (int b = 1; b <= 9; ++b) {
            int f = a / b;
            while (f * b > a) --f;
            ++checks;
            if (floor_div(a, b) != f) ++mismatches;
        }
    const int corner[2][2] = {{1, 1}, {300, 417}};
    const int small[] = {2, 3, 12}, large[] = {31, 32, 127};
    for (int R : small)
        for (const auto &p : corner)
            for (int ei = -(2 * R + 2); ei <= 2 * R + 2; ++ei)
                for (int ej = -(2 * R + 2); ej <= 2 * R + 2; ++ej)
                    for (int wins = 0; wins < 2; ++wins) {
                        const Rival r{ei, ej, wins != 0};
                        check_rows(R, p[0], p[1], &r, 1);
                    }
    for (int R : large)
        for (const auto &p : corner) {
            const int axis[][2] = {{0, 2 * R}, {0, -2 * R}, {2 * R, 0}, {-2 * R, 0}, {0, 2 * R + 1}, {2 * R + 1, 0}, {0, 0}, {0, 1}, {1, 0}, {-1, -1},
                                   {0, 6}, {4, 4}, {R, R}, {-R, R}, {2 * R + 2, 2 * R + 2}};
            for (const auto &e : axis)
                for (int wins = 0; wins < 2; ++wins) {
                    const Rival r{e[0], e[1], wins != 0};
                    check_rows(R, p[0], p[1], &r, 1);
                }
            for (int s = 0; s < (R == 127 ? 60 : 400); ++s) {
                const Rival r{rnd(-(2 * R + 2), 2 * R + 2), rnd(-(2 * R + 2), 2 * R + 2), rnd(0, 1) != 0};
                check_rows(R, p[0], p[1], &r, 1);
            }
        }
    // several rivals: the rows stay one interval
    for (int R : {3, 12, 31, 32, 127})
        for (int s = 0; s < (R == 127 ? 30 : 300); ++s) {
            Rival rv[31];
            const int n = s % 3 == 0 ? 31 : rnd(2, 6);
            for (int k = 0; k < n; ++k) rv[k] = Rival{rnd(-2 * R, 2 * R), rnd(-2 * R, 2 * R), rnd(0, 1) != 0};
            check_rows(R, 40, 50, rv, n);
        }
    std::printf("%lld checks, %lld mismatches\n", checks, mismatches);
    return mismatches ? 1 : 0;
}
