// Stand-alone host check of csrc/dog_prune_words.hpp (tests/test_prune_words_cpu.py builds and runs it, plain and under
// AddressSanitizer + UBSan): the energies and V that the word helpers give for one band of a tile, dword by dword as
// dog_prune_kernel walks it, against the direct Σ (p − dc)² and max |p − dc| in 64-bit.  Exit status 1 on any difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dog_prune_words.hpp"

using namespace pdog;

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

enum Kind { ZERO, FULL, CHECKER, NOZERO, RANDOM, BRIGHT };
static const char *kind_name[] = {"all-0", "all-255", "0/255", "never-0", "random", "bright"};

static long failures = 0, checks = 0;

// One band: `rows` rows × `width` tile columns; frame columns [f0, f1) hold pixels, the others the fill; the columns
// [lo, hi) are counted.
static void check_band(Kind kind, int rows, int width, int f0, int f1, int lo, int hi, int fill, int dc)
{
    const int nq = (width + 3) / 4;
    std::vector<uint8_t> px((size_t)rows * nq * 4);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < nq * 4; ++c) {
            uint8_t v = 0;
            switch (kind) {
            case ZERO: v = 0; break;
            case FULL: v = 255; break;
            case CHECKER: v = ((r + c) & 1) ? 255 : 0; break;
            case NOZERO: v = (uint8_t)(1 + rnd() % 255); break;
            case RANDOM: v = (uint8_t)(rnd() & 0xff); break;
            case BRIGHT: v = (uint8_t)(140 + rnd() % 100); break;
            }
            px[(size_t)r * nq * 4 + c] = v;
        }
    if (hi > width) hi = width;
    if (lo > hi) lo = hi;
    // direct
    int64_t e_ref = 0, s_ref = 0, v_ref = 0;
    for (int r = 0; r < rows; ++r)
        for (int c = lo; c < hi; ++c) {
            const int p = (c >= f0 && c < f1) ? px[(size_t)r * nq * 4 + c] : fill;
            const int64_t v = p - dc;
            e_ref += v * v;
            s_ref += v;
            if (llabs(v) > v_ref) v_ref = llabs(v);
        }
    // the helpers
    const uint32_t fill4 = (uint32_t)fill * 0x01010101u;
    PwAcc acc = pw_init();
    for (int r = 0; r < rows; ++r)
        for (int q = 0; q < nq; ++q) {
            uint32_t w;
            memcpy(&w, &px[(size_t)r * nq * 4 + 4 * q], 4);
            pw_update(acc, pw_words(w, pw_mask(4 * q, f0, f1), pw_mask(4 * q, lo, hi), fill4));
        }
    const int n = rows * (hi - lo);
    const uint32_t e = pw_energy(acc.s2, acc.s1, n, dc);
    const int s = pw_sum(acc.s1, n, dc);
    const int v = pw_V(pw_pmax(acc), pw_pmin(acc), dc);
    ++checks;
    if ((int64_t)e != e_ref || (int64_t)s != s_ref || (int64_t)v != v_ref) {
        if (++failures <= 20)
            printf("MISMATCH %s rows=%d width=%d frame=[%d,%d) range=[%d,%d) fill=%d dc=%d: E %u vs %lld, sum %d vs %lld, V %d vs %lld\n",
                   kind_name[kind], rows, width, f0, f1, lo, hi, fill, dc, e, (long long)e_ref, s, (long long)s_ref, v, (long long)v_ref);
    }
}

int main()
{
    const Kind kinds[] = {ZERO, FULL, CHECKER, NOZERO, RANDOM, BRIGHT};
    // tile widths that are no multiple of 4, ranges that start at every offset inside a dword, every dc
    for (Kind k : kinds)
        for (int width : {5, 18, 37, 81, 130})
            for (int lo = 0; lo < 4; ++lo)
                for (int dc = 0; dc < 256; dc += (k == RANDOM ? 1 : 15)) {
                    const int hi = lo + 1 + (int)(rnd() % (unsigned)width);
                    check_band(k, 8, width, 0, width, lo, hi, 128, dc);                                   // tile inside the frame
                    check_band(k, 1 + (int)(rnd() % 8), width, (int)(rnd() % 7), width - (int)(rnd() % 7), lo, hi, (int)(rnd() & 0xff), dc); // padding left and right
                }
    // ranges that start anywhere and are one column wide (a remainder column's cut inside a dword)
    for (Kind k : kinds)
        for (int c = 0; c < 21; ++c) check_band(k, 8, 21, 2, 19, c, c + 1, 200, 77);
    // a range with nothing in it
    check_band(RANDOM, 8, 21, 0, 21, 9, 9, 128, 128);
    // the widest slot, l = 149: 8 rows × 212 columns, at the extremes of the 32-bit range
    for (Kind k : kinds)
        for (int dc : {0, 1, 127, 128, 254, 255}) {
            check_band(k, 8, 212, 0, 212, 0, 212, 128, dc);
            check_band(k, 8, 213, 0, 213, 1, 213, 255, dc);
            check_band(k, 8, 215, 3, 100, 3, 215, 0, dc);
        }
    printf("prune words: %ld checks, %ld mismatches\n", checks, failures);
    return failures ? 1 : 0;
}
