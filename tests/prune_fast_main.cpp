// Stand-alone host check of what the pre-pass's fast paths rest on (csrc/dog_prune_words.hpp; tests/test_prune_fast_cpu.py builds
// and runs it, plain and under AddressSanitizer + UBSan).  Exit status 1 on any difference.
//   extremes    pw_extremes (odd bytes unmasked) against a byte-by-byte maximum / minimum of the counted bytes: all-equal words,
//               0x00 / 0xff in each single byte position beside random others, a million random words with random `counted`
//               masks (none counted among them), single words and runs of words in one accumulator.
//   pair input  ((float)pa − fdc) + ((float)pb − fdc) as pw_centred / pw_pair_input form it against (float)(pa + pb − 2·dc), bit
//               for bit (the sign of zero too), for all 256³ (pa, pb, dc).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "dog_prune_words.hpp"

using namespace pdog;

static uint32_t rng_state = 2463534242u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

static long failures = 0, checks = 0;
static void fail(const char *what, unsigned long long a, unsigned long long b, unsigned long long c)
{
    if (++failures <= 20) printf("MISMATCH %s: %llx %llx %llx\n", what, a, b, c);
}

// ---- extremes ----
struct Ref { int pmax = 0, pmin = 255; }; // (pw_pmax / pw_pmin of nothing counted)
static void ref_add(Ref &r, uint32_t w, uint32_t counted)
{
    for (int i = 0; i < 4; ++i)
        if ((counted >> (8 * i)) & 0xffu) {
            const int p = (int)((w >> (8 * i)) & 0xffu);
            if (p > r.pmax) r.pmax = p;
            if (p < r.pmin) r.pmin = p;
        }
}
static void check_acc(const char *what, const PwAcc &a, const Ref &r, uint32_t w, uint32_t counted)
{
    ++checks;
    if (pw_pmax(a) != r.pmax || pw_pmin(a) != r.pmin) fail(what, w, counted, ((unsigned long long)pw_pmax(a) << 24) | ((unsigned long long)pw_pmin(a) << 16) | ((unsigned)r.pmax << 8) | (unsigned)r.pmin);
}
// one word alone under `counted`
static void check_word(uint32_t w, uint32_t counted)
{
    const uint32_t fill4 = 0x80808080u;
    {
        PwAcc a = pw_init();
        Ref r;
        pw_extremes(a, pw_words(w, 0xffffffffu, counted, fill4));
        ref_add(r, w, counted);
        check_acc("general", a, r, w, counted);
    }
}
static uint32_t random_mask() { return ((rnd() & 1u) ? 0xffu : 0u) | ((rnd() & 1u) ? 0xff00u : 0u) | ((rnd() & 1u) ? 0xff0000u : 0u) | ((rnd() & 1u) ? 0xff000000u : 0u); }

static void check_extremes()
{
    for (uint32_t v = 0; v < 256; ++v) // all-equal words
        for (uint32_t counted : {0xffffffffu, 0x000000ffu, 0x0000ff00u, 0x00ff0000u, 0xff000000u, 0x00ffff00u, 0u}) check_word(v * 0x01010101u, counted);
    for (int pos = 0; pos < 4; ++pos) // 0x00 / 0xff in one byte position beside random others
        for (uint32_t ext : {0x00u, 0xffu})
            for (int n = 0; n < 4096; ++n) {
                const uint32_t w = (rnd() & ~(0xffu << (8 * pos))) | (ext << (8 * pos));
                check_word(w, 0xffffffffu);
                check_word(w, random_mask());
                check_word(w, 0xffu << (8 * pos));    // only the extreme byte counted
                check_word(w, ~(0xffu << (8 * pos))); // every byte but it
            }
    for (int n = 0; n < 1000000; ++n) { // random words, random masks (none counted among them)
        const uint32_t w = rnd();
        check_word(w, random_mask());
        check_word(w, 0xffffffffu);
    }
    // runs: one accumulator over many words
    for (int run = 0; run < 20000; ++run) {
        PwAcc a = pw_init();
        Ref r;
        const int len = 1 + (int)(rnd() % 40u);
        const uint32_t lo = rnd() & 0xffu, span = 1u + (rnd() & 0xffu); // (narrow ranges: the extremes move late in a run)
        uint32_t w = 0, counted = 0;
        for (int j = 0; j < len; ++j) {
            w = 0;
            for (int i = 0; i < 4; ++i) w |= ((lo + rnd() % span) & 0xffu) << (8 * i);
            counted = (rnd() & 3u) ? 0xffffffffu : random_mask();
            pw_extremes(a, pw_words(w, 0xffffffffu, counted, 0x80808080u));
            ref_add(r, w, counted);
        }
        check_acc("run", a, r, w, counted);
    }
}

// ---- pair input ----
static void check_pairs()
{
    for (int dc = 0; dc < 256; ++dc) {
        const float fdc = (float)dc;
        float c[256];
        for (int p = 0; p < 256; ++p) c[p] = pw_centred((uint32_t)p, fdc);
        for (int pa = 0; pa < 256; ++pa)
            for (int pb = 0; pb < 256; ++pb) {
                const float got = pw_pair_input(c[pa], c[pb]), want = (float)(pa + pb - 2 * dc);
                uint32_t gb, wb;
                memcpy(&gb, &got, 4);
                memcpy(&wb, &want, 4);
                ++checks;
                if (gb != wb) fail("pair", (unsigned)pa, (unsigned)pb, (unsigned)dc);
            }
        for (int p = 0; p < 256; ++p) { // the centre tap's input
            const float want = (float)(p - dc);
            ++checks;
            if (memcmp(&c[p], &want, 4) != 0) fail("centre", (unsigned)p, (unsigned)dc, 0);
        }
    }
}

int main()
{
    check_extremes();
    check_pairs();
    printf("prune fast paths: %ld checks, %ld mismatches\n", checks, failures);
    return failures ? 1 : 0;
}
