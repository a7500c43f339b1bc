// Stand-alone host check of the clamped loads of csrc/dog_prune_words.hpp (tests/test_prune_clamp_cpu.py builds and runs it,
// plain and under AddressSanitizer + UBSan): a word of the tile rebuilt from the load at the clamped column and row
// (pw_clamp_col, pw_clamp_row, pw_shift, pw_rebuild32 / 64) against the byte-by-byte statement — the frame's byte where the
// pixel lies inside the frame, 0 elsewhere — and, through pw_words, the substituted words for every mask and fill.  The
// frame is an exact-size heap block per row: a load that leaves the frame's columns is an AddressSanitizer error.
// Exit status 1 on any difference.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "dog_prune_words.hpp"

using namespace pdog;

static uint32_t rng_state = 2468u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static long failures = 0, checks = 0;

struct Frame {
    int fh, fw;
    std::vector<std::unique_ptr<uint8_t[]>> rows; // a block of exactly fw bytes per row
    Frame(int h, int w) : fh(h), fw(w)
    {
        for (int r = 0; r < h; ++r) {
            rows.emplace_back(new uint8_t[(size_t)w]);
            for (int c = 0; c < w; ++c) rows.back()[(size_t)c] = (uint8_t)(1 + rnd() % 255); // never 0: a zero byte is a byte from outside
        }
    }
};

// the statement: byte i of the word at frame row gi, column gj
static uint64_t bytewise(const Frame &f, int gi, int gj, int width)
{
    uint64_t w = 0;
    if (gi < 0 || gi >= f.fh) return 0;
    for (int i = 0; i < width; ++i)
        if (gj + i >= 0 && gj + i < f.fw) w |= (uint64_t)f.rows[(size_t)gi][(size_t)(gj + i)] << (8 * i);
    return w;
}

// the clamped load of `width` bytes and the rebuilt word
static uint64_t clamped(const Frame &f, int gi, int gj, int width)
{
    const int gic = pw_clamp_row(gi, f.fh), gjc = pw_clamp_col(gj, f.fw, width);
    const PwShift s = pw_shift(gjc - gj, width);
    if (width == 4) {
        uint32_t w;
        memcpy(&w, &f.rows[(size_t)gic][(size_t)gjc], 4);
        return pw_rebuild32(w, s);
    }
    uint64_t w;
    memcpy(&w, &f.rows[(size_t)gic][(size_t)gjc], 8);
    return pw_rebuild64(w, s);
}

static void check_word(const Frame &f, int gi, int gj, int width, uint32_t counted, int fill)
{
    const bool rin = gi >= 0 && gi < f.fh;
    const uint64_t want = bytewise(f, gi, gj, width), got = clamped(f, gi, gj, width);
    const uint32_t fill4 = (uint32_t)fill * 0x01010101u;
    for (int h = 0; h < width / 4; ++h) {
        const uint32_t in = rin ? pw_mask(gj + 4 * h, 0, f.fw) : 0u;
        const uint32_t ww = (uint32_t)(want >> (32 * h)), gw = (uint32_t)(got >> (32 * h));
        const PwWords a = pw_words(ww, in, counted, fill4), b = pw_words(gw, in, counted, fill4);
        ++checks;
        // inside the frame's rows the rebuilt word is the statement's whole word wherever any of its bytes lies in the frame
        const bool word_ok = !rin || in == 0u || gw == ww;
        if (!word_ok || a.wz != b.wz || a.wo != b.wo || (gw & in) != (ww & in)) {
            if (++failures <= 20)
                printf("MISMATCH frame %dx%d row %d col %d width %d half %d counted %08x fill %d: word %08x vs %08x, wz %08x vs %08x, wo %08x vs %08x\n",
                       f.fh, f.fw, gi, gj, width, h, counted, fill, gw, ww, b.wz, a.wz, b.wo, a.wo);
        }
    }
}

int main()
{
    const uint32_t masks[] = {0xffffffffu, 0u, 0x000000ffu, 0x0000ff00u, 0x00ff0000u, 0xff000000u, 0x00ffffffu, 0xffffff00u, 0x0000ffffu};
    // frames from the narrowest a load fits into (fw = width) upwards, widths that are no multiple of 4 among them; every
    // column from far left of the frame to far right of it (every clamp distance, |d| ≥ width included), rows above, inside
    // and below
    for (int width : {4, 8})
        for (int fw : {width, width + 1, 11, 16, 83})
            for (int fh : {1, 3}) {
                const Frame f(fh, fw);
                for (int gi = -2; gi <= fh + 1; ++gi)
                    for (int gj = -2 * width - 3; gj <= fw + 2 * width + 3; ++gj)
                        for (uint32_t m : masks) {
                            check_word(f, gi, gj, width, m, 128);
                            check_word(f, gi, gj, width, m, (int)(rnd() & 0xff));
                        }
            }
    // the clamps themselves
    for (int fw : {4, 8, 9, 83})
        for (int width : {4, 8}) {
            if (fw < width) continue;
            for (int gj = -40; gj < fw + 40; ++gj) {
                const int c = pw_clamp_col(gj, fw, width);
                ++checks;
                if (c < 0 || c + width > fw || (gj >= 0 && gj + width <= fw && c != gj)) { ++failures; printf("MISMATCH clamp_col %d fw %d width %d -> %d\n", gj, fw, width, c); }
            }
        }
    for (int fh : {1, 2, 7})
        for (int gi = -9; gi < fh + 9; ++gi) {
            const int r = pw_clamp_row(gi, fh);
            ++checks;
            if (r < 0 || r >= fh || (gi >= 0 && gi < fh && r != gi)) { ++failures; printf("MISMATCH clamp_row %d fh %d -> %d\n", gi, fh, r); }
        }
    printf("prune clamp: %ld checks, %ld mismatches\n", checks, failures);
    return failures ? 1 : 0;
}
