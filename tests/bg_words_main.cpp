// The background model's word arithmetic (csrc/dog_bg_words.hpp) held against direct byte arithmetic on the host: the byte-lane
// >= compare and the saturating subtraction for all 256 x 256 byte pairs in every lane (the other lanes holding other pairs), and
// the bisection's median for every K in 1 ... 64 at its tier against a direct sort — all-equal stacks of each of the 256 values,
// stacks of 0 and 255 in every proportion, stacks of few values (ties everywhere), random stacks — rank (K - 1) / 2 per lane.
// Prints "<n> mismatches"; exits non-zero on any.
#include "dog_bg_words.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace pdog;

static long long bad = 0, checks = 0;
static uint32_t rng_state = 20261020u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}
static void expect(bool ok, const char *what, long long a, long long b, long long c)
{
    ++checks;
    if (!ok && bad++ < 20) std::printf("MISMATCH %s (%lld, %lld, %lld)\n", what, a, b, c);
}
static int lane(uint32_t w, int i) { return (int)((w >> (8 * i)) & 0xffu); }

// a stack of k words (lane i of word j = v[i][j]) through the tier's median, against the sort
static void check_median(const uint8_t v[4][BW_MAX_SAMPLES], int k, const char *what)
{
    uint32_t t = 0;
    const int kmax = bw_tier(k);
    auto run = [&](auto &x) {
        const int n = (int)(sizeof x / sizeof x[0]);
        for (int j = 0; j < n; ++j) {
            x[j] = 0xffffffffu;
            if (j < k) x[j] = (uint32_t)v[0][j] | (uint32_t)v[1][j] << 8 | (uint32_t)v[2][j] << 16 | (uint32_t)v[3][j] << 24;
        }
    };
    if (kmax == 8) { uint32_t x[8]; run(x); t = bw_median<8>(x, k); }
    else if (kmax == 16) { uint32_t x[16]; run(x); t = bw_median<16>(x, k); }
    else if (kmax == 32) { uint32_t x[32]; run(x); t = bw_median<32>(x, k); }
    else { uint32_t x[64]; run(x); t = bw_median<64>(x, k); }
    for (int i = 0; i < 4; ++i) {
        uint8_t s[BW_MAX_SAMPLES];
        std::copy(v[i], v[i] + k, s);
        std::sort(s, s + k);
        expect(lane(t, i) == s[(k - 1) / 2], what, k, lane(t, i), s[(k - 1) / 2]);
    }
}

int main()
{
    // the compare, the count and the subtraction: all byte pairs, in every lane
    for (int a = 0; a < 256; ++a)
        for (int b = 0; b < 256; ++b) {
            uint32_t wa = 0, wb = 0;
            int pa[4], pb[4];
            for (int i = 0; i < 4; ++i) {
                pa[i] = (a + 85 * i) & 0xff;
                pb[i] = (b + 51 * i * i) & 0xff;
                wa |= (uint32_t)pa[i] << (8 * i);
                wb |= (uint32_t)pb[i] << (8 * i);
            }
            const uint32_t ge = bw_ge(wa, wb), cnt = bw_count(0x3f003f00u, ge), sub = bw_sub4(wa, wb);
            for (int i = 0; i < 4; ++i) {
                expect(lane(ge, i) == (pa[i] >= pb[i] ? 0x80 : 0), "bw_ge", pa[i], pb[i], i);
                expect(lane(cnt, i) == ((i & 1) ? 0x3f : 0) + (pa[i] >= pb[i]), "bw_count", pa[i], pb[i], i);
                const int d = 128 + pa[i] - pb[i];
                expect(lane(sub, i) == (d < 0 ? 0 : d > 255 ? 255 : d), "bw_sub4", pa[i], pb[i], i);
            }
        }
    for (int k = 1; k <= BW_MAX_SAMPLES; ++k) {
        expect(bw_tier(k) >= k && (bw_tier(k) == 8 || bw_tier(k) / 2 < k), "bw_tier", k, bw_tier(k), 0);
        uint8_t v[4][BW_MAX_SAMPLES];
        for (int val = 0; val < 256; ++val) {            // all-equal, each of the 256 values (the lanes hold four different ones)
            for (int i = 0; i < 4; ++i) std::fill(v[i], v[i] + k, (uint8_t)((val + 64 * i) & 0xff));
            check_median(v, k, "all-equal");
        }
        for (int n255 = 0; n255 <= k; ++n255) {           // 0 / 255 in every proportion, the 255s first, last, and interleaved
            for (int j = 0; j < k; ++j) {
                v[0][j] = j < n255 ? 255 : 0;
                v[1][j] = j >= k - n255 ? 255 : 0;
                v[2][j] = (j * n255) / k != ((j + 1) * n255) / k ? 255 : 0;
                v[3][j] = j < n255 ? 0 : 255;
            }
            check_median(v, k, "0/255");
        }
        for (int rep = 0; rep < 200; ++rep) {             // ties: two to five values, neighbours among them
            const int nv = 2 + rep % 4, base = (int)(rnd() % 252);
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < k; ++j) v[i][j] = (uint8_t)(base + (int)(rnd() % (unsigned)nv));
            check_median(v, k, "ties");
        }
        for (int rep = 0; rep < 400; ++rep) {             // random
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < k; ++j) v[i][j] = (uint8_t)(rnd() >> 11);
            check_median(v, k, "random");
        }
    }
    std::printf("%lld checks, %lld mismatches\n", checks, bad);
    return bad ? 1 : 0;
}
