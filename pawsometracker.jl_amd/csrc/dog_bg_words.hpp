// dog_bg_words.hpp — the background model's arithmetic on one dword of four pixels (dog_background.hpp), free of HIP so that a
// host program can hold it against a direct sort (tests/bg_words_main.cpp).  include/pawsome_background.h states the rule.
//
// THE MEDIAN is a bisection on the VALUE, one bit per step from the top, in all four byte lanes at once: with t the bits decided
// so far, the value at 0-based rank r of the K samples sorted ascending is >= t | bit exactly when at least K − r samples are, so
// a step counts the samples that are >= the trial (a byte-lane compare, its result a 0 / 1 per lane added into a word of four
// byte counters; a count is at most 64 and fits its lane) and keeps the bit in the lanes whose count suffices.  After eight
// steps t is that value.  No order among the samples is used, so any order of the frames gives the same bits.
// The samples of a pixel sit in an array of KMAX words, KMAX one of the tiers bw_tier names; the words behind the K-th hold
// 0xff in every lane.  Those rank above or with every sample, so the rank-r value is unchanged, and they pass every compare, so
// the count needed becomes KMAX − r (bw_need).
//
// THE SUBTRACTION clamp(128 + f − b, 0, 255) runs on the even and on the odd bytes as two 16-bit halves each: u = 384 + f − b
// lies in 129 ... 639, so no borrow leaves a half; u − 256 is the unclamped value, bit 9 of u says "above 255" and bits 8 | 9
// "not below 0".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BW_HD __host__ __device__ inline
#else
#define BW_HD inline
#endif
#if defined(__clang__)
#define BW_UNROLL _Pragma("unroll") // (the device's arrays of samples stay in registers only where these loops are unrolled)
#else
#define BW_UNROLL
#endif

namespace pdog {

constexpr uint32_t BW_H = 0x80808080u, BW_L = 0x7f7f7f7fu, BW_EVEN = 0x00ff00ffu, BW_ONES = 0x00010001u;
constexpr int BW_MAX_SAMPLES = 64; // PDOG_BG_MAX_SAMPLES

// 0x80 in every byte lane where a's byte >= b's.  d: the low seven bits compared (bit 7 of a lane of d is set iff a's seven
// are >= b's; a lane of d lies in 1 ... 255, so no borrow leaves it); the top bits decide where they differ.
BW_HD uint32_t bw_ge(uint32_t a, uint32_t b)
{
    const uint32_t d = (a | BW_H) - (b & BW_L);
    return ((a & ~b) | (~(a ^ b) & d)) & BW_H;
}
// the four byte counters after one more compare
BW_HD uint32_t bw_count(uint32_t cnt, uint32_t ge) { return cnt + (ge >> 7); }

// the smallest tier that holds k samples, and the count a lane needs at that tier to keep a bit (r = (k − 1) / 2)
BW_HD int bw_tier(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64; }
BW_HD uint32_t bw_need(int k, int kmax) { return 0x01010101u * (uint32_t)(kmax - (k - 1) / 2); }

// One bisection step over the KMAX words of a pixel quad: bit `b` (7 ... 0) is kept in the lanes where at least need4's count
// of words are >= the trial.
template <int KMAX>
BW_HD uint32_t bw_step(const uint32_t (&x)[KMAX], uint32_t t, int b, uint32_t need4)
{
    const uint32_t trial = t | (0x01010101u << b);
    uint32_t cnt = 0;
    BW_UNROLL
    for (int k = 0; k < KMAX; ++k) cnt = bw_count(cnt, bw_ge(x[k], trial));
    return t | (bw_ge(cnt, need4) >> (7 - b));
}
// the lower median of the first k of KMAX words (the rest 0xffffffff), lane by lane
template <int KMAX>
BW_HD uint32_t bw_median(const uint32_t (&x)[KMAX], int k)
{
    const uint32_t need4 = bw_need(k, KMAX);
    uint32_t t = 0;
    BW_UNROLL
    for (int b = 7; b >= 0; --b) t = bw_step<KMAX>(x, t, b, need4);
    return t;
}

// clamp(128 + f − b, 0, 255) in the two 16-bit halves of e = bytes of f, g = bytes of b (each & BW_EVEN)
BW_HD uint32_t bw_sub2(uint32_t e, uint32_t g)
{
    const uint32_t u = (e + 0x01800180u) - g;                      // 384 + f − b per half
    const uint32_t hi = (u >> 9) & BW_ONES, ok = ((u >> 8) & BW_ONES) | hi;
    return ((u & BW_EVEN) | ((hi << 8) - hi)) & ((ok << 8) - ok);  // 0xff where above 255; 0 where below 0
}
// the same for the four pixels of a dword
BW_HD uint32_t bw_sub4(uint32_t f, uint32_t b)
{
    return bw_sub2(f & BW_EVEN, b & BW_EVEN) | (bw_sub2((f >> 8) & BW_EVEN, (b >> 8) & BW_EVEN) << 8);
}

} // namespace pdog
