// dog_prune_words.hpp — the pre-pass's arithmetic on one dword of four pixels (dog_prune.hpp), free of HIP so that a host
// program can hold it against the direct sums (tests/prune_words_main.cpp).
//
// The energy of a set of n pixels about the window's DC level comes from the raw pixels' moments, exactly, in integers:
//     Σ (p − dc)² = Σ p² − 2·dc·Σ p + n·dc²,          Σ (p − dc) = Σ p − n·dc,
// and V = max |p − dc| = max(pmax − dc, dc − pmin).  Per dword the device forms Σ p² and Σ p with one v_dot4_u32_u8 each
// and the four bytes' maxima and minima as two packed 16-bit halves each (the even bytes in place, the odd bytes left in
// the high byte of their half: a common factor of 256 does not change an order, so no shift is needed).
//
// A dword is counted through two substituted words (pw_words):
//     wz — what the sums and the maximum see: the frame's byte where the pixel lies inside the frame, the fill where it lies
//          outside the frame but inside the tile, 0 where the pixel is not counted at all (a column at or past the tile's width
//          or outside the column range asked for, a row at or past the tile's height);
//     wo — what the minimum sees: the same, with 0xff for the bytes that are not counted, so that they never are the minimum
//          (a zeroed byte on a bright window would give a wrong V).
// n is geometry (rows × columns counted), never counted at run time.
//
// RANGE.  The widest slot, at l = 149, is 8 rows × 212 columns: Σ p² ≤ 1696·255² ≈ 1.11e8, n·dc² likewise, 2·dc·Σ p ≤ 2.21e8;
// a dword's 8-row sums are far smaller.  pw_energy adds before it subtracts: every intermediate lies in [0, 2.21e8] < 2³².
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PW_HD __host__ __device__ inline
#else
#define PW_HD inline
#endif

namespace pdog {

// 0xff in byte i iff column col0 + i lies in [lo, hi)
PW_HD uint32_t pw_low_bytes(int n) { return n >= 4 ? 0xffffffffu : n <= 0 ? 0u : (1u << (8 * n)) - 1u; } // 0xff in the bytes below n
PW_HD uint32_t pw_mask(int col0, int lo, int hi) { return pw_low_bytes(hi - col0) & ~pw_low_bytes(lo - col0); }

// The substituted words of one loaded dword.  in_frame: the bytes whose pixel lies inside the frame (w is read there only);
// counted: the bytes that are counted at all.
struct PwWords { uint32_t wz, wo; };
PW_HD PwWords pw_words(uint32_t w, uint32_t in_frame, uint32_t counted, uint32_t fill4)
{
    const uint32_t keep = in_frame & counted;
    const uint32_t z = (w & keep) | (fill4 & counted & ~keep);
    return PwWords{z, z | ~counted};
}

// CLAMPED LOADS.  A word of the tile that hangs over the frame's left or right edge is not read byte by byte: the load starts
// at the asked column clamped into [0, fw − width] (pw_clamp_col; the row likewise into [0, fh − 1], pw_clamp_row), so every
// byte read lies in a row of the frame at a column of the frame, and the tile's word is the loaded one shifted by the clamp
// distance d = clamped − asked column (pw_shift, pw_rebuild32 / 64): d > 0 (over the left edge) moves the bytes up, d < 0
// (over the right edge) down, and zeros come in where the column lies outside the frame.  Where |d| ≥ width no byte of the
// word lies inside the frame (its in-frame mask is 0) and the rebuilt word is not specified.  Needs fw ≥ width.
PW_HD int pw_clamp_col(int gj, int fw, int width) { return gj < 0 ? 0 : gj > fw - width ? fw - width : gj; }
PW_HD int pw_clamp_row(int gi, int fh) { return gi < 0 ? 0 : gi > fh - 1 ? fh - 1 : gi; }
struct PwShift { unsigned up, down; }; // bits
PW_HD PwShift pw_shift(int d, int width)
{
    const int m = width - 1, u = d > m ? m : d, n = -d > m ? m : -d;
    return PwShift{d > 0 ? 8u * (unsigned)u : 0u, d < 0 ? 8u * (unsigned)n : 0u};
}
PW_HD uint32_t pw_rebuild32(uint32_t w, PwShift s) { return (w << s.up) >> s.down; }
PW_HD uint64_t pw_rebuild64(uint64_t w, PwShift s) { return (w << s.up) >> s.down; }

#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short pw_us2 __attribute__((ext_vector_type(2)));
PW_HD uint32_t pw_dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }
PW_HD uint32_t pw_pk_max(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(pw_us2, a), __builtin_bit_cast(pw_us2, b)));
}
PW_HD uint32_t pw_pk_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(pw_us2, a), __builtin_bit_cast(pw_us2, b)));
}
PW_HD uint32_t pw_mul24(uint32_t a, uint32_t b) { return __umul24(a, b); } // a, b < 2²⁴
PW_HD float pw_sqrt_est(float x) { return __builtin_amdgcn_sqrtf(x); }
#else
PW_HD uint32_t pw_mul24(uint32_t a, uint32_t b) { return a * b; }
PW_HD float pw_sqrt_est(float x) { return __builtin_sqrtf(x); }
PW_HD uint32_t pw_dot4(uint32_t a, uint32_t b, uint32_t c)
{
    for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xffu) * ((b >> (8 * i)) & 0xffu);
    return c;
}
PW_HD uint32_t pw_pk_max(uint32_t a, uint32_t b)
{
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al : bl) | ((ah > bh ? ah : bh) << 16);
}
PW_HD uint32_t pw_pk_min(uint32_t a, uint32_t b)
{
    const uint32_t al = a & 0xffffu, bl = b & 0xffffu, ah = a >> 16, bh = b >> 16;
    return (al < bl ? al : bl) | ((ah < bh ? ah : bh) << 16);
}
#endif

constexpr uint32_t PW_EVEN = 0x00ff00ffu, PW_ODD = 0xff00ff00u;

// Σ p², Σ p and the packed extremes of the pixels counted so far
struct PwAcc {
    uint32_t s2, s1;
    uint32_t max_e, max_o, min_e, min_o; // two 16-bit halves each: the even bytes; the odd bytes in the halves' high bytes (the low bytes: anything)
};
PW_HD PwAcc pw_init() { return PwAcc{0u, 0u, 0u, 0u, PW_EVEN, PW_ODD}; }

// the sums of one dword: two dot instructions
PW_HD void pw_moments(uint32_t &s2, uint32_t &s1, uint32_t wz)
{
    s2 = pw_dot4(wz, wz, s2);
    s1 = pw_dot4(wz, 0x01010101u, s1);
}
// the extremes of one dword: one and and two packed min / max per word.  Only the even bytes are masked: a 16-bit half orders
// by its high byte first, so the unmasked word leaves the largest (smallest) odd byte in the high byte of max_o (min_o)
// whatever the low bytes hold, and pw_pmax / pw_pmin read that byte alone.
PW_HD void pw_extremes(PwAcc &a, PwWords x)
{
    a.max_e = pw_pk_max(a.max_e, x.wz & PW_EVEN);
    a.max_o = pw_pk_max(a.max_o, x.wz);
    a.min_e = pw_pk_min(a.min_e, x.wo & PW_EVEN);
    a.min_o = pw_pk_min(a.min_o, x.wo);
}
PW_HD void pw_update(PwAcc &a, PwWords x)
{
    pw_moments(a.s2, a.s1, x.wz);
    pw_extremes(a, x);
}

// the largest / smallest counted pixel (0 / 255 when nothing was counted)
PW_HD int pw_pmax(const PwAcc &a)
{
    const uint32_t e = (a.max_e & 0xffffu) > (a.max_e >> 16) ? (a.max_e & 0xffffu) : (a.max_e >> 16);
    const uint32_t o = (a.max_o & 0xffffu) > (a.max_o >> 16) ? (a.max_o & 0xffffu) : (a.max_o >> 16);
    return (int)(e > (o >> 8) ? e : (o >> 8));
}
PW_HD int pw_pmin(const PwAcc &a)
{
    const uint32_t e = (a.min_e & 0xffffu) < (a.min_e >> 16) ? (a.min_e & 0xffffu) : (a.min_e >> 16);
    const uint32_t o = (a.min_o & 0xffffu) < (a.min_o >> 16) ? (a.min_o & 0xffffu) : (a.min_o >> 16);
    return (int)(e < (o >> 8) ? e : (o >> 8));
}

// THE PAIR INPUT of L's row pass.  The strips feed a pair of taps with ((float)pa − fdc) + ((float)pb − fdc), fdc = (float)dc.
// Every term is an exact integer of at most ten bits, so that equals (float)(pa + pb − 2·dc) bit for bit, a zero sum being +0
// either way (tests/prune_fast_main.cpp, all 2²⁴ triples).  A pixel is centred once (pw_centred) and serves every pair and
// output that reads it; a pair input is one add.
PW_HD float pw_centred(uint32_t p, float fdc) { return (float)p - fdc; }
PW_HD float pw_pair_input(float ca, float cb) { return ca + cb; }

// Σ (p − dc)² of n pixels from their moments (RANGE above)
PW_HD uint32_t pw_energy(uint32_t s2, uint32_t s1, int n, int dc) { return (s2 + (uint32_t)n * (uint32_t)(dc * dc)) - 2u * (uint32_t)dc * s1; }
// ⌈16·√e⌉ exactly, for the energy of one 8 × 8 cell (e ≤ 64·255² < 2²⁴: exact as a float, 256·e < 2³²).  The estimate
// 16·sqrt((float)e) is within 0.01 of the true value whichever square root forms it (one rounding of the device's
// instruction or of the host's is below 2e-7 relative, of at most 32640), so its integer part t is at most the answer
// (an integer above t − 0.01) and at least the answer − 2 (which is below t + 2.01); two compare-and-steps reach the
// smallest r with r² ≥ 256·e.
PW_HD uint32_t pw_root16(uint32_t e)
{
    const uint32_t e256 = e << 8;
    uint32_t r = (uint32_t)(16.0f * pw_sqrt_est((float)e));
    r += pw_mul24(r, r) < e256;
    r += pw_mul24(r, r) < e256;
    return r;
}
// Σ (p − dc)
PW_HD int pw_sum(uint32_t s1, int n, int dc) { return (int)s1 - n * dc; }
// max |p − dc| from the extremes (0 when nothing was counted)
PW_HD int pw_V(int pmax, int pmin, int dc)
{
    const int up = pmax - dc, dn = dc - pmin, v = up > dn ? up : dn;
    return v > 0 ? v : 0;
}

} // namespace pdog
