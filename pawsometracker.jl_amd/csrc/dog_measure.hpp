// dog_measure.hpp — what the detection stops one step short of: the response at a tracked position and the position to
// better than a pixel.
//
// `findmax` (/root/reference/src/PawsomeTracker.jl:59) returns (value, index) and the reference keeps the index only.  For
// n positions dog_measure_kernel evaluates the reference's buff[I] (:57) at the position and at its four neighbours —
// exact_pixel's arithmetic (dog_exact.hpp): dense l×l Float64, kernel column-major order, product and sum rounded apart,
// PaddedView fill — so the five values are this repository's restatement of the reference bit for bit, and stand on the
// same two last-bit assumptions as exact mode (include/pawsome_dog.h).  The SUB-PIXEL RULE on top of them is this
// library's addition, not the reference's: per axis a parabola through the three values, its vertex clamped to half a
// pixel (subpixel_rule below: ONE function for the host helper pdog_subpixel and for the kernel).
//
// No Float64 FMA may appear in the kernel (an `a*b + c` contracted into one would round once where the reference rounds
// twice), and its ISA is checked for that with a plain search for the opcode.  gfx950 has no Float64 division instruction:
// `x / y` expands into a reciprocal estimate refined by FMAs, so a single division — or the table p / 255.0 computed in
// the kernel, as the refinement does — would put the opcode back.  Hence two things here: the N0f8 table is folded at
// compile time (kN0f8), and the rule's one division per axis is a long division on the significands in integer arithmetic
// (div_rn: correctly rounded, ties to even, every special case of IEEE 754), the same instructions on the host and on the
// device.  It runs once per position beside five l²-term chains.
#pragma once
#include "dog_exact.hpp"

namespace pdog {

// a / b, IEEE 754 binary64, round to nearest even — in integer arithmetic (see the header).
__host__ __device__ inline double div_rn(double a, double b)
{
    typedef unsigned long long u64;
    constexpr u64 SIGN = 1ull << 63, INF = 0x7ffull << 52, QNAN = 0x7ff8ull << 48, MANT = (1ull << 52) - 1, ONE = 1ull << 52;
    u64 ua, ub, out;
    __builtin_memcpy(&ua, &a, 8);
    __builtin_memcpy(&ub, &b, 8);
    const u64 sign = (ua ^ ub) & SIGN;
    int ea = (int)((ua >> 52) & 0x7ff), eb = (int)((ub >> 52) & 0x7ff);
    u64 ma = ua & MANT, mb = ub & MANT;
    const bool a_zero = !ea && !ma, b_zero = !eb && !mb;
    if (ea == 0x7ff || eb == 0x7ff) {
        if ((ea == 0x7ff && ma) || (eb == 0x7ff && mb) || ea == eb) out = QNAN; // a NaN, or ∞ / ∞
        else out = sign | (ea == 0x7ff ? INF : 0);                              // ∞ / finite, finite / ∞
    } else if (b_zero) {
        out = a_zero ? QNAN : (sign | INF);
    } else if (a_zero) {
        out = sign;
    } else {
        // significands with the leading one at bit 52 (subnormals shifted up), value = m · 2^(e − 1075)
        if (ea) ma |= ONE; else { const int s = __builtin_clzll(ma) - 11; ma <<= s; ea = 1 - s; }
        if (eb) mb |= ONE; else { const int s = __builtin_clzll(mb) - 11; mb <<= s; eb = 1 - s; }
        int E = ea - eb + 1023; // biased exponent of the quotient once ma / mb lies in [1, 2)
        if (ma < mb) { ma <<= 1; --E; }
        // restoring division: q = ⌊(ma / mb)·2^54⌋ in [2^54, 2^55) — 53 result bits, a guard bit, and the sticky bit below
        u64 q = 0, rem = ma;
        for (int k = 0; k < 55; ++k) {
            q <<= 1;
            if (rem >= mb) { rem -= mb; q |= 1; }
            rem <<= 1;
        }
        q |= rem != 0;
        if (E >= 0x7ff) {
            out = sign | INF;
        } else {
            int s = 2;                   // bits to drop: two for a normal result, more for a subnormal one
            if (E < 1) { s += 1 - E; E = 1; }
            if (s > 62) s = 62;          // (q < 2^55: everything is dropped and the result rounds to zero)
            const u64 lost = q & ((1ull << s) - 1), half = 1ull << (s - 1);
            u64 r = q >> s;
            if (lost > half || (lost == half && (r & 1))) ++r;
            // r carries the leading one (bit 52) of a normal result: added, not or-ed, so a carry out of the significand
            // moves the exponent up by itself; a subnormal result (r < 2^52) leaves the exponent field at zero
            out = ((u64)(E - 1) << 52) + r;
            if ((out >> 52) >= 0x7ff) out = INF;
            out |= sign;
        }
    }
    double res;
    __builtin_memcpy(&res, &out, 8);
    return res;
}

// The sub-pixel rule.  r = {c, up, down, left, right}: the response at the 1-based position (i, j) and at (i−1, j),
// (i+1, j), (i, j−1), (i, j+1).  Per axis, m the lower-index neighbour and p the higher one: den = (m − c) + (p − c),
// num = m − p; the offset is 0 unless den < 0 (not a strict maximum along the axis, a flat patch, a NaN), otherwise
// (0.5·num) / den clamped to [−0.5, 0.5] (at a true 3-point maximum |num| ≤ |den|: the clamp acts only where the integer
// position was clamped into the frame, :61, or the window's peak sat on the window border below a larger response outside).
__host__ __device__ inline double subpixel_offset(double c, double m, double p)
{
#pragma clang fp contract(off)
    const double den = (m - c) + (p - c);
    const double num = m - p;
    if (!(den < 0)) return 0.0;
    double off = div_rn(0.5 * num, den);
    if (off > 0.5) off = 0.5;
    if (off < -0.5) off = -0.5;
    return off;
}
__host__ __device__ inline void subpixel_rule(const double r[5], int i, int j, double out[2])
{
#pragma clang fp contract(off)
    out[0] = (double)i + subpixel_offset(r[0], r[1], r[2]);
    out[1] = (double)j + subpixel_offset(r[0], r[3], r[4]);
}

// Float64(::N0f8) = p / 255.0 for every byte, folded by the compiler (IEEE division, round to nearest: the values the
// refinement's run-time table holds)
struct N0f8Table {
    double v[256];
};
constexpr N0f8Table make_n0f8_table()
{
    N0f8Table t{};
    for (int p = 0; p < 256; ++p) t.v[p] = (double)p / 255.0;
    return t;
}
static __device__ const N0f8Table kN0f8 = make_n0f8_table();

struct MeasureGeo {
    const uint8_t *frames;
    long long frame_stride, row_stride;
    const int32_t *frame_index; // null: position b looks at frame b
    const int32_t *ij;          // [n][2], 1-based (row, col); clamped into the frame first (as pdog_diag_point does)
    int n;
    int fh, fw, fill, L;
    int ppw;                    // positions per wave (1 … MEASURE_PPW)
    int tile_pitch, tile_bytes; // a position's (l+2)×(l+2) pixel tile in LDS: row pitch and size in bytes; 0 = no tile (below)
    const double *K64;          // dense Float64 kernel, l×l column-major (:41-43)
    double *out_resp5;          // null or [n][5] {c, up, down, left, right}
    double *out_sub;            // null or [n][2] 1-based (row, col)
};

// One lane per (position, value): up to 12 positions in 60 lanes of a wave, one wave per workgroup (a small n still
// spreads over the CUs).  The l² terms of one value are a strictly sequential chain by definition; the parallelism is across
// values and positions, and the lanes of a wave step through K together, so the kernel's table reads are scalar loads.
//
// The five patches of a position overlap in all but one row or column, and every pixel is read l² times over: the wave
// first copies each position's (l+2)×(l+2) pixels into LDS, the PaddedView fill (:48) materialised, and the chains then
// run on exact_patch over that tile — the inner loop is two LDS reads (pixel, table), a multiplication and an addition,
// and no lane ever takes a per-pixel bounds path.  Read straight from the frame instead (exact_pixel; tile_pitch = 0) a
// wave's 60 byte gathers per term thrash the vector L1 and the same work takes 1.9× as long; that path
// remains for long kernels (l > 93), whose tiles would leave a wave fewer than four positions.  How many positions a wave takes follows from the tile's
// size (measure_layout): four workgroups per CU where the tiles allow it, one per SIMD.
constexpr int MEASURE_NT = 64;
constexpr int MEASURE_PPW = 12;              // positions per wave at most: 60 lanes
constexpr int MEASURE_WG_LDS = 38400;        // tile bytes per workgroup that leave room for four workgroups per CU (+ 2 KB table each)
constexpr int MEASURE_MIN_PPW = 4;           // fewer tiles than this per wave: the frame is read in place (measured at 8 and at 1; pawsome_dog.hip)

// rows `pitch` bytes apart and tiles `bytes` apart, both an odd number of dwords: the lanes of a wave read the same
// (row, column) of different tiles, and a position's up / down lanes rows one pitch apart
__host__ __device__ constexpr int measure_tile_pitch(int L) { return ((L + 2 + 3) / 4 * 4) % 8 == 0 ? (L + 2 + 3) / 4 * 4 + 4 : (L + 2 + 3) / 4 * 4; }
__host__ __device__ constexpr int measure_tile_bytes(int L) { return ((L + 2) * measure_tile_pitch(L)) % 8 == 0 ? (L + 2) * measure_tile_pitch(L) + 4 : (L + 2) * measure_tile_pitch(L); }

constexpr int MEASURE_UNR = 16;              // a lane's loads in flight while a tile is staged

// exact_patch (dog_exact.hpp) over a tile in LDS — the same l² terms in the same order (kernel column-major: K is
// contiguous along it), product and sum rounded apart — with the pixel reads of the NEXT eight terms issued before the
// additions of these eight: exact_patch waits for each block's pixels, then for its table entries, then adds, and a wave
// alone on its SIMD (the tiles leave room for four per CU) has nothing else to run meanwhile.
__device__ __forceinline__ double tile_value(const unsigned char *patch, int pitch, int L, k64_ptr K, const double *lut)
{
    const int LL = L * L; // ≥ 25
    int ki = 0, kj = 0;
    auto next_offset = [&]() { // tile offset of the next term's pixel: rows within a kernel column, then the next column
        const int o = ki * pitch + kj;
        if (++ki == L) { ki = 0; ++kj; }
        return o;
    };
    double tmp = 0.0;
    unsigned char p[8];
    double kc[8]; // these eight terms' kernel entries (scalar registers), loaded a block ahead like the pixels
#pragma unroll
    for (int u = 0; u < 8; ++u) { p[u] = patch[next_offset()]; kc[u] = K[u]; }
    int t = 0;
    for (; t + 16 <= LL; t += 8) { // every block of eight but the last
        double a[8], kn[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = lut[p[u]];
#pragma unroll
        for (int u = 0; u < 8; ++u) { p[u] = patch[next_offset()]; kn[u] = K[t + 8 + u]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) tmp = exact_mac(tmp, a[u], kc[u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) kc[u] = kn[u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) tmp = exact_mac(tmp, lut[p[u]], kc[u]); // the last whole block: nothing left to fetch ahead
    t += 8;
    for (; t < LL; ++t) tmp = exact_mac(tmp, lut[patch[next_offset()]], K[t]);
    return tmp;
}

static __global__ __launch_bounds__(MEASURE_NT) void dog_measure_kernel(const MeasureGeo g)
{
    __shared__ double lut[256];
    extern __shared__ __attribute__((aligned(16))) unsigned char tiles[];
    const int lane = threadIdx.x, hw = g.L >> 1;
    for (int p = lane; p < 256; p += MEASURE_NT) lut[p] = kN0f8.v[p];
    if (g.tile_pitch) {
        const int T = g.L + 2, da = MEASURE_NT / T, dc = MEASURE_NT - da * T;
        for (int s = 0; s < g.ppw; ++s) {
            const long long pos = (long long)blockIdx.x * g.ppw + s;
            if (pos >= g.n) break;
            const int i = min(max(g.ij[2 * pos], 1), g.fh), j = min(max(g.ij[2 * pos + 1], 1), g.fw);
            const long long fidx = g.frame_index ? (long long)g.frame_index[pos] : pos;
            const uint8_t *__restrict__ frame = g.frames + fidx * g.frame_stride;
            unsigned char *tile = tiles + s * g.tile_bytes;
            const int oi = i - 2 - hw, oj = j - 2 - hw; // 0-based frame coordinates of the tile's first pixel: one pixel beyond the centre's patch
            int a = lane / T, c = lane - a * T;         // (row, column) of this lane's next pixel, stepped without a division
            // batches of MEASURE_UNR pixels per lane: every load first — unconditional, at an address clamped into the
            // frame — then the PaddedView fill (:48) selected and the stores (a load per iteration waited for its own
            // store: a round trip to memory per pixel)
            for (int e0 = lane; e0 < T * T; e0 += MEASURE_UNR * MEASURE_NT) {
                unsigned char px[MEASURE_UNR];
                int ra[MEASURE_UNR], rc[MEASURE_UNR];
#pragma unroll
                for (int u = 0; u < MEASURE_UNR; ++u) {
                    ra[u] = a;
                    rc[u] = c;
                    const int gi = min(max(oi + a, 0), g.fh - 1), gj = min(max(oj + c, 0), g.fw - 1); // (a surplus item of the last batch too)
                    px[u] = frame[(long long)gi * g.row_stride + gj];
                    a += da;
                    c += dc;
                    if (c >= T) { c -= T; ++a; }
                }
#pragma unroll
                for (int u = 0; u < MEASURE_UNR; ++u) {
                    if (e0 + u * MEASURE_NT >= T * T) continue;
                    const int gi = oi + ra[u], gj = oj + rc[u];
                    const bool in = gi >= 0 && gi < g.fh && gj >= 0 && gj < g.fw;
                    tile[ra[u] * g.tile_pitch + rc[u]] = in ? px[u] : (unsigned char)g.fill;
                }
            }
        }
    }
    __syncthreads();
    const int slot = lane / 5, v = lane - 5 * slot;
    const long long pos = (long long)blockIdx.x * g.ppw + slot;
    const bool act = slot < g.ppw && pos < g.n;
    double val = 0.0;
    int i = 1, j = 1;
    if (act) {
        i = min(max(g.ij[2 * pos], 1), g.fh);
        j = min(max(g.ij[2 * pos + 1], 1), g.fw);
        const int di = v == 1 ? -1 : v == 2 ? 1 : 0, dj = v == 3 ? -1 : v == 4 ? 1 : 0;
        const k64_ptr K = (k64_ptr)(unsigned long long)g.K64;
        if (g.tile_pitch) {
            const unsigned char *patch = tiles + slot * g.tile_bytes + (1 + di) * g.tile_pitch + (1 + dj);
            val = tile_value(patch, g.tile_pitch, g.L, K, lut);
        } else {
            const long long fidx = g.frame_index ? (long long)g.frame_index[pos] : pos;
            const uint8_t *__restrict__ frame = g.frames + fidx * g.frame_stride;
            val = exact_pixel(frame, g.row_stride, g.fh, g.fw, g.fill, i - 1 + di - hw, j - 1 + dj - hw, g.L, K, lut);
        }
        if (g.out_resp5) g.out_resp5[5 * pos + v] = val;
    }
    // the position's five values to its first lane (lanes past the wave's end hand back their own value: never used)
    double r[5];
    r[0] = val;
#pragma unroll
    for (int k = 1; k < 5; ++k) r[k] = __shfl_down(val, k, 64);
    if (act && v == 0 && g.out_sub) {
        double s[2];
        subpixel_rule(r, i, j, s);
        g.out_sub[2 * pos] = s[0];
        g.out_sub[2 * pos + 1] = s[1];
    }
}

} // namespace pdog
