// dog_shape.hpp — the kernel of the shape rule (include/pawsome_shape.h states it; pdog_shape.hpp holds its Float64 part).
// pawsome_shape.hip includes this file, and dog_blob.hpp for the steps it shares (shape_stage_tile ... shape_contrast).
//
// shape_kernel: ONE workgroup of 256 threads per position, for every radius (no tiers: the loops below scale with R).
//   1. The patch's bounding rows, D = 2R + 1 rows of D bytes, go into LDS as rows of W = ceil(D / 4) dwords, the PaddedView
//      fill (:48) materialised: every patch byte is read from memory once.  A lane owns one dword of one row and loads it as
//      the background kernels load theirs (dog_background.hpp, bg_load4): at the column clamped into 0 ... w - 4 and the row
//      clamped into the frame, so every byte read lies inside a row's w bytes for any base address and any row stride; the
//      bytes that belong to the patch are then picked out of the word, and the fill where the pixel lies outside the frame.
//      Frames narrower than 4 are read byte by byte.
//   2. A 256-bin histogram of the disc pixels in LDS (LDS atomics; nothing atomic touches global memory).
//   3. Every wave finds the bin of rank (N - 1) / 2 for itself: a lane sums four bins, the wave scans the 64 sums with
//      shuffles, and the median is the number of bins whose inclusive prefix does not exceed the rank.
//   4. c from the staged 3 x 3 (R >= 2: it lies inside the tile).
//   5. The six sums per lane in int32, reduced within the wave by shuffles and across the four waves through LDS.
//   6. Eight ordinary vector stores; and the six Float64 of shape::derive by one lane, if asked.
// The loops over the bounding box run over D rows of 2^colbits columns (colbits = ceil(log2 D)): row and column of an item
// are a shift and a mask, and the items past column D are skipped.  No cooperative launch, no waiting on other workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include "pdog_shape.hpp"

namespace pdog {

constexpr int kShapeThreads = 256;
constexpr int kShapeWaves = kShapeThreads / 64;

struct ShapeGeo {
    const uint8_t *frames;
    long long frame_stride, row_stride;
    const int32_t *frame_index; // null: position b looks at frame b
    const int32_t *ij;          // [n][2], 1-based (row, col); clamped into the frame first
    int n;
    int fh, fw, fill, darker;
    int R, min_contrast;
    int colbits;                // ceil(log2(2R + 1)): 3 ... 8
    int rank;                   // (N - 1) / 2, N the number of disc pixels
    int32_t *out_sums;          // null or [n][8]
    double *out_shape;          // null or [n][6]
};

// LDS bytes of the tile: D rows of W dwords
__host__ __device__ constexpr int shape_tile_words(int R) { return (2 * R + 1) * ((2 * R + 1 + 3) / 4); }

__device__ __forceinline__ int shape_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Steps 1 - 4, shared with the blob kernel (dog_blob.hpp), which measures the same patch against the same b and c.  The
// geometry goes in BY VALUE and the loop bounds are handed over: with it by reference, or with D and W recomputed inside,
// shape_kernel's SGPR figure moved from the 64 it had before the steps were functions (profiles/blob_kernel_regs.txt).
// 1. the tile: D rows of W dwords from (i0, j0), the 0-based frame coordinates of its first pixel
__device__ __forceinline__ void shape_stage_tile(const ShapeGeo g, const uint8_t *__restrict__ frame, int i0, int j0, uint32_t fill,
                                                 uint32_t *tile, int tid, int D, int W)
{
    const int wb = g.colbits - 2, items = D << wb; // W <= 2^wb
#pragma unroll 4
    for (int e = tid; e < items; e += kShapeThreads) {
        const int r = e >> wb, k = e & ((1 << wb) - 1);
        if (k >= W) continue;
        const int gi = i0 + r, c0 = j0 + 4 * k;
        const bool row_in = gi >= 0 && gi < g.fh;
        const uint8_t *rowp = frame + (long long)min(max(gi, 0), g.fh - 1) * g.row_stride;
        uint32_t word = 0;
        if (g.fw >= 4) {
            const int cj = min(max(c0, 0), g.fw - 4);
            uint32_t v;
            __builtin_memcpy(&v, rowp + cj, 4);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = c0 + b;
                const bool in = row_in && col >= 0 && col < g.fw; // then 0 <= col - cj <= 3
                const uint32_t px = in ? (v >> (8 * ((col - cj) & 3))) & 0xffu : fill;
                word |= px << (8 * b);
            }
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = c0 + b;
                const bool in = row_in && col >= 0 && col < g.fw;
                const uint32_t px = in ? (uint32_t)rowp[min(max(col, 0), g.fw - 1)] : fill;
                word |= px << (8 * b);
            }
        }
        tile[r * W + k] = word;
    }
}

// 2. the histogram of the disc (hist zeroed, and a barrier passed, before)
__device__ __forceinline__ void shape_histogram(const ShapeGeo g, const uint8_t *px, uint32_t *hist, int tid, int R, int D, int P,
                                                int cmask, int items, int R2)
{
    for (int e = tid; e < items; e += kShapeThreads) {
        const int r = e >> g.colbits, c = e & cmask;
        const int dy = r - R, dx = c - R;
        if (c < D && dy * dy + dx * dx <= R2) atomicAdd(&hist[px[r * P + c]], 1u);
    }
}

// 3. the lower median, by every wave for itself: the number of bins whose inclusive prefix is <= rank
__device__ __forceinline__ int shape_median(const uint32_t *hist, int lane, int rank)
{
    const uint4 h4 = *(const uint4 *)&hist[4 * lane];
    const int own = (int)(h4.x + h4.y + h4.z + h4.w);
    int incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    const int p0 = incl - own + (int)h4.x, p1 = p0 + (int)h4.y, p2 = p1 + (int)h4.z;
    return shape_wave_sum((p0 <= rank) + (p1 <= rank) + (p2 <= rank) + (incl <= rank));
}

// 4. the target's contrast, from the staged 3 x 3
__device__ __forceinline__ int shape_contrast(const uint8_t *px, int R, int P, int b, int darker)
{
    int c = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int p = px[(R + dy) * P + R + dx];
            c = max(c, darker ? b - p : p - b);
        }
    return c;
}

#ifndef PDOG_SHAPE_STEPS_ONLY // (dog_blob.hpp takes the steps above and leaves the kernel to pawsome_shape.hip's unit)
static __global__ __launch_bounds__(kShapeThreads) void shape_kernel(const ShapeGeo g)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[256];
    __shared__ int red[kShapeWaves][6];
    extern __shared__ __attribute__((aligned(16))) uint32_t tile[]; // D rows of W dwords
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long pos = blockIdx.x;
    const int R = g.R, D = 2 * R + 1, W = (D + 3) >> 2, P = 4 * W;
    const int i = min(max(g.ij[2 * pos], 1), g.fh), j = min(max(g.ij[2 * pos + 1], 1), g.fw);
    const long long fidx = g.frame_index ? (long long)g.frame_index[pos] : pos;
    const uint8_t *__restrict__ frame = g.frames + fidx * g.frame_stride;

    const int i0 = i - 1 - R, j0 = j - 1 - R; // 0-based frame coordinates of the tile's first pixel
    const uint32_t fill = (uint32_t)g.fill & 0xffu;

    hist[tid] = 0;
    shape_stage_tile(g, frame, i0, j0, fill, tile, tid, D, W);
    __syncthreads();
    const uint8_t *px = (const uint8_t *)tile;
    const int cmask = (1 << g.colbits) - 1, items = D << g.colbits, R2 = R * R;
    shape_histogram(g, px, hist, tid, R, D, P, cmask, items, R2);
    __syncthreads();
    const int b = shape_median(hist, lane, g.rank);
    const int c = shape_contrast(px, R, P, b, g.darker);
    // 5. the sums over the mask
    int n = 0, sy = 0, sx = 0, syy = 0, syx = 0, sxx = 0;
    if (c >= g.min_contrast) {
        for (int e = tid; e < items; e += kShapeThreads) {
            const int r = e >> g.colbits, cc = e & cmask;
            const int dy = r - R, dx = cc - R;
            if (cc < D && dy * dy + dx * dx <= R2) {
                const int p = px[r * P + cc];
                const int s = g.darker ? b - p : p - b;
                if (2 * s >= c) {
                    n += 1;
                    sy += dy;
                    sx += dx;
                    syy += dy * dy;
                    syx += dy * dx;
                    sxx += dx * dx;
                }
            }
        }
    }
    n = shape_wave_sum(n);
    sy = shape_wave_sum(sy);
    sx = shape_wave_sum(sx);
    syy = shape_wave_sum(syy);
    syx = shape_wave_sum(syx);
    sxx = shape_wave_sum(sxx);
    if (lane == 0) {
        red[wave][0] = n;
        red[wave][1] = sy;
        red[wave][2] = sx;
        red[wave][3] = syy;
        red[wave][4] = syx;
        red[wave][5] = sxx;
    }
    __syncthreads();
    // 6. the results
    if (tid == 0) {
        int32_t s[8];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            int v = 0;
#pragma unroll
            for (int w = 0; w < kShapeWaves; ++w) v += red[w][k];
            s[k] = v;
        }
        s[6] = b;
        s[7] = c;
        if (g.out_sums) {
#pragma unroll
            for (int k = 0; k < 8; ++k) g.out_sums[8 * pos + k] = s[k];
        }
        if (g.out_shape) {
            double o[6];
            shape::derive(s, i, j, o);
#pragma unroll
            for (int k = 0; k < 6; ++k) g.out_shape[6 * pos + k] = o[k];
        }
    }
}

#endif

} // namespace pdog
