// dog_diag.hpp — the reference's diagnostic overlay (src/diagnose.jl:26-38) on device-resident frames: every frame
// resized into the 360×640 buffer (imresize!, bilinear, centre-aligned), then the dot at the scaled position and the
// path of the last ≤ 100 scaled positions drawn in the target colour.  The label (renderstring!) is not drawn.
//
// The arithmetic is the restatement's (tests/diag_restatement.py, assumptions (a)–(e) in include/pawsome_dog.h):
// Float64, each product and sum rounded on its own (no contraction: the pragma below), rint = round half to even.
//
//   dog_diag_resize_kernel   workgroups over (frame, 256 chunks of 16 output bytes); one 16-B store per thread.
//                            A pixel whose two weights are 0 (exact subsampling: 1080×1920) is the source byte
//                            itself (1 · raw/255 · 255 rounds back to raw), so that path reads only the rows it keeps.
//   dog_diag_overlay_kernel  one workgroup per frame after the resize (stream order): lane t < 99 walks segment t of
//                            the frame's trace with Bresenham, lane 99 draws the 3×3 dot; byte stores of one colour,
//                            so overlapping pixels need no order.  Workgroup 0 of the call's last launch also writes the
//                            trace state the next call starts from (double-buffered: the state it reads stays intact).
//
// Over a frame table and several targets (include/pawsome_overlay.h):
//   dog_diag_resize_kernel<·, TABLE>  output k is frame table[k] of the stack: one uniform load per workgroup.  The table
//                            travels in DiagResizeTableGeo, which derives from the plain argument struct, so the two plain
//                            instances are passed the bytes they were passed before.
//   dog_diag_overlay_targets_kernel   workgroups over (step, target): workgroup (k, t) draws target t's segments and dot
//                            onto output k, from target t's positions (ij_stride positions apart) and target t's 99
//                            inherited points; workgroup (0, t) of the call's last launch writes target t's next state.
//
// Every scaled point lies in [0, 360] × [0, 640] (positions are clamped into the frame first), every write is
// checked against the buffer, and a segment has at most 641 steps.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#pragma clang fp contract(off)

namespace pdog {

constexpr int kDiagH = 360, kDiagW = 640;            // DIAGNOSTIC_VIDEO_SIZE, src/diagnose.jl:2
constexpr int kDiagTrace = 100;                      // TRACE_BUFFER_SIZE, src/diagnose.jl:3
constexpr int kDiagHist = kDiagTrace - 1;            // points a call inherits from the previous ones
constexpr int kDiagChunk = 16;                       // output bytes per resize thread
constexpr int kDiagChunksPerRow = kDiagW / kDiagChunk;
constexpr int kDiagChunksPerFrame = kDiagH * kDiagChunksPerRow;
constexpr int kDiagResizeThreads = 256;
constexpr int kDiagBlocksPerFrame = (kDiagChunksPerFrame + kDiagResizeThreads - 1) / kDiagResizeThreads;
constexpr int kDiagOverlayThreads = 128;              // 99 segments + the dot
constexpr int64_t kDiagFrameBytes = (int64_t)kDiagH * kDiagW;

struct DiagResizeGeo {
    const uint8_t *frames;      // first frame of this launch
    int64_t frame_stride, row_stride;
    int h, w, clamp;            // clamp: either axis upsamples
    double sy, offy, sx, offx;  // s = n_in / n_out, off = 0.5 - s * 0.5 (host)
    uint8_t *out;               // first output frame of this launch
};

struct DiagResizeTableGeo : DiagResizeGeo { // frames: frame 0 of the stack
    const int32_t *table;       // frame index of this launch's first output
};

struct DiagOverlayGeo {
    const int32_t *ij;          // the call's 1-based positions, n x 2
    const int2 *hist_in;        // the last hcnt scaled points before the call, oldest first
    int2 *hist_out;             // written by workgroup 0 when write_hist
    uint8_t *out;               // the call's first output frame
    int n, k0, hcnt, write_hist;
    int h, w;
    double ry, rx;              // 360 / h, 640 / w (host)
    int color;
};

struct DiagOverlayTargetsGeo : DiagOverlayGeo { // ij, hist_in, hist_out: target 0's; target t's hist lies t * kDiagHist further
    int64_t ij_stride;          // positions between two targets' rows of ij
};

// one output index I (1-based) -> first tap, second tap (= first where its weight is 0), weight of the second
__device__ __forceinline__ void diag_tap(int I, double s, double off, int n, int clamp, int &i0, int &i1, double &f)
{
    double y = (double)I * s + off;
    if (clamp) y = fmin(fmax(y, 1.0), (double)n);
    const double iy = floor(y);
    f = y - iy;
    i0 = min(max((int)iy, 1), n); // (no-op: y lies in [1, n] for every size)
    i1 = f == 0.0 ? i0 : min(i0 + 1, n);
}

template <bool kAligned, bool TABLE = false>
__global__ __launch_bounds__(kDiagResizeThreads) void dog_diag_resize_kernel(const std::conditional_t<TABLE, DiagResizeTableGeo, DiagResizeGeo> g,
                                                                             const double *lut)
{
    __shared__ double p[256]; // raw / 255.0, computed on the host (assumption (a))
    p[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int k = blockIdx.x / kDiagBlocksPerFrame;
    const int c = (blockIdx.x - k * kDiagBlocksPerFrame) * kDiagResizeThreads + threadIdx.x;
    if (c >= kDiagChunksPerFrame) return;
    const int I = c / kDiagChunksPerRow + 1, J0 = (c - (I - 1) * kDiagChunksPerRow) * kDiagChunk + 1;
    int i0, i1;
    double fy;
    diag_tap(I, g.sy, g.offy, g.h, g.clamp, i0, i1, fy);
    int fidx = k;
    if constexpr (TABLE) fidx = g.table[k]; // (checked on the host: 0 ... n_frames - 1)
    const uint8_t *src = g.frames + (int64_t)fidx * g.frame_stride;
    const uint8_t *r0 = src + (int64_t)(i0 - 1) * g.row_stride, *r1 = src + (int64_t)(i1 - 1) * g.row_stride;
    const double gy = 1.0 - fy;
    uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int jj = 0; jj < kDiagChunk; ++jj) {
        int j0, j1;
        double fx;
        diag_tap(J0 + jj, g.sx, g.offx, g.w, g.clamp, j0, j1, fx);
        uint32_t b;
        if (fy == 0.0 && fx == 0.0) {
            b = r0[j0 - 1];
        } else {
            const double gx = 1.0 - fx;
            const double v = gx * (gy * p[r0[j0 - 1]] + fy * p[r1[j0 - 1]]) + fx * (gy * p[r0[j1 - 1]] + fy * p[r1[j1 - 1]]);
            b = (uint32_t)fmin(fmax(rint(v * 255.0), 0.0), 255.0);
        }
        wd[jj >> 2] |= b << (8 * (jj & 3));
    }
    uint8_t *o = g.out + (int64_t)k * kDiagFrameBytes + (int64_t)(I - 1) * kDiagW + (J0 - 1);
    if (kAligned) {
        *(uint4 *)o = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    } else {
#pragma unroll
        for (int jj = 0; jj < kDiagChunk; ++jj) o[jj] = (uint8_t)(wd[jj >> 2] >> (8 * (jj & 3)));
    }
}

// scaled point of the call's position idx (idx < 0: one of the inherited points); false where the trace has none
__device__ __forceinline__ bool diag_point(const DiagOverlayGeo &g, int idx, int2 &q)
{
    if (idx >= 0) {
        const int i = min(max(g.ij[2 * idx], 1), g.h), j = min(max(g.ij[2 * idx + 1], 1), g.w);
        q = make_int2((int)rint((double)i * g.ry), (int)rint((double)j * g.rx));
        return true;
    }
    const int hpos = g.hcnt + idx;
    if (hpos < 0) return false;
    q = g.hist_in[hpos];
    return true;
}

__device__ __forceinline__ void diag_plot(uint8_t *o, int a, int b, uint8_t color)
{
    if (a >= 1 && a <= kDiagH && b >= 1 && b <= kDiagW) o[(a - 1) * kDiagW + (b - 1)] = color; // drawifinbounds!
}

// what workgroup `blk` of a launch draws onto output k = g.k0 + blk of one target's trace
__device__ __forceinline__ void diag_draw(const DiagOverlayGeo &g, int blk)
{
    const int k = g.k0 + blk, t = threadIdx.x;
    uint8_t *o = g.out + (int64_t)k * kDiagFrameBytes;
    const uint8_t color = (uint8_t)g.color;
    int2 p0, p1;
    if (t < kDiagHist) {
        // segment t of the trace: slot t -> slot t + 1, slot kDiagHist being frame k itself (older -> newer)
        if (diag_point(g, k - kDiagHist + t, p0) && diag_point(g, k - kDiagHist + t + 1, p1)) {
            int y0 = p0.x, x0 = p0.y;
            const int y1 = p1.x, x1 = p1.y;
            const int dx = abs(x1 - x0), dy = abs(y1 - y0);
            const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
            int err2 = dx > dy ? dx : -dy; // 2 * err: the reference's err is a Float64 half-integer
            for (int step = 0; step <= kDiagW + kDiagH; ++step) { // (at most 641 steps reach the end)
                diag_plot(o, y0, x0, color);
                if (x0 == x1 && y0 == y1) break;
                const int e2 = err2;
                if (e2 > -2 * dx) { err2 -= 2 * dy; x0 += sx; }
                if (e2 < 2 * dy) { err2 += 2 * dx; y0 += sy; }
            }
        }
    } else if (t == kDiagHist) {
        diag_point(g, k, p0);
        for (int a = -1; a <= 1; ++a) // ((a/2)^2 + (b/2)^2 < 1: the 3 x 3 block
            for (int b = -1; b <= 1; ++b) diag_plot(o, p0.x + a, p0.y + b, color);
    }
    if (g.write_hist && blk == 0) {
        const int cnt = min(kDiagHist, g.hcnt + g.n);
        if (t < cnt && diag_point(g, g.n - cnt + t, p1)) g.hist_out[t] = p1;
    }
}

__global__ __launch_bounds__(kDiagOverlayThreads) void dog_diag_overlay_kernel(const DiagOverlayGeo g)
{
    diag_draw(g, (int)blockIdx.x);
}

__global__ __launch_bounds__(kDiagOverlayThreads) void dog_diag_overlay_targets_kernel(const DiagOverlayTargetsGeo tg)
{
    const int t = blockIdx.y;
    DiagOverlayGeo g = tg; // target t's view: the outputs are shared
    g.ij += 2 * ((int64_t)t * tg.ij_stride);
    g.hist_in += t * kDiagHist;
    g.hist_out += t * kDiagHist;
    diag_draw(g, (int)blockIdx.x);
}

} // namespace pdog
