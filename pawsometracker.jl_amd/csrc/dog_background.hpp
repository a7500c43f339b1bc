// dog_background.hpp — the two kernels of the background model (include/pawsome_background.h states the rule,
// dog_bg_words.hpp holds the arithmetic on a dword of four pixels).  pawsome_background.hip alone includes this file.
//
// (a) bg_median_kernel<KMAX, WIDE>: a lane owns ONE dword of four adjacent pixels and loads it from each of the K sample frames
//     into registers — K independent loads in flight, a wave's 256 B of every frame coalesced — then decides the median's eight
//     bits in those registers (bw_median).  Every sample byte is read once from memory.  K is a run-time value within the tier
//     KMAX (8, 16, 32 or 64 words); the loops over the tier are unrolled, so the array never leaves the registers: no scratch.
// (b) bg_subtract_kernel: a lane owns 16 adjacent pixels of one output row: one 16-byte load of the frame, one of the model
//     (the same 2 MB for every step: cache hits), four bw_sub4, one 16-byte store.  The frame of a step is one scalar load.
//
// LAYOUTS.  Rows are addressed by column, never by address: any base, any row stride >= w.  A dword or a 16-byte piece that
// lies inside the row is loaded and stored unaligned, whole.  The LAST dword of a row that is no multiple of 4 wide is loaded
// at the column clamped to w − 4 and shifted down (bg_load4: every byte read lies in the row's w bytes; rows narrower than 4
// are read byte by byte) and stored byte by byte, so nothing behind a row's w bytes is read into a result or written.
#pragma once
#include <hip/hip_runtime.h>
#include "dog_bg_words.hpp"

namespace pdog {

constexpr int kBgThreads = 256;

// columns col ... col + 3 of a row of w bytes as a dword; the bytes at and behind column w are unspecified
__device__ __forceinline__ uint32_t bg_load4(const uint8_t *row, int col, int w)
{
    uint32_t v = 0;
    if (w >= 4) {
        const int cj = min(col, w - 4);
        __builtin_memcpy(&v, row + cj, 4);
        return v >> (8 * (col - cj));
    }
    for (int i = 0; i < w; ++i) v |= (uint32_t)row[i] << (8 * i); // (col is 0)
    return v;
}
// the bytes of v that lie in the row
__device__ __forceinline__ void bg_store4(uint8_t *row, int col, int w, uint32_t v)
{
    if (col + 4 <= w) {
        __builtin_memcpy(row + col, &v, 4);
        return;
    }
    for (int i = 0; col + i < w; ++i) row[col + i] = (uint8_t)(v >> (8 * i));
}

struct BgMedianGeo {
    const uint8_t *frames;
    const int32_t *samples; // device: KMAX frame indices, checked on the host — the k of the call, then its last one repeated
    uint8_t *model;         // h rows of w bytes, dense
    int64_t frame_stride, row_stride;
    int h, w, wpr, k;       // wpr = ceil(w / 4) dwords per row
};

// WIDE: w >= 4, every load one dword at the lane's clamped column.  The KMAX loads carry no condition — the words behind the
// k-th re-read the k-th frame's (a cache hit) and are replaced by 0xffffffff — so all of them are in flight at once; a load
// under `if (k < g.k)` ends its block in s_waitcnt vmcnt(0), and the 64 loads then cost 64 latencies in a row.
template <int KMAX, bool WIDE>
__global__ __launch_bounds__(kBgThreads) void bg_median_kernel(const BgMedianGeo g)
{
    const unsigned idx = blockIdx.x * (unsigned)kBgThreads + threadIdx.x;
    if (idx >= (unsigned)g.h * (unsigned)g.wpr) return;
    const int row = (int)(idx / (unsigned)g.wpr), col = 4 * (int)(idx % (unsigned)g.wpr);
    const int cj = WIDE ? min(col, g.w - 4) : 0;
    const uint8_t *p = g.frames + (int64_t)row * g.row_stride + cj;
    uint32_t x[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        const uint8_t *q = p + (int64_t)g.samples[k] * g.frame_stride;
        uint32_t v;
        if (WIDE) __builtin_memcpy(&v, q, 4);
        else v = bg_load4(q, 0, g.w);
        x[k] = v;
        if (KMAX == 64 && k % 16 == 15) __builtin_amdgcn_sched_barrier(0); // (64 frame offsets at once do not fit the SGPRs)
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) x[k] = k < g.k ? x[k] : 0xffffffffu;
    const uint32_t t = bw_median<KMAX>(x, g.k) >> (8 * (col - cj)); // (the shift commutes with the lanes' arithmetic)
    bg_store4(g.model + (int64_t)row * g.w, col, g.w, t);
}

struct BgSubtractGeo {
    const uint8_t *frames;
    const int32_t *table;   // device: this launch's steps, checked on the host
    const uint8_t *model;
    uint8_t *out;           // this launch's first output
    int64_t frame_stride, row_stride, out_frame_stride, out_row_stride;
    int h, w, ppr;          // ppr = ceil(w / 16) pieces per row
};

// grid (ceil(h * ppr / kBgThreads), steps)
__global__ __launch_bounds__(kBgThreads) void bg_subtract_kernel(const BgSubtractGeo g)
{
    const unsigned idx = blockIdx.x * (unsigned)kBgThreads + threadIdx.x;
    if (idx >= (unsigned)g.h * (unsigned)g.ppr) return;
    const int row = (int)(idx / (unsigned)g.ppr), col = 16 * (int)(idx % (unsigned)g.ppr);
    const int step = blockIdx.y;
    const uint8_t *f = g.frames + (int64_t)g.table[step] * g.frame_stride + (int64_t)row * g.row_stride;
    const uint8_t *b = g.model + (int64_t)row * g.w;
    uint8_t *o = g.out + (int64_t)step * g.out_frame_stride + (int64_t)row * g.out_row_stride;
    if (col + 16 <= g.w) {
        uint4 fv, bv, ov;
        __builtin_memcpy(&fv, f + col, 16);
        __builtin_memcpy(&bv, b + col, 16);
        ov.x = bw_sub4(fv.x, bv.x);
        ov.y = bw_sub4(fv.y, bv.y);
        ov.z = bw_sub4(fv.z, bv.z);
        ov.w = bw_sub4(fv.w, bv.w);
        __builtin_memcpy(o + col, &ov, 16);
        return;
    }
    for (int c = col; c < g.w; c += 4) bg_store4(o, c, g.w, bw_sub4(bg_load4(f, c, g.w), bg_load4(b, c, g.w)));
}

} // namespace pdog
