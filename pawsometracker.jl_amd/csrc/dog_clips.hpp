// dog_clips.hpp — the kernels of pawsome_clips.hip (pdog_clips_*): mode(_img) (src/PawsomeTracker.jl:47) of many
// device-resident frames at once, and the kernel that starts a frame-by-frame walk over many clips (the step between two
// frames is dog_step.hpp's).  Included by pawsome_clips.hip only; nothing here touches the tracker's own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pdog {

constexpr int kClipsModeThreads = 256; // one table entry per thread: the tables have 256 bins

struct ClipsModeGeo {
    const uint8_t *frames;
    long long frame_stride, row_stride;
    const int32_t *frame_index; // NULL: entry b looks at frame b
    int n_frames;
    int h, w;
    int cpr;      // pieces per row: the unaligned head and ceil(w / 16) 16-byte pieces after it
    int parts;    // workgroups per frame (multi-workgroup form), 1 otherwise
};

// The tie rule is dog_mode_kernel's (dog_kernels.hpp): StatsBase.mode keeps the value whose count FIRST exceeds the running
// maximum of a column-major scan; every value that ends with the maximum count reaches it at its LAST occurrence, so the
// winner has the largest count and, among equals, the earliest last occurrence (column-major index j·h + i, stored + 1 so
// that 0 means "never seen").  As one key: count in the high word, the complement of the last occurrence in the low word.
__device__ inline unsigned long long clips_mode_key(unsigned count, unsigned last1)
{
    return ((unsigned long long)count << 32) | (unsigned)~last1;
}

// Rows [0, h) of one frame, pieces `first`, first + step, ….  Piece q of row i: q = 0 is the scalar head up to the first
// 16-byte boundary of the row's address, q >= 1 the 16 bytes after it — one vector load — or the scalar tail.  A lane run-lengths its own bytes before it
// touches LDS: a run costs one add of its length and one max of its last column-major index, not two atomics per pixel.
__device__ inline void clips_mode_accumulate(const uint8_t *__restrict__ img, long long row_stride, int h, int w, int cpr,
                                             long long first, long long step, unsigned *shist, unsigned *slast)
{
    const long long items = (long long)h * cpr;
    for (long long base = first; base < items; base += step) {
        const long long it = base + threadIdx.x;
        unsigned long long lo = 0, hi = 0;
        int len = 0, i = 0;
        long long c0 = 0;
        if (it < items) {
            i = (int)(it / cpr);
            const int q = (int)(it - (long long)i * cpr);
            const uint8_t *row = img + (long long)i * row_stride;
            const int head = min((int)((16u - (unsigned)((uintptr_t)row & 15u)) & 15u), w);
            if (q == 0) {
                len = head;
            } else {
                c0 = head + 16ll * (q - 1);
                len = (int)max(0ll, min(16ll, (long long)w - c0));
            }
            if (len == 16) {
                const uint4 v = *reinterpret_cast<const uint4 *>(row + c0);
                lo = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
                hi = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
            } else {
                for (int k = 0; k < len; ++k) {
                    const unsigned long long b = row[c0 + k];
                    if (k < 8) lo |= b << (8 * k);
                    else hi |= b << (8 * (k - 8));
                }
            }
        }
        unsigned cur = (unsigned)(lo & 255u);
        // the column-major index (+ 1) of this piece's byte k is idx0 + k·h
        const unsigned idx0 = (unsigned)(c0 * h + i) + 1u;
        if (len > 0) {
            unsigned run = 1;
#pragma unroll
            for (int k = 1; k < 16; ++k) {
                if (k < len) {
                    const unsigned b = (unsigned)(((k < 8 ? lo : hi) >> (8 * (k & 7))) & 255u);
                    if (b != cur) {
                        atomicAdd(&shist[cur], run);
                        atomicMax(&slast[cur], idx0 + (unsigned)(k - 1) * (unsigned)h);
                        cur = b;
                        run = 0;
                    }
                    ++run;
                }
            }
            atomicAdd(&shist[cur], run);
            atomicMax(&slast[cur], idx0 + (unsigned)(len - 1) * (unsigned)h);
        }
    }
}

// The winner of 256 (count, last occurrence) pairs, one per thread, through LDS.  Distinct values never share a last
// occurrence, so the maximal key belongs to one thread (a frame has at least one pixel).
__device__ inline void clips_mode_resolve(unsigned count, unsigned last1, unsigned long long *skey, int32_t *out)
{
    const unsigned long long key = clips_mode_key(count, last1);
    skey[threadIdx.x] = key;
    __syncthreads();
    for (int s = kClipsModeThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) skey[threadIdx.x] = max(skey[threadIdx.x], skey[threadIdx.x + s]);
        __syncthreads();
    }
    if (count != 0u && key == skey[0]) *out = (int32_t)threadIdx.x;
}

// An entry whose frame index lies outside [0, n_frames) reads nothing and reports -1.
__device__ inline bool clips_mode_frame(const ClipsModeGeo &g, int b, const uint8_t *&img)
{
    const long long fi = g.frame_index ? (long long)g.frame_index[b] : (long long)b;
    if (fi < 0 || fi >= g.n_frames) return false;
    img = g.frames + fi * g.frame_stride;
    return true;
}

// Many frames: one workgroup per frame, both tables in LDS, the winner resolved by the same workgroup.
static __global__ __launch_bounds__(kClipsModeThreads) void clips_mode_frame_kernel(ClipsModeGeo g, int32_t *__restrict__ out)
{
    __shared__ unsigned shist[256], slast[256];
    __shared__ unsigned long long skey[256];
    const int b = (int)blockIdx.x;
    const uint8_t *img = nullptr;
    if (!clips_mode_frame(g, b, img)) { // (the same for the whole workgroup)
        if (threadIdx.x == 0) out[b] = -1;
        return;
    }
    shist[threadIdx.x] = 0;
    slast[threadIdx.x] = 0;
    __syncthreads();
    clips_mode_accumulate(img, g.row_stride, g.h, g.w, g.cpr, 0, kClipsModeThreads, shist, slast);
    __syncthreads();
    clips_mode_resolve(shist[threadIdx.x], slast[threadIdx.x], skey, out + b);
}

// Few large frames: g.parts workgroups per frame, each flushes its LDS tables into the frame's zeroed global table
// (512 words: counts, last occurrences); clips_mode_resolve_kernel, next on the stream, picks the winners.
static __global__ __launch_bounds__(kClipsModeThreads) void clips_mode_part_kernel(ClipsModeGeo g, unsigned *__restrict__ table)
{
    __shared__ unsigned shist[256], slast[256];
    const int e = (int)(blockIdx.x / (unsigned)g.parts), part = (int)(blockIdx.x % (unsigned)g.parts);
    const uint8_t *img = nullptr;
    if (!clips_mode_frame(g, e, img)) return;
    shist[threadIdx.x] = 0;
    slast[threadIdx.x] = 0;
    __syncthreads();
    clips_mode_accumulate(img, g.row_stride, g.h, g.w, g.cpr, (long long)part * kClipsModeThreads, (long long)g.parts * kClipsModeThreads, shist, slast);
    __syncthreads();
    if (shist[threadIdx.x]) {
        unsigned *tab = table + 512ll * e;
        atomicAdd(&tab[threadIdx.x], shist[threadIdx.x]);
        atomicMax(&tab[256 + threadIdx.x], slast[threadIdx.x]);
    }
}

static __global__ __launch_bounds__(kClipsModeThreads) void clips_mode_resolve_kernel(ClipsModeGeo g, const unsigned *__restrict__ table,
                                                                                 int32_t *__restrict__ out)
{
    __shared__ unsigned long long skey[256];
    const int b = (int)blockIdx.x;
    const uint8_t *img = nullptr;
    if (!clips_mode_frame(g, b, img)) {
        if (threadIdx.x == 0) out[b] = -1;
        return;
    }
    const unsigned *tab = table + 512ll * b;
    clips_mode_resolve(tab[threadIdx.x], tab[256 + threadIdx.x], skey, out + b);
}

// ---- the walk over many clips (pdog_clips_track) ----
// Slot p of the plan is clip order[p]; guess, step and frame index are per slot, so a fill group is a contiguous slice of
// all three.  Before the first frame: every slot's frame index (its clip's first frame) and first guess; with first = 1
// the start of every clip that has a first frame is also its first position, copied as given (src/PawsomeTracker.jl:104,
// :161).  len = NULL: every clip has n_frames frames.
static __global__ void clips_init_kernel(const int32_t *__restrict__ order, int n_slots, int n_clips, int n_frames, int first,
                                         const int32_t *__restrict__ len, const int32_t *__restrict__ start,
                                         int32_t *__restrict__ fidx, int32_t *__restrict__ guess, int32_t *__restrict__ out)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p < n_slots) {
        const int c = order[p];
        fidx[p] = c * n_frames;
        guess[2 * p] = start[2 * c];
        guess[2 * p + 1] = start[2 * c + 1];
    }
    if (first && p < n_clips && (len ? len[p] : n_frames) >= 1) {
        const long long o = 2ll * p * n_frames;
        out[o] = start[2 * p];
        out[o + 1] = start[2 * p + 1];
    }
}

} // namespace pdog
