// dog_frame_blobs.hpp — the kernels of the frame-blob rule (include/pawsome_frame_blobs.h states it and says why every loop
// ends; pdog_frame_blobs.hpp holds the arithmetic on row words).  pawsome_frame_blobs.hip alone includes this file.
//
// A label is a pixel index r * w + c of the frame, -1 outside the mask; a blob's label is its smallest index, its `first`.
// Seven kernels per round of steps, each a launch of its own, so that what one writes the next one reads behind a kernel
// boundary; inside a kernel, workgroups meet only in atomics, and the labels that several workgroups lower are read with
// relaxed agent-scope loads.  grid.y is the step of the round.
//   (a) fb_label_kernel     one workgroup per 64 x 64 tile.  Four lanes load a tile row's 64 pixels, 16 bytes each, and build
//                           its row word in LDS.  The nodes of the tile's union-find are the RUNS of the row words (a run's
//                           pixels are joined already); a lane joins its 16 columns' links to the row above (links_up, and
//                           links_left / links_right for connectivity 8) with atomic minima in LDS.  Every pixel then gets the
//                           global index of its run's root, which is the tile-local `first`.
//   (b) fb_merge_kernel     one lane per pixel of a tile's first row, first column and (connectivity 8) last column: the pairs
//                           of neighbours that a tile border separates, joined in the global label array — corners too.
//   (c) fb_flatten_kernel   every mask pixel finds its root and stores it; the roots' areas are counted, a wave adding once
//                           per stretch of lanes that share a root.
//   (d) fb_count_kernel, fb_scan_kernel, fb_rank_kernel
//                           roots are the pixels with label == own index.  Blocks of the raster count their kept roots, one
//                           workgroup per step scans the counts, and the blocks then number their kept roots in raster
//                           order — no cursor whose value depends on arrival.  The roots' area words are REUSED for the
//                           rank (or -1: filtered out, or behind the cap), and the kept blobs' rows get their start values.
//   (e) fb_sums_kernel      a wave per 64 pixels of a row: the stretches of lanes that share a kept blob add their closed sums
//                           (run_sums) and the contrasts' sum, taken from a wave prefix sum, with 64-bit integer atomics.
// LAYOUTS.  Frames are addressed by column: any base, any row stride >= w.  A 16-byte piece inside the row is loaded
// unaligned, whole; the row's last piece is loaded byte by byte up to column w.  Lanes beyond the frame hold no mask bit and
// store nothing.
#pragma once
#include <hip/hip_runtime.h>
#include "pdog_frame_blobs.hpp"

namespace pdog {
namespace fblobs {

constexpr int kLabelThreads = 256; // 64 rows x 4 pieces of 16 columns
constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;

struct Geo {
    const uint8_t *frames;
    const int32_t *table;  // device: this round's steps, checked on the host
    int32_t *labels;       // [steps in flight][h * w]
    int32_t *area;         // [steps in flight][h * w]: a root's pixel count, then its rank
    int32_t *block_counts; // [steps in flight][n_blocks]: kept roots per block of kThreads pixels, then their offsets
    int64_t *out_words;    // this round's first row: [steps][cap][12]
    int32_t *out_count;    // this round's first pair: [steps][2]
    int64_t frame_stride, row_stride, min_area, max_area;
    int h, w, n_pix, n_blocks, level, darker, min_contrast, conn8, cap;
};

__device__ __forceinline__ int load_label(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// find and union (pdog_frame_blobs.hpp) on labels in global memory and, with kLds, in LDS
template <bool kLds>
__device__ __forceinline__ int uf_find(int32_t *par, int x)
{
    return uf_find([par](int i) { return kLds ? __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : load_label(par + i); },
                   [par](int i, int v) { return atomicMin(par + i, v); }, x);
}
template <bool kLds>
__device__ __forceinline__ void uf_union(int32_t *par, int a, int b)
{
    uf_union([par](int i) { return kLds ? __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : load_label(par + i); },
             [par](int i, int v) { return atomicMin(par + i, v); }, a, b);
}

// ---- (a) ----
// 16 pixels of a row from column c on as mask bits; nothing at or behind column w is read
__device__ __forceinline__ uint32_t mask16(const uint8_t *row, int c, int w, int level, bool darker, int min_contrast)
{
    uint32_t bits = 0;
    if (c + 16 <= w) {
        uint4 v;
        __builtin_memcpy(&v, row + c, 16);
        const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) bits |= (uint32_t)(contrast((int)((d[j >> 2] >> (8 * (j & 3))) & 255u), level, darker) >= min_contrast) << j;
        return bits;
    }
    for (int j = 0; c + j < w; ++j) bits |= (uint32_t)(contrast((int)row[c + j], level, darker) >= min_contrast) << j;
    return bits;
}

// grid (tiles across, tiles down, steps)
__global__ __launch_bounds__(kLabelThreads) void fb_label_kernel(const Geo g)
{
    __shared__ uint16_t s_bits[kTile * 4];
    __shared__ int32_t s_par[kTile * kTile];
    __shared__ int s_count;
    const int t = threadIdx.x, r = t >> 2, q = t & 3, step = blockIdx.z;
    const int row = blockIdx.y * kTile + r, col = blockIdx.x * kTile + 16 * q;
    if (t == 0) s_count = 0;
    uint32_t bits = 0;
    if (row < g.h && col < g.w)
        bits = mask16(g.frames + (int64_t)g.table[step] * g.frame_stride + (int64_t)row * g.row_stride, col, g.w, g.level, g.darker != 0, g.min_contrast);
    s_bits[t] = (uint16_t)bits;
#pragma unroll
    for (int j = 0; j < 16; ++j) s_par[r * kTile + 16 * q + j] = r * kTile + 16 * q + j;
    __syncthreads();
    if (bits) atomicAdd(&s_count, __popc(bits));
    const auto word = [&](int rr) {
        return (uint64_t)s_bits[4 * rr] | (uint64_t)s_bits[4 * rr + 1] << 16 | (uint64_t)s_bits[4 * rr + 2] << 32 | (uint64_t)s_bits[4 * rr + 3] << 48;
    };
    const uint64_t m = word(r), up = r ? word(r - 1) : 0, mine = 0xffffull << (16 * q);
    // the links of this lane's 16 columns to the row above
    for (uint64_t l = links_up(m, up) & mine; l; l &= l - 1) {
        const int c = __builtin_ctzll(l);
        uf_union<true>(s_par, r * kTile + run_start(m, c), (r - 1) * kTile + run_start(up, c));
    }
    if (g.conn8) {
        for (uint64_t l = links_left(m, up) & mine; l; l &= l - 1) {
            const int c = __builtin_ctzll(l);
            uf_union<true>(s_par, r * kTile + run_start(m, c), (r - 1) * kTile + run_start(up, c - 1));
        }
        for (uint64_t l = links_right(m, up) & mine; l; l &= l - 1) {
            const int c = __builtin_ctzll(l);
            uf_union<true>(s_par, r * kTile + run_start(m, c), (r - 1) * kTile + run_start(up, c + 1));
        }
    }
    __syncthreads();
    // every run that starts in this lane's columns points at its root
    for (uint64_t l = run_starts(m) & mine; l; l &= l - 1) {
        const int node = r * kTile + __builtin_ctzll(l);
        __hip_atomic_store(s_par + node, uf_find<true>(s_par, node), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (t == 0 && s_count) atomicAdd(g.out_count + 2 * step + 1, s_count);
    if (row >= g.h || col >= g.w) return;
    int32_t *out = g.labels + (int64_t)step * g.n_pix + (int64_t)row * g.w + col;
    int32_t lab[16];
    int cur = -1;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = 16 * q + j;
        if ((m >> c) & 1) {
            if (cur < 0) {
                const int root = s_par[r * kTile + run_start(m, c)];
                cur = (blockIdx.y * kTile + (root >> 6)) * g.w + blockIdx.x * kTile + (root & 63);
            }
        } else {
            cur = -1;
        }
        lab[j] = cur;
    }
    if (col + 16 <= g.w && (g.w & 3) == 0) { // 16-byte stores where every row of every step begins on a multiple of 16 bytes
#pragma unroll
        for (int j = 0; j < 16; j += 4) *reinterpret_cast<int4 *>(out + j) = make_int4(lab[j], lab[j + 1], lab[j + 2], lab[j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (col + j < g.w) out[j] = lab[j];
    }
}

// ---- (b) ----
// Items: the pixels of every tile row's first row (n_hb rows of w), then of every tile column's first column (n_vb columns of
// h), then, for connectivity 8, of the last column before each of those.  grid (ceil(items / kThreads), steps)
__global__ __launch_bounds__(kThreads) void fb_merge_kernel(const Geo g)
{
    int32_t *L = g.labels + (int64_t)blockIdx.y * g.n_pix;
    const int n_hb = (g.h - 1) / kTile, n_vb = (g.w - 1) / kTile, w = g.w;
    int idx = blockIdx.x * kThreads + threadIdx.x;
    const auto at = [&](int r, int c) { return r >= 0 && r < g.h && c >= 0 && c < w ? L[r * w + c] : -1; };
    if (idx < n_hb * w) { // pairs with the row above, across a horizontal border
        const int r = (idx / w + 1) * kTile, c = idx % w;
        if (at(r, c) < 0) return;
        if (at(r - 1, c) >= 0) {
            uf_union<false>(L, r * w + c, (r - 1) * w + c);
        } else if (g.conn8) { // (with (r-1, c) set, its own joins reach (r-1, c-1) and (r-1, c+1))
            if (at(r - 1, c - 1) >= 0) uf_union<false>(L, r * w + c, (r - 1) * w + c - 1);
            if (at(r - 1, c + 1) >= 0) uf_union<false>(L, r * w + c, (r - 1) * w + c + 1);
        }
        return;
    }
    idx -= n_hb * w;
    if (idx < n_vb * g.h) { // pairs with the column to the left, across a vertical border
        const int c = (idx / g.h + 1) * kTile, r = idx % g.h;
        if (at(r, c) < 0) return;
        if (at(r, c - 1) >= 0) {
            uf_union<false>(L, r * w + c, r * w + c - 1);
        } else if (g.conn8 && at(r - 1, c - 1) >= 0) { // (with (r, c-1) set, its own join reaches (r-1, c-1))
            uf_union<false>(L, r * w + c, (r - 1) * w + c - 1);
        }
        return;
    }
    idx -= n_vb * g.h;
    if (g.conn8 && idx < n_vb * g.h) { // the pair up and to the right, across a vertical border
        const int c = (idx / g.h + 1) * kTile - 1, r = idx % g.h;
        if (at(r, c) >= 0 && at(r - 1, c) < 0 && at(r - 1, c + 1) >= 0) uf_union<false>(L, r * w + c, (r - 1) * w + c + 1);
    }
}

// ---- (c) ----
// grid (n_blocks, steps)
__global__ __launch_bounds__(kThreads) void fb_flatten_kernel(const Geo g)
{
    int32_t *L = g.labels + (int64_t)blockIdx.y * g.n_pix;
    const int p = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
    int root = -1;
    if (p < g.n_pix) {
        const int l = load_label(L + p);
        if (l >= 0) {
            root = uf_find<false>(L, l);
            if (root != l) __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // one add per stretch of lanes that share a root
    const int before = __shfl_up(root, 1);
    const uint64_t bounds = __ballot(lane == 0 || root != before);
    if (root >= 0 && ((bounds >> lane) & 1)) atomicAdd(g.area + (int64_t)blockIdx.y * g.n_pix + root, next_bound(bounds, lane) - lane);
}

// ---- (d) ----
// whether pixel p is a kept root, and the exclusive count of kept roots below it in its block (*total: the block's count)
__device__ __forceinline__ bool kept_root(const Geo &g, int step, int p, int *below, int *total)
{
    __shared__ int s_wave[kThreads / 64];
    bool kept = false;
    if (p < g.n_pix && g.labels[(int64_t)step * g.n_pix + p] == p) {
        const int64_t n = g.area[(int64_t)step * g.n_pix + p];
        kept = n >= g.min_area && n <= g.max_area;
    }
    const uint64_t b = __ballot(kept);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) {
        off += k < wave ? s_wave[k] : 0;
        sum += s_wave[k];
    }
    *below = off + __popcll(b & ((1ull << lane) - 1));
    *total = sum;
    return kept;
}

__global__ __launch_bounds__(kThreads) void fb_count_kernel(const Geo g)
{
    int below, total;
    kept_root(g, blockIdx.y, blockIdx.x * kThreads + threadIdx.x, &below, &total);
    if (threadIdx.x == 0) g.block_counts[(int64_t)blockIdx.y * g.n_blocks + blockIdx.x] = total;
}

// one workgroup per step: the blocks' counts become their exclusive prefix sums, the total the step's count
__global__ __launch_bounds__(kScanThreads) void fb_scan_kernel(const Geo g)
{
    __shared__ int s_wave[kScanThreads / 64];
    __shared__ int s_run;
    int32_t *counts = g.block_counts + (int64_t)blockIdx.x * g.n_blocks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (int base = 0; base < g.n_blocks; base += kScanThreads) {
        const int i = base + threadIdx.x;
        const int v = i < g.n_blocks ? counts[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int off = s_run, sum = 0;
        for (int k = 0; k < kScanThreads / 64; ++k) {
            off += k < wave ? s_wave[k] : 0;
            sum += s_wave[k];
        }
        if (i < g.n_blocks) counts[i] = off + incl - v;
        __syncthreads();
        if (threadIdx.x == 0) s_run += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) g.out_count[2 * blockIdx.x] = s_run;
}

__global__ __launch_bounds__(kThreads) void fb_rank_kernel(const Geo g)
{
    const int step = blockIdx.y, p = blockIdx.x * kThreads + threadIdx.x;
    int below, total;
    const bool kept = kept_root(g, step, p, &below, &total);
    if (p >= g.n_pix || g.labels[(int64_t)step * g.n_pix + p] != p) return;
    int rank = -1;
    if (kept) {
        rank = g.block_counts[(int64_t)step * g.n_blocks + blockIdx.x] + below;
        if (rank >= g.cap) rank = -1;
    }
    g.area[(int64_t)step * g.n_pix + p] = rank; // (this lane alone reads and writes a root's word in this kernel)
    if (rank < 0) return;
    int64_t *o = g.out_words + ((int64_t)step * g.cap + rank) * kWords; // (zero so far)
    o[W_RMIN] = g.h;
    o[W_RMAX] = -1;
    o[W_CMIN] = g.w;
    o[W_CMAX] = -1;
    o[W_FIRST] = p;
}

// ---- (e) ----
__device__ __forceinline__ void add64(int64_t *p, int64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

// a wave per 64 pixels of a row; grid (ceil(h * ceil(w / 64) / 4), steps)
__global__ __launch_bounds__(kThreads) void fb_sums_kernel(const Geo g)
{
    const int step = blockIdx.y, lane = threadIdx.x & 63, wpr = (g.w + 63) / 64;
    const int item = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (item >= g.h * wpr) return; // (the whole wave)
    const int row = item / wpr, col = (item % wpr) * 64 + lane;
    int rank = -1, s = 0;
    if (col < g.w) {
        const int l = g.labels[(int64_t)step * g.n_pix + row * g.w + col];
        if (l >= 0) rank = g.area[(int64_t)step * g.n_pix + l];
        if (rank >= 0) s = contrast((int)g.frames[(int64_t)g.table[step] * g.frame_stride + (int64_t)row * g.row_stride + col], g.level, g.darker != 0);
    }
    int incl = s; // the contrasts' prefix sum over the wave: at most 64 * 255
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    const int before = __shfl_up(rank, 1);
    const uint64_t bounds = __ballot(lane == 0 || rank != before);
    const int end = next_bound(bounds, lane);         // one past the stretch's last lane
    const int upto = __shfl(incl, end - 1), excl = incl - s;
    if (rank < 0 || !((bounds >> lane) & 1)) return;
    int64_t n, sx, sxx;
    const int64_t a = col, b = col + (end - lane) - 1, y = row;
    run_sums(a, b, &n, &sx, &sxx);
    int64_t *o = g.out_words + ((int64_t)step * g.cap + rank) * kWords;
    add64(o + W_N, n);
    add64(o + W_SY, n * y);
    add64(o + W_SX, sx);
    add64(o + W_SYY, n * y * y);
    add64(o + W_SYX, y * sx);
    add64(o + W_SXX, sxx);
    add64(o + W_SS, (int64_t)(upto - excl));
    atomicMin(reinterpret_cast<long long *>(o + W_RMIN), (long long)y);
    atomicMax(reinterpret_cast<long long *>(o + W_RMAX), (long long)y);
    atomicMin(reinterpret_cast<long long *>(o + W_CMIN), (long long)a);
    atomicMax(reinterpret_cast<long long *>(o + W_CMAX), (long long)b);
}

} // namespace fblobs
} // namespace pdog
