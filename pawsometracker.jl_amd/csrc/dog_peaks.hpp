// dog_peaks.hpp — the K best, mutually separated peaks of a window's FP32 response map (include/pawsome_peaks.h states
// the rule; tests/peaks_restatement.py restates it in NumPy and this kernel is held to that bit for bit).
//
// THE RULE in short, for a window with guess g, radii r and an H x W frame, over its column-major map R
// (idx = col * n1 + row, window pixel (row, col) = frame pixel (g1 - r1 + row, g2 - r2 + col)):
//   pick 1        the position the detect kernels returned for the window (exact mode's, clamped, :61); value = max of R
//   candidates    window pixels inside the frame, no NaN, local maxima among their up to eight neighbours in the window:
//                 R(p) > R(q) for a neighbour of smaller idx, R(p) >= R(q) for one of larger idx
//   pick k >= 2   the candidate of largest R (ties: smallest idx) whose squared distance to EVERY earlier pick, in integers,
//                 is at least min_distance²; the selection ends when none is left
//   outputs       count in 1 … K, 1-based (row, col), FP32 values; beyond count (0, 0) and −inf
// Picks 2 … K are ranked in FP32 on whichever family's map this is: exact mode (dog_exact.hpp) decides pick 1 only.
//
// THE KERNEL.  One workgroup of PEAKS_NT threads per window, no wait between workgroups, no dynamic LDS.
//   Phase A  one pass over the map, thread t at idx = t, t + PEAKS_NT, …: consecutive lanes hold consecutive rows of a column,
//            so the centre loads are coalesced; the eight neighbours of a pixel are re-read through L1/L2 (they were the
//            centres of the lanes beside it and of the two neighbouring columns a few iterations away), in two stages of
//            independent loads: the two same-column neighbours beside the centre, then — for the pixels still standing — the
//            six of the columns left and right.  The pass keeps the window's maximum (pick 1's value) and appends every
//            candidate (value, idx) to a list in LDS.  The append order is whatever the atomics make it; nothing below
//            depends on it: idx breaks every tie.  K = 1 needs the maximum only and builds no list.
//   Phase B  up to K − 1 rounds over the list.  A round kills the entries the NEWEST pick suppresses (idx := −1; an entry is
//            always visited by the same thread) and takes the masked argmax of the rest — per thread, then per wave (two DPP
//            reductions: the maximum, then the smallest idx among the lanes that hold it), then across the waves through LDS.
//   Overflow A window with more candidates than the list holds (PEAKS_LIST entries), or a launch with no_list set, runs its
//            rounds over the map itself: in-frame test, value against the thread's best, distance to every earlier pick (held
//            in LDS), and last the local-maximum test.  Same picks, K − 1 passes over the map instead of one.
// Bounds: every load of R is at b * n1 * n2 + idx with 0 <= idx < n1 * n2 (neighbours are tested against the window's edges
// first); the guess only enters the in-frame test and is widened to 64 bits there, so a wild device guess reads nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pdog {
namespace peaks {

constexpr int PEAKS_NT = 1024;     // threads per workgroup (sixteen waves: a large window is one workgroup's to walk)
constexpr int PEAKS_MAX_K = 32;    // PDOG_PEAKS_MAX_K
constexpr int PEAKS_LIST = 1536;   // candidates the LDS list holds (8 B each, 12 KiB): a noise-only 271 x 481 window at l = 65 has ~1100 … 1300
constexpr int kNoIdx = 0x7fffffff;

struct PeaksGeo {
    const float *resp;          // [n][n2][n1] maps
    const int32_t *guesses;     // [n][2]
    const int32_t *ij1;         // [n][2] what the detect kernels returned: pick 1
    int32_t *out_ij;            // [n][k][2]
    float *out_peak;            // [n][k] or null
    int32_t *out_count;         // [n] or null
    unsigned long long *stat;   // [0] windows served, [1] windows whose list overflowed
    long long md2;              // min_distance²
    int n1, n2, r1, r2, fh, fw, k, no_list;
};

// The DPP steps of dog_kernels.hpp's wave_reduce_bits (quad xor 1, xor 2, mirrors in 8 and 16, row broadcasts): lane 63 ends
// up with the wave's result, handed back uniform.
template <typename F>
__device__ __forceinline__ int wave_reduce(int v, F op)
{
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false));
    return __builtin_amdgcn_readlane(v, 63);
}
// (value descending, idx ascending) over the wave: the maximum, then the smallest idx among the lanes that hold it.  No lane
// holds a NaN; a lane without an entry holds (−inf, kNoIdx).
__device__ __forceinline__ void wave_argmax(float &v, int &idx)
{
    const float m = __builtin_bit_cast(float, wave_reduce(__builtin_bit_cast(int, v), [](int a, int b) {
        return __builtin_bit_cast(int, fmaxf(__builtin_bit_cast(float, a), __builtin_bit_cast(float, b)));
    }));
    idx = wave_reduce(v == m ? idx : kNoIdx, [](int a, int b) { return a < b ? a : b; });
    v = m;
}

// (b) of the rule for window pixel (row, col), value v = R[idx] (no NaN), in two stages of independent loads — a chain of nine
// dependent loads per pixel is what the pass would otherwise wait for.  Stage 1: the two neighbours in the pixel's own column
// (vu above, vd below; the caller loads them beside the centre).  It lets about one pixel in three through on noise, far fewer
// on a smooth map.
__device__ __forceinline__ bool column_max(bool up, bool down, float v, float vu, float vd)
{
    return (!up || v > vu) && (!down || v >= vd);
}
// Stage 2: the six neighbours in the two columns beside it, loaded together.
__device__ __forceinline__ bool side_columns_max(const float *__restrict__ R, int n1, int n2, int row, int col, int idx, float v)
{
    const bool up = row > 0, down = row + 1 < n1, left = col > 0, right = col + 1 < n2;
    const float ninf = -__builtin_huge_valf();
    const int il = idx - n1, ir = idx + n1; // the same row in the column to the left / right
    const float l0 = left && up ? R[il - 1] : ninf, l1 = left ? R[il] : ninf, l2 = left && down ? R[il + 1] : ninf;
    const float r0 = right && up ? R[ir - 1] : ninf, r1 = right ? R[ir] : ninf, r2 = right && down ? R[ir + 1] : ninf;
    const bool lok = !left || ((!up || v > l0) && v > l1 && (!down || v > l2));
    const bool rok = !right || ((!up || v >= r0) && v >= r1 && (!down || v >= r2));
    return lok && rok;
}
__device__ __forceinline__ bool is_local_max(const float *__restrict__ R, int n1, int n2, int row, int col, int idx, float v)
{
    const bool up = row > 0, down = row + 1 < n1;
    const float ninf = -__builtin_huge_valf();
    const float vu = up ? R[idx - 1] : ninf, vd = down ? R[idx + 1] : ninf;
    return column_max(up, down, v, vu, vd) && side_columns_max(R, n1, n2, row, col, idx, v);
}

__global__ __launch_bounds__(PEAKS_NT) void dog_peaks_kernel(const PeaksGeo g)
{
    __shared__ float s_val[PEAKS_LIST];
    __shared__ int s_idx[PEAKS_LIST];
    __shared__ float s_wv[2][PEAKS_NT / 64];
    __shared__ int s_wi[2][PEAKS_NT / 64];
    __shared__ int s_pick[PEAKS_MAX_K][2];
    __shared__ int s_count;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n1 = g.n1, n2 = g.n2, npix = n1 * n2;
    const float *__restrict__ R = g.resp + (long long)b * npix;
    const float ninf = -__builtin_huge_valf();
    // frame coordinates (1-based) of window pixel (0, 0); 64 bits: a device guess may be anything
    const long long f1 = (long long)g.guesses[2 * b] - g.r1, f2 = (long long)g.guesses[2 * b + 1] - g.r2;
    // the window's rows and columns that lie inside the frame: row in [ra, rb), col in [ca, cb)
    const int ra = (int)min(max(1 - f1, 0LL), (long long)n1), rb = (int)min(max(g.fh + 1 - f1, 0LL), (long long)n1);
    const int ca = (int)min(max(1 - f2, 0LL), (long long)n2), cb = (int)min(max(g.fw + 1 - f2, 0LL), (long long)n2);
    if (tid == 0) s_count = 0;
    __syncthreads();

    // ---- phase A: the window's maximum and the candidate list (no list for K = 1: pick 1 needs the maximum only) ----
    const bool want_list = !g.no_list && g.k > 1;
    float bv = ninf;
    int bi = kNoIdx;
    for (int base = 0; base < npix; base += PEAKS_NT) { // (uniform trip count: the ballot below wants whole waves)
        const int idx = base + tid;
        bool cand = false;
        float v = 0.f;
        if (idx < npix) {
            const int col = idx / n1, row = idx - col * n1;
            const bool in = want_list && row >= ra && row < rb && col >= ca && col < cb;
            const bool up = row > 0, down = row + 1 < n1;
            v = R[idx];
            const float vu = in && up ? R[idx - 1] : ninf, vd = in && down ? R[idx + 1] : ninf;
            if (v > bv || (v == bv && bi == kNoIdx)) { bv = v; bi = idx; } // the first idx of the maximum; a NaN never enters
            if (in && v == v && column_max(up, down, v, vu, vd)) cand = side_columns_max(R, n1, n2, row, col, idx, v);
        }
        const unsigned long long m = __ballot(cand);
        if (m) {
            int slot = 0;
            if (lane == 0) slot = atomicAdd(&s_count, __popcll(m));
            slot = __builtin_amdgcn_readfirstlane(slot) + __popcll(m & ((1ull << lane) - 1ull));
            if (cand && slot < PEAKS_LIST) { s_val[slot] = v; s_idx[slot] = idx; }
        }
    }
    wave_argmax(bv, bi);
    if (lane == 0) { s_wv[0][wave] = bv; s_wi[0][wave] = bi; }
    __syncthreads();
    float wmax = ninf;
    int wmax_i = kNoIdx;
    for (int w = 0; w < PEAKS_NT / 64; ++w) {
        const float ov = s_wv[0][w];
        const int oi = s_wi[0][w];
        if (ov > wmax || (ov == wmax && oi < wmax_i)) { wmax = ov; wmax_i = oi; }
    }
    const int total = s_count;
    const bool scan_map = g.no_list || total > PEAKS_LIST;
    const int cnt = scan_map ? 0 : total;

    // ---- pick 1: the detect kernels' position, the map's maximum ----
    int pi = g.ij1[2 * b], pj = g.ij1[2 * b + 1];
    int32_t *out_ij = g.out_ij + (long long)b * g.k * 2;
    float *out_peak = g.out_peak ? g.out_peak + (long long)b * g.k : nullptr;
    if (tid == 0) {
        out_ij[0] = pi;
        out_ij[1] = pj;
        if (out_peak) out_peak[0] = wmax_i == kNoIdx ? ninf : R[wmax_i];
        s_pick[0][0] = pi;
        s_pick[0][1] = pj;
        atomicAdd(g.stat, 1ull);
        if (!g.no_list && total > PEAKS_LIST) atomicAdd(g.stat + 1, 1ull);
    }
    __syncthreads();

    // ---- phase B: greedy rounds ----
    int count = 1;
    for (; count < g.k; ++count) {
        bv = ninf;
        bi = kNoIdx;
        if (!scan_map) {
            for (int e = tid; e < cnt; e += PEAKS_NT) {
                const int idx = s_idx[e];
                if (idx < 0) continue;
                const int col = idx / n1, row = idx - col * n1;
                const long long di = f1 + row - pi, dj = f2 + col - pj; // in-frame candidate, in-frame pick: small
                if (di * di + dj * dj < g.md2) { s_idx[e] = -1; continue; }
                const float v = s_val[e];
                if (v > bv || (v == bv && idx < bi)) { bv = v; bi = idx; }
            }
        } else {
            for (int idx = tid; idx < npix; idx += PEAKS_NT) {
                const int col = idx / n1, row = idx - col * n1;
                if (!(row >= ra && row < rb && col >= ca && col < cb)) continue;
                const float v = R[idx];
                if (!(v > bv || (v == bv && bi == kNoIdx))) continue; // (the thread's idx only grows; a NaN fails both)
                bool free_ = true;
                for (int p = 0; p < count && free_; ++p) {
                    const long long di = f1 + row - s_pick[p][0], dj = f2 + col - s_pick[p][1];
                    free_ = di * di + dj * dj >= g.md2;
                }
                if (free_ && is_local_max(R, n1, n2, row, col, idx, v)) { bv = v; bi = idx; }
            }
        }
        wave_argmax(bv, bi);
        const int par = count & 1; // (two sets of slots: a wave may write the next round's while another still reads this one's)
        if (lane == 0) { s_wv[par][wave] = bv; s_wi[par][wave] = bi; }
        __syncthreads();
        float pv = ninf;
        int pidx = kNoIdx;
        for (int w = 0; w < PEAKS_NT / 64; ++w) {
            const float ov = s_wv[par][w];
            const int oi = s_wi[par][w];
            if (ov > pv || (ov == pv && oi < pidx)) { pv = ov; pidx = oi; }
        }
        if (pidx == kNoIdx) break; // uniform: every thread read the same slots
        const int col = pidx / n1, row = pidx - col * n1;
        pi = (int)(f1 + row);
        pj = (int)(f2 + col);
        if (tid == 0) {
            out_ij[2 * count] = pi;
            out_ij[2 * count + 1] = pj;
            if (out_peak) out_peak[count] = R[pidx]; // (the entry's own bits: pv may be the other zero)
            s_pick[count][0] = pi;
            s_pick[count][1] = pj;
        }
        if (scan_map) __syncthreads(); // the next round reads s_pick
    }
    for (int e = count + tid; e < g.k; e += PEAKS_NT) {
        out_ij[2 * e] = 0;
        out_ij[2 * e + 1] = 0;
        if (out_peak) out_peak[e] = ninf;
    }
    if (tid == 0 && g.out_count) g.out_count[b] = count;
}

} // namespace peaks
} // namespace pdog
