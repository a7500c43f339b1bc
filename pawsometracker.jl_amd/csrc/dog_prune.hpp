// dog_prune.hpp — the pre-pass of the roll family's batch path: which sub-chunks of which strips can hold the window's peak.
//
// A step's result is one position per window plus exact mode's decision whether a near-tie exists.  Most of a window
// provably holds neither, and the roll kernel (dog_roll.hpp) is at its instruction-issue limit: the only work left to take
// out is work the result does not need.  This kernel reads every window's padded tile once and leaves, per strip and per
// remainder column, the contiguous range of 8-row output blocks that the roll / thin kernels must still compute.
//
// THE BOUND.  A response is f(p) = Σ K·v / 255 with v = pixel − dc, the values the kernels convolve (fill outside the frame,
// the window's own DC level).  By Cauchy–Schwarz |f(p)| ≤ ‖K‖₂ · ‖v‖₂(the inputs p sees) / 255.  ‖K‖₂ comes from the host in
// double, rounded up (pdog_math.cpp, dog_kernel_norm_up).  The energies are exact integers:
//     E[slot][sc] = Σ v² over the 8 tile rows of sub-chunk sc × the tile columns the slot's outputs read
//                   (a strip of w ≤ 64 columns: w + l − 1; a remainder column: l),
// and output block j (rows 8j … 8j+7) of a slot sees sub-chunks j … j + prune_span(l) − 1 (nine at l = 65).  What the FP32
// kernels compute differs from f by at most the family's δ(V) = (T/2)·V/255 (dog_exact.hpp, exact_factors; T = ExactCtl::T is
// 2δ at V = 255), V = max |v| over the window's tile.  No other error constant enters.
//
// THE LOWER BOUND L on the window's maximum is the response at 8 × 8 output pixels, chosen from the 8 × 8-pixel cell sums the
// energy pass builds on its way: around the cell whose direction-signed 3 × 3-cell sum is largest.  Any set is valid; a better
// one only prunes more.  They are evaluated in the roll family's own operation order (row pass: pairs ascending, centre last,
// both Gaussians per packed FMA; column pass: taps ascending, the g₊ term then the g₋ term into one f32 — dog_thin_kernel's
// statement of it), so L is a value the strips also produce; one δ(V) is subtracted all the same.
//
// A block is EXCLUDED iff  ‖K‖₂·sqrt(ΣE)/255 + δ(V) < L − δ(V) − T_max,  T_max the largest threshold a later stage uses at
// V = 255 (the flag's T and the rescan's T_rescan).  Per slot the kernel keeps the contiguous hull [y_a, y_b) of the blocks it
// cannot exclude, in whole blocks; an empty hull skips the slot.
//
// WHY POSITIONS AND FLAGS CANNOT CHANGE.  Let M be the window's computed maximum; L ≤ M, because L's pixels are computed by the
// strips too and their own block is never excluded (its bound is at least |f| ≥ L − δ).  An excluded pixel q has
// f(q) ≤ bound, so its computed response is below bound + δ(V) < L − δ(V) − T_max ≤ M − T_max: it is not the maximum, and it is
// not within the flag threshold or any rescan threshold of the maximum either.  The true runner-up, if it lies within T of M,
// is not excluded and is computed, so `best − second ≤ T` decides as before; `second` may differ only where the window is not
// flagged either way.  The reference's argmax p* has a computed response ≥ M − T: it is kept, its column's bit stands in its
// strip's mask (column maximum ≥ M − T ≥ strip maximum − T) and its strip passes the refinement's slot test, so a flagged
// window's refinement still finds it; every pixel the refinement no longer rescans has f(q) < f(p*) and could not have won.
// For columns that hold a pixel within T of M the masks of kept strips are unchanged.
//
// WHERE IT STOPS PAYING: where the background's energy under the kernel reaches the target's response (heavy noise or
// texture, noise-only and flat windows: nothing is excluded and the pre-pass is paid for nothing).  launch_strips reads the
// kept / total counts this kernel publishes and stops running it on such batches (pawsome_dog.hip, "pruning policy").
//
// The ranges travel in LaunchGeo::part_mask: slot [b][s] holds (first block | one past the last block << 32) when the roll /
// thin kernels start (LaunchGeo::prune) and the strip's column mask, as ever, when they end.
#pragma once
#include "dog_roll.hpp"

namespace pdog {

struct PruneGeo {
    LaunchGeo g;              // frames, guesses, geometry, nstrips / nthin / thin_x0 / nslots, ex.T, part_mask (receives the ranges)
    double kinv;              // 255 / ‖K‖₂ with ‖K‖₂ rounded up
    float tmax;               // T_max (header comment)
    int darker;               // sign of the cell sums that point at a target
    unsigned long long *stat; // [0] kept, [1] total (slot, sub-chunk) pairs since the tracker was created, [2] arrivals of the batch in flight
    unsigned long long *host; // one host-coherent word: the low halves of [0] and ([1] << 32) as the last workgroup of a batch saw them
};

constexpr int PRUNE_NT = 256;
constexpr int PRUNE_B = 8; // the L pixels: PRUNE_B × PRUNE_B outputs
struct PruneLds { size_t cell, E, R, patch, total; };
__host__ __device__ inline PruneLds prune_lds(int n1, int n2, int L, int nslots)
{
    const size_t NA = n1 + L - 1, nsub = (NA + ROLL_CH - 1) / ROLL_CH, ncx = (size_t)(n2 + L - 1 + 7) / 8;
    const size_t PH = PRUNE_B + L - 1, PP = (PH + 3) / 4 * 4;
    PruneLds o;
    o.cell = 0;
    o.E = o.cell + nsub * ncx * 4;
    o.R = (o.E + (size_t)nslots * nsub * 4 + 7) / 8 * 8;
    o.patch = o.R + PH * PRUNE_B * sizeof(f2);
    o.total = (o.patch + PH * PP + 15) / 16 * 16;
    return o;
}

#ifndef PDOG_ROLL_INST_ONLY
// One workgroup per window.
static __global__ __launch_bounds__(PRUNE_NT) void dog_prune_kernel(const PruneGeo pg, const f2 *__restrict__ taps_row, const f2 *__restrict__ taps_col)
{
    constexpr int NT = PRUNE_NT, NW = NT / 64, CH = ROLL_CH, TW = ROLL_TW, PB = PRUNE_B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LaunchGeo &g = pg.g;
    const int L = g.L, hw = L / 2, H = L / 2;
    const int NA = g.n1 + L - 1, TWin = g.n2 + L - 1, nsub = (NA + CH - 1) / CH, ncx = (TWin + 7) / 8, TQ = (TWin + 3) / 4;
    const PruneLds lo = prune_lds(g.n1, g.n2, L, g.nslots);
    int *cell = reinterpret_cast<int *>(smem + lo.cell);           // [nsub][ncx] Σ v over 8 × 8-pixel cells of the tile
    unsigned *E = reinterpret_cast<unsigned *>(smem + lo.E);       // [nslots][nsub]
    f2 *R = reinterpret_cast<f2 *>(smem + lo.R);                   // [PB + l − 1][PB] row-pass outputs of the L pixels
    uint8_t *patch = smem + lo.patch;                              // their input pixels
    __shared__ int s_sum[NW], s_v[NW], s_cv[NW], s_ci[NW], s_cellbest, s_kept;
    __shared__ double s_emax;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int g1 = g.guesses[2 * b], g2 = g.guesses[2 * b + 1];
    const int fidx = g.frame_index ? g.frame_index[b] : b;
    const uint8_t *__restrict__ frame = g.frames + (long long)fidx * g.frame_stride;
    const int ti0 = g1 - g.r1 - 1 - hw, wj0 = g2 - g.r2 - 1 - hw; // frame row / column of the tile's first pixel
    const tap_ptr trow = as_taps(taps_row), tcol = as_taps(taps_col);

    // ---- the window's DC level: the strips' samples and rounding ----
    int dc;
    {
        int sum = wave_sum(dc_sample_sum(g, frame, ti0, wj0, L, tid, NT));
        if (lane == 0) s_sum[wave] = sum;
        if (tid == 0) s_kept = 0;
        __syncthreads();
        int tot = 0;
        for (int w = 0; w < NW; ++w) tot += s_sum[w];
        dc = dc_from_sum(tot, g.fill);
    }

    // ---- energies: one item = the 8 rows of a band × one dword of columns; the items of the whole tile are dealt out to the
    // threads in order (consecutive lanes read consecutive dwords of a row: coalesced; 99 % of the lanes have work, where a
    // lane per dword of ONE row left 17 of 64 busy in the second pass over a 321-byte row).  An item adds its Σ v to its
    // 8 × 8 cell and its column energies to every slot that reads those columns, with LDS atomics (integers: exact in any
    // order).  Products through the 24-bit multiplier: |v| ≤ 255, and the full 32-bit multiply runs at a quarter of its rate ----
    const int ncols = g.nthin ? g.thin_x0 : g.n2; // window columns the strips cover
    const int ws = min(TW, ncols);
    for (int i = tid; i < nsub * ncx + g.nslots * nsub; i += NT) cell[i] = 0; // (E follows cell in the layout)
    __syncthreads();
    int vmax = 0;
    for (int it = tid; it < nsub * TQ; it += NT) {
        const int band = it / TQ, d = it - band * TQ;
        unsigned e[4] = {0u, 0u, 0u, 0u};
        int s = 0;
        const int gj = wj0 + 4 * d;
        const bool cols_in = gj >= 0 && gj + 4 <= g.fw && 4 * d + 4 <= TWin;
#pragma unroll
        for (int r = 0; r < CH; ++r) {
            const int a = band * CH + r, gi = ti0 + a;
            if (a >= NA) continue; // (rows past the tile are read by no output)
            int p[4];
            if (cols_in && gi >= 0 && gi < g.fh) {
                uint32_t w;
                __builtin_memcpy(&w, frame + (long long)gi * g.row_stride + gj, 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) p[i] = (int)((w >> (8 * i)) & 0xffu);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int gjj = gj + i;
                    p[i] = 4 * d + i >= TWin ? dc // (columns past the tile: v = 0)
                           : (gi >= 0 && gi < g.fh && gjj >= 0 && gjj < g.fw) ? (int)frame[(long long)gi * g.row_stride + gjj] : g.fill;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = p[i] - dc;
                e[i] += (unsigned)__mul24(v, v);
                s += v;
                vmax = max(vmax, abs(v));
            }
        }
        atomicAdd(&cell[band * ncx + (d >> 1)], s); // two dwords = one 8-column cell
        for (int sl = 0; sl < g.nslots; ++sl) {
            const bool strip = sl < g.nstrips;
            const int c0 = strip ? ((ncols >= TW) ? min(sl * TW, ncols - TW) : 0) : g.thin_x0 + (sl - g.nstrips);
            const int lo = c0 - 4 * d, hi = lo + (strip ? ws + L - 1 : L); // the slot's columns, counted from this dword's first
            unsigned sum = 0; // (a slot's band total is at most 8 · 212 · 255² < 2³¹)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i >= lo && i < hi) sum += e[i];
            if (sum) atomicAdd(&E[sl * nsub + band], sum);
        }
    }
    vmax = wave_reduce_bits(vmax, [](int a, int c) { return a > c ? a : c; });
    if (lane == 0) s_v[wave] = vmax;
    __syncthreads();

    // ---- where to take L: the cell whose direction-signed 3 × 3-cell sum is largest ----
    {
        int bv = -0x7fffffff, bi = 0;
        for (int c = tid; c < nsub * ncx; c += NT) {
            const int cy = c / ncx, cx = c - cy * ncx;
            int s = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = cy + dy, xx = cx + dx;
                    if (yy >= 0 && yy < nsub && xx >= 0 && xx < ncx) s += cell[yy * ncx + xx];
                }
            if (pg.darker) s = -s;
            if (s > bv) { bv = s; bi = c; }
        }
        const int m = wave_reduce_bits(bv, [](int a, int c) { return a > c ? a : c; });
        const int mi = wave_min(bv == m ? bi : 0x7fffffff);
        if (lane == 0) { s_cv[wave] = m; s_ci[wave] = mi; }
        __syncthreads();
        if (tid == 0) {
            int wv = s_cv[0], wi = s_ci[0];
            for (int w = 1; w < NW; ++w)
                if (s_cv[w] > wv || (s_cv[w] == wv && s_ci[w] < wi)) { wv = s_cv[w]; wi = s_ci[w]; }
            s_cellbest = wi;
        }
        __syncthreads();
    }
    int V = 0;
    for (int w = 0; w < NW; ++w) V = max(V, s_v[w]);
    const int cy = s_cellbest / ncx, cx = s_cellbest - cy * ncx;
    // the cell's centre is tile pixel (8cy + 4, 8cx + 4) = the centre input of output (8cy + 4 − l÷2, 8cx + 4 − l÷2)
    const int ny = min(PB, g.n1), nx = min(PB, g.n2);
    const int oy = min(max(CH * cy + 4 - hw - PB / 2, 0), g.n1 - ny), ox = min(max(8 * cx + 4 - hw - PB / 2, 0), g.n2 - nx);
    const int PH = ny + L - 1, PW = nx + L - 1, PP = (PB + L - 1 + 3) / 4 * 4;
    for (int e = tid; e < PH * PW; e += NT) {
        const int a = e / PW, c = e - a * PW;
        const int gi = ti0 + oy + a, gj = wj0 + ox + c;
        patch[a * PP + c] = (gi >= 0 && gi < g.fh && gj >= 0 && gj < g.fw) ? frame[(long long)gi * g.row_stride + gj] : (uint8_t)g.fill;
    }
    __syncthreads();
    // row pass in the strips' order: pairs k ascending, centre last
    const float fdc = (float)dc;
    for (int task = tid; task < PH * nx; task += NT) {
        const int a = task / nx, xo = task - a * nx;
        const uint8_t *p = patch + a * PP + xo;
        f2 acc = f2{0.f, 0.f};
        for (int k = 0; k < H; ++k) acc = fma_bcast(((float)p[k] - fdc) + ((float)p[L - 1 - k] - fdc), trow[k], acc);
        acc = fma_bcast((float)p[H] - fdc, trow[H], acc);
        R[a * PB + xo] = acc;
    }
    __syncthreads();
    if (wave == 0) {
        // column pass in the strips' order: taps ascending, the g₊ term then the g₋ term into one f32
        const int yo = lane & (PB - 1), xo = lane / PB;
        const bool ok = yo < ny && xo < nx;
        const f2 *rp = R + (ok ? yo * PB + xo : 0);
        float acc = 0.f;
        for (int t = 0; t < L; ++t) {
            const f2 r = rp[t * PB];
            const f2 w = tcol[t];
            acc = __builtin_fmaf(r.x, w.x, acc);
            acc = __builtin_fmaf(r.y, w.y, acc);
        }
        const float Lv = wave_max(ok ? acc : -__builtin_huge_valf());
        if (lane == 0) {
            // excluded iff ‖K‖₂·sqrt(ΣE)/255 + δ(V) < L − δ(V) − T_max  ⇔  ΣE < ((L − 2δ(V) − T_max)·255/‖K‖₂)²; the threshold a
            // hair low, for the double arithmetic of this line
            const double dV = 0.5 * (double)g.ex.T * ((double)V * (1.0 / 255.0)) * 1.00001;
            const double thr = (double)Lv - 2.0 * dV - (double)pg.tmax;
            const double q = thr * pg.kinv;
            s_emax = (thr > 0.0 && pg.tmax < __builtin_huge_valf()) ? q * q * (1.0 - 0x1p-30) : -1.0; // −1: nothing can be excluded
        }
    }
    __syncthreads();

    // ---- per slot: the hull of the blocks that cannot be excluded ----
    const int nblk = (g.n1 + CH - 1) / CH, NS = prune_span(L);
    for (int sl = tid; sl < g.nslots; sl += NT) {
        const unsigned *Es = E + sl * nsub;
        unsigned long long sum = 0;
        for (int sc = 0; sc < min(NS, nsub); ++sc) sum += Es[sc];
        int ba = -1, bb = 0;
        for (int j = 0; j < nblk; ++j) {
            if ((double)sum >= s_emax) { if (ba < 0) ba = j; bb = j + 1; }
            sum -= Es[j];
            if (j + NS < nsub) sum += Es[j + NS];
        }
        if (ba < 0) ba = bb = 0;
        g.part_mask[(long long)b * g.nslots + sl] = (unsigned long long)(unsigned)ba | ((unsigned long long)(unsigned)bb << 32);
        atomicAdd(&s_kept, prune_sc_hi(ba, bb, L, nsub) - ba);
    }
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_fetch_add(pg.stat, (unsigned long long)s_kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(pg.stat + 1, (unsigned long long)(g.nslots * nsub), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the last workgroup of the batch publishes both counts where the host sees them without a copy or a wait (the way
        // dog_finish_kernel publishes its flagged count): one plain store per batch
        const unsigned long long arrived = __hip_atomic_fetch_add(pg.stat + 2, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == (unsigned long long)gridDim.x - 1) {
            __hip_atomic_store(pg.stat + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long k = __hip_atomic_load(pg.stat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), tt = __hip_atomic_load(pg.stat + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(pg.host, (k & 0xffffffffull) | (tt << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
#endif // PDOG_ROLL_INST_ONLY

} // namespace pdog
