// dog_blob.hpp — the kernel of the blob rule (include/pawsome_blob.h states it): the shape rule's measurement over the
// connected component of the mask under the position.  pawsome_blob.hip includes this file, and pawsome_split.hip for the split
// instances (below).
//
// blob_kernel<TIER>: ONE workgroup of 256 threads per position, as shape_kernel.
//   1 - 4. The tile, the histogram, the median b and the contrast c are dog_shape.hpp's own functions (one copy).
//   5.  The mask as a BITMAP in LDS, one bit per pixel of the bounding box: the four waves walk the box as shape_kernel's loops
//       do and a wave ballot turns 64 items into a word; row r is `nws` u64 (1, 2 or 4: the box is 2^colbits columns wide).
//       n_mask is the popcount of the ballots.
//   5a. The seed from the staged 3 x 3.
//   5b. The fill, sweeps of pdog_blob_fill.hpp's row operations until one adds no bit:
//         TIER 1, R <= 31 (a row is one u64): lane r of wave 0 owns row r; the neighbour rows come from lane shuffles and the
//           vote is a wave ballot — no barrier and no LDS access inside the loop; waves 1 - 3 wait at the barrier behind it.
//         TIER 2, R = 32 ... 127: thread r owns row r with M_r and F_r as four u64 in registers, publishes F_r in LDS (over the
//           mask bitmap, which every thread has read by then) and reads the rows r - 1 and r + 1 after a barrier; the vote is a
//           flag in LDS: two barriers per sweep.  Three flags take turns so that clearing the next one never meets a read.
//       The exit condition is a wave vote (tier 1) or an LDS word read behind a barrier (tier 2): uniform where it is tested.
//       Every sweep but the last adds a pixel, so the loop ends after at most (blob pixels) + 1 sweeps; it waits for no other
//       workgroup, and nothing atomic touches global memory.
//   6.  The six sums and n_rim over the blob's bitmap, reduced as shape_kernel reduces its sums; ten ordinary vector stores;
//       shape::derive by one lane where the floats are asked for.
//
// blob_kernel<TIER, SplitGeo>: the SPLIT rule (include/pawsome_split.h) as instances of the same kernel — every step above is the
// one copy; what follows is compiled into them alone (`if constexpr (Geo::split)`), and blob_kernel<TIER, BlobGeo> is what it was.
//   0.  A workgroup is one position (s, a) of a set; its element `pos` is the block index in either accepted layout.  Every wave
//       reads the set's other positions, one per lane (at most 31), clamps them and keeps those with |p - q|^2 <= (2R)^2: a
//       ballot compacts the kept ones into LDS as (ei, ej, wins) and its popcount is the rival count — the same in every wave,
//       since all four vote on the same data.
//   5c. The row's owner (lane r, thread r) cuts the row's column interval by every rival (pdog_split_cell.hpp: O(rivals) per
//       row) and splits its mask row in registers into M & cell, which the fill then runs on, and M & ~cell, the rival side.
//       n_cell is the popcount of the first.
//   6'. n_contact = popcount of F & (the rival side shifted left and right | the rival-side rows above and below): tier 1 by
//       lane shuffles, tier 2 through a second bitmap of D * nws u64 in LDS (the cross-word bits handed over).  That bitmap lies
//       OVER THE TILE, whose last reader (the mask and the seed) is a barrier behind by then: beside the first bitmap it would
//       make R = 127 need 82 112 bytes, and two workgroups would no longer share a CU's 160 KiB (split_lds_bytes below).
//   The fill loop is untouched, the only new loop runs over the <= 31 rivals, and twelve ordinary vector stores go out.
#pragma once
#define PDOG_SHAPE_STEPS_ONLY
#include "dog_shape.hpp"
#include "pdog_blob_fill.hpp"
#include "pdog_split_cell.hpp"

namespace pdog {

struct BlobGeo {
    ShapeGeo s;        // out_sums: null or [n][10]
    int eight;         // connectivity 8 (else 4)
    uint32_t *sweeps;  // null, or [n]: the sweeps every position took (the ablation build's counter; null otherwise)
    static constexpr bool split = false;
};

// the split rule's geometry: s.n = n_sets * n_targets positions, element s * n_targets + a (set-major) or a * n_sets + s
struct SplitGeo {
    ShapeGeo s;        // out_sums: null or [n][12]
    int eight;
    uint32_t *sweeps;
    int n_sets, n_targets;
    int target_major;  // strides (1, n_sets) (else (n_targets, 1))
    static constexpr bool split = true;
};

constexpr int kSplitMaxTargets = 32;

// u64 words of a bitmap row, and dynamic LDS bytes of the kernel: the tile (an even number of dwords) and the bitmap
__host__ __device__ constexpr int blob_row_words(int colbits) { return colbits <= 6 ? 1 : 1 << (colbits - 6); }
__host__ __device__ constexpr int blob_tile_words(int R) { return (shape_tile_words(R) + 1) & ~1; }
__host__ __device__ constexpr size_t blob_lds_bytes(int R, int colbits)
{
    return sizeof(uint32_t) * (size_t)blob_tile_words(R) + sizeof(uint64_t) * (size_t)(2 * R + 1) * blob_row_words(colbits);
}
// the split instances: behind the bitmap the rival list, 32 x (ei, ej, wins, -).  Tier 2's rival-side bitmap takes the tile's
// place (D * nws * 8 <= D * D bytes from D = 65 on), so R = 127 stays at 73 952 bytes: two workgroups per CU, as blob_kernel<2>.
__host__ __device__ constexpr size_t split_lds_bytes(int R, int colbits)
{
    return blob_lds_bytes(R, colbits) + sizeof(int) * 4 * kSplitMaxTargets;
}

// 5c. the row's cell as an interval of bitmap columns c0 ... c1 (empty: c0 > c1)
__device__ __forceinline__ void split_row_interval(const int *rivals, int nr, int r, int R, int &c0, int &c1)
{
    int lo = -R, hi = R;
    for (int k = 0; k < nr; ++k) splitcell::cut_row(lo, hi, r - R, rivals[4 * k], rivals[4 * k + 1], rivals[4 * k + 2] != 0);
    c0 = lo + R;
    c1 = hi + R;
}

template <int TIER, class Geo = BlobGeo>
static __global__ __launch_bounds__(kShapeThreads) void blob_kernel(const Geo bg)
{
    constexpr bool SPLIT = Geo::split;
    constexpr int NRED = SPLIT ? 10 : 8, NOUT = SPLIT ? 12 : 10;
    __shared__ __attribute__((aligned(16))) uint32_t hist[256];
    __shared__ int red[kShapeWaves][NRED];
    __shared__ int chg[3];
    extern __shared__ __attribute__((aligned(16))) uint32_t tile[]; // D rows of W dwords, then D rows of nws u64
    const ShapeGeo &g = bg.s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long pos = blockIdx.x;
    const int R = g.R, D = 2 * R + 1, W = (D + 3) >> 2, P = 4 * W;
    const int i = min(max(g.ij[2 * pos], 1), g.fh), j = min(max(g.ij[2 * pos + 1], 1), g.fw);
    long long fidx = g.frame_index ? (long long)g.frame_index[pos] : pos;
    const int nws = TIER == 1 ? 1 : blob_row_words(g.colbits);
    uint64_t *bits = (uint64_t *)(tile + blob_tile_words(R));
    // 0. (split) the set's rivals, compacted: every wave votes on the same data, wave 0 writes the list
    [[maybe_unused]] int nr = 0;
    [[maybe_unused]] uint64_t *rbits = nullptr;    // tier 2: the rival-side bitmap, over the tile once the mask and the seed are read
    [[maybe_unused]] int *rivals = nullptr;
    if constexpr (SPLIT) {
        rbits = (uint64_t *)tile;
        rivals = (int *)(bits + D * nws);
        const int T = bg.n_targets, S = bg.n_sets;
        const int set = bg.target_major ? (int)(pos % S) : (int)(pos / T), a = bg.target_major ? (int)(pos / S) : (int)(pos % T);
        if (!g.frame_index) fidx = set;
        bool keep = false;
        int ei = 0, ej = 0;
        if (lane < T && lane != a) {
            const long long el = bg.target_major ? (long long)lane * S + set : (long long)set * T + lane;
            ei = min(max(g.ij[2 * el], 1), g.fh) - i;
            ej = min(max(g.ij[2 * el + 1], 1), g.fw) - j;
            keep = (long long)ei * ei + (long long)ej * ej <= 4ll * R * R;
        }
        const uint64_t bal = __ballot(keep);
        nr = __popcll(bal);
        if (keep && wave == 0) {
            const int at = __popcll(bal & ((1ull << lane) - 1ull));
            rivals[4 * at] = ei;
            rivals[4 * at + 1] = ej;
            rivals[4 * at + 2] = a < lane;
            rivals[4 * at + 3] = 0;
        }
    }
    const uint8_t *__restrict__ frame = g.frames + fidx * g.frame_stride;
    const int i0 = i - 1 - R, j0 = j - 1 - R;
    const uint32_t fill = (uint32_t)g.fill & 0xffu;
    const bool eight = bg.eight != 0;

    hist[tid] = 0;
    shape_stage_tile(g, frame, i0, j0, fill, tile, tid, D, W);
    __syncthreads();
    const uint8_t *px = (const uint8_t *)tile;
    const int cmask = (1 << g.colbits) - 1, items = D << g.colbits, R2 = R * R;
    shape_histogram(g, px, hist, tid, R, D, P, cmask, items, R2);
    __syncthreads();
    const int b = shape_median(hist, lane, g.rank);
    const int c = shape_contrast(px, R, P, b, g.darker);

    // 5. the mask's bitmap: a wave's 64 items are 64 columns of one row (colbits >= 6) or whole rows of 2^colbits columns
    int n_mask = 0;
    {
        const bool have = c >= g.min_contrast;
        const int padded = (items + 63) & ~63;
        for (int base = wave * 64; base < padded; base += kShapeThreads) {   // wave-uniform bounds: every lane votes
            const int e = base + lane, r = e >> g.colbits, cc = e & cmask;
            const int dy = r - R, dx = cc - R;
            bool in = have && e < items && cc < D && dy * dy + dx * dx <= R2;
            if (in) {
                const int p = px[r * P + cc];
                const int s = g.darker ? b - p : p - b;
                in = 2 * s >= c;
            }
            const uint64_t bal = __ballot(in);
            if (g.colbits >= 6) {             // items is a multiple of 64 then: lane 0's row r < D, and cc >> 6 < nws
                if (lane == 0) bits[r * nws + (cc >> 6)] = bal;
            } else if (cc == 0 && e < items) {
                bits[r] = (bal >> lane) & ((1ull << (1 << g.colbits)) - 1ull);
            }
            if (lane == 0) n_mask += __popcll(bal);
        }
    }
    // 5a. the seed: the first pixel of the 3 x 3, row-major, at the contrast c
    int seed_r = R, seed_c = R;
    {
        bool found = false;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int p = px[(R + dy) * P + R + dx];
                const int s = g.darker ? b - p : p - b;
                if (!found && s == c) {
                    found = true;
                    seed_r = R + dy;
                    seed_c = R + dx;
                }
            }
    }
    if (TIER == 2 && tid < 3) chg[tid] = 0;
    __syncthreads();
    // 5b. the fill.  The seed is taken through the mask: an empty mask (c < min_contrast) leaves the blob empty.
    uint32_t sweeps = 0;
    [[maybe_unused]] int n_cell = 0, n_contact = 0;
    if (TIER == 1) {
        if (wave == 0) {
            uint64_t M = lane < D ? bits[lane] : 0;
            [[maybe_unused]] uint64_t V = 0;           // (split) the rival side of the row: M & ~cell
            if constexpr (SPLIT) {
                int c0, c1;
                split_row_interval(rivals, nr, lane, R, c0, c1);
                const uint64_t cell = splitcell::span_word(c0, c1, 0);
                V = M & ~cell;
                M &= cell;
                n_cell = __popcll(M);
            }
            uint64_t F = lane == seed_r ? (1ull << seed_c) & M : 0;
            for (;;) {
                uint64_t up = __shfl_up(F, 1, 64), dn = __shfl_down(F, 1, 64);
                if (lane == 0) up = 0;
                if (lane == 63) dn = 0;
                const uint64_t nf = blobfill::sweep_row1(M, F, up, dn, eight);
                const bool more = __any(nf != F);     // a wave vote: the same for every lane
                F = nf;
                ++sweeps;
                if (!more) break;
            }
            if (lane < D) bits[lane] = F;
            if constexpr (SPLIT) {
                uint64_t vu = __shfl_up(V, 1, 64), vd = __shfl_down(V, 1, 64);
                if (lane == 0) vu = 0;
                if (lane == 63) vd = 0;
                n_contact = __popcll(F & ((V << 1) | (V >> 1) | vu | vd));
            }
        }
        __syncthreads();
    } else {
        const bool act = tid < D;
        blobfill::Row4 M, F;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            M.w[k] = act && k < nws ? bits[tid * nws + k] : 0;
            F.w[k] = 0;
        }
        [[maybe_unused]] blobfill::Row4 V;                 // (split) the rival side of the row, published for the rows next to it
        if constexpr (SPLIT) {
            int c0 = 0, c1 = -1;
            if (act) split_row_interval(rivals, nr, tid, R, c0, c1);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t cell = splitcell::span_word(c0, c1, k);
                V.w[k] = M.w[k] & ~cell;
                M.w[k] &= cell;
                n_cell += __popcll(M.w[k]);
                if (act && k < nws) rbits[tid * nws + k] = V.w[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) F.w[k] = tid == seed_r && k == (seed_c >> 6) ? (1ull << (seed_c & 63)) & M.w[k] : 0;
        __syncthreads();                               // the bitmap is read: F goes over it
        int cur = 0;
        for (;;) {
            const int nxt = cur == 2 ? 0 : cur + 1;
            if (act) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nws) bits[tid * nws + k] = F.w[k];
            }
            if (tid == 0) chg[nxt] = 0;                // last read two barriers ago
            __syncthreads();
            if (act) {
                blobfill::Row4 up, dn;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    up.w[k] = tid > 0 && k < nws ? bits[(tid - 1) * nws + k] : 0;
                    dn.w[k] = tid + 1 < D && k < nws ? bits[(tid + 1) * nws + k] : 0;
                }
                const blobfill::Row4 nf = blobfill::sweep_row4(M, F, up, dn, eight);
                if (blobfill::differ4(nf, F)) chg[cur] = 1;
                F = nf;
            }
            __syncthreads();
            ++sweeps;
            if (!chg[cur]) break;                      // one LDS word behind a barrier: the same for every thread
            cur = nxt;
        }
        // the last sweep changed nothing: the published rows are the blob
        if constexpr (SPLIT) {
            if (act) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint64_t v = (V.w[k] << 1) | (k > 0 ? V.w[k - 1] >> 63 : 0);
                    v |= (V.w[k] >> 1) | (k < 3 ? V.w[k + 1] << 63 : 0);
                    if (tid > 0 && k < nws) v |= rbits[(tid - 1) * nws + k];
                    if (tid + 1 < D && k < nws) v |= rbits[(tid + 1) * nws + k];
                    n_contact += __popcll(F.w[k] & v);
                }
            }
        }
    }
    // 6. the sums over the blob, and the blob pixels with an edge neighbour outside the disc
    int n = 0, sy = 0, sx = 0, syy = 0, syx = 0, sxx = 0, n_rim = 0;
    for (int e = tid; e < items; e += kShapeThreads) {
        const int r = e >> g.colbits, cc = e & cmask;
        if (cc < D && ((bits[r * nws + (cc >> 6)] >> (cc & 63)) & 1ull)) {
            const int dy = r - R, dx = cc - R;
            const int ay = abs(dy) + 1, ax = abs(dx) + 1;
            n += 1;
            sy += dy;
            sx += dx;
            syy += dy * dy;
            syx += dy * dx;
            sxx += dx * dx;
            n_rim += (ay * ay + dx * dx > R2) || (dy * dy + ax * ax > R2);
        }
    }
    n = shape_wave_sum(n);
    sy = shape_wave_sum(sy);
    sx = shape_wave_sum(sx);
    syy = shape_wave_sum(syy);
    syx = shape_wave_sum(syx);
    sxx = shape_wave_sum(sxx);
    n_rim = shape_wave_sum(n_rim);
    if (lane == 0) {
        red[wave][0] = n;
        red[wave][1] = sy;
        red[wave][2] = sx;
        red[wave][3] = syy;
        red[wave][4] = syx;
        red[wave][5] = sxx;
        red[wave][6] = n_mask;
        red[wave][7] = n_rim;
    }
    if constexpr (SPLIT) {
        n_cell = shape_wave_sum(n_cell);
        n_contact = shape_wave_sum(n_contact);
        if (lane == 0) {
            red[wave][8] = n_cell;
            red[wave][9] = n_contact;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int32_t s[NOUT];
#pragma unroll
        for (int k = 0; k < NRED; ++k) {
            int v = 0;
#pragma unroll
            for (int w = 0; w < kShapeWaves; ++w) v += red[w][k];
            s[k < 6 ? k : k + 2] = v;
        }
        s[6] = b;
        s[7] = c;
        if (g.out_sums) {
#pragma unroll
            for (int k = 0; k < NOUT; ++k) g.out_sums[NOUT * pos + k] = s[k];
        }
        if (g.out_shape) {
            double o[6];
            shape::derive(s, i, j, o);
#pragma unroll
            for (int k = 0; k < 6; ++k) g.out_shape[6 * pos + k] = o[k];
        }
        if (bg.sweeps) bg.sweeps[pos] = sweeps;
    }
}

} // namespace pdog
