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
// THE CELL BOUND, a second stage inside the first stage's hull.  One inequality per block against everything the block reads
// is loose: a block that sees a disc only through the kernel's outermost rows stays, and so does a neighbouring strip that sees
// it through its outermost columns.  Cut the tile into 8 × 8 cells, as the energy pass does.  Output cell (yb, xb) is window rows
// 8yb … 8yb + 7, columns 8xb … 8xb + 7; its output (y, x) = (8yb + i, 8xb + j) reads tile rows y … y + l − 1, that is the input
// cells (yb + dy, xb + dx), dy, dx < NS = prune_span(l), and lays on cell (dy, dx) exactly the kernel rows
// rows(i, dy) = [8dy − i, 8dy − i + 8) ∩ [0, l) and the like columns: the NS² boxes tile K.  Cauchy–Schwarz per input cell gives
//     255·|f(y, x)| ≤ Σ_{dy,dx} ‖K[rows(i, dy), cols(j, dx)]‖₂ · sqrt(Ec[yb + dy][xb + dx])
//                  ≤ Σ_{dy,dx} W[dy][dx] · sqrt(Ec[yb + dy][xb + dx]) =: B(yb, xb),
// Ec = Σ v² over the input cell (fill and DC level as in the energies, zero outside the tile) and W[dy][dx] the largest of the
// 64 partial norms.  An output cell is excluded iff B < 255·(L − 2δ(V) − T_max): the first stage's own threshold, only the left
// side is new.  A block of a slot stays iff the first stage keeps it AND an output cell that meets the slot's columns (a strip at
// c0 of w columns: cells c0 >> 3 … (c0 + w − 1) >> 3, nine where the strip is shifted off the grid; a remainder column: its one
// cell) is not excluded; the refined range is the contiguous hull of those blocks, a sub-range of the first stage's, maybe empty.
// WHY NOTHING CHANGES: an excluded pixel q lies in an excluded cell or outside the first stage's hull; either way
// |f(q)| ≤ bound/255 < L − 2δ(V) − T_max, the inequality the argument above starts from, which then carries over word for word.
// The cell that holds L's best pixel p has B ≥ 255·|f(p)| ≥ 255·(L − δ(V)) and is never excluded: L ≤ M stands, and no window's
// refined ranges are all empty while its first-stage ranges are not.
// ARITHMETIC: exact and the same on every machine, every rounding towards keeping.  r = ⌈16·√Ec⌉ as an integer (pw_root16: the
// f32 estimate corrected by integer comparisons), 16 bits per cell in LDS; Wq = ⌈2¹²·W/‖K‖₂⌉ from the host (pdog_math.cpp,
// dog_refine_weights); Σ Wq·r in 64-bit integers, any order; the threshold ⌊2¹⁶·q·(1 − 2⁻³⁰)⌋ with the first stage's
// q = (L − 2δ(V) − T_max)·255/‖K‖₂ (B·‖K‖₂ ≤ Σ Wq·r·‖K‖₂/2¹⁶).  tests/prune_refine_restatement.py states it in NumPy and the
// kernel's job list equals it entry for entry.  Nothing to do where the first stage excludes nothing (thr ≤ 0, an infinite T_max).
// The first stage, its counts (stat[0] / stat[1], the packed word's `kept`, the host word) and the policy are as before: the
// refined range goes into the range words, the job list and the empty strips' Peak.  Where the roots would push the dynamic LDS
// past the host's limit, or NS > PRUNE_REFINE_MAX_SPAN, the launch passes wq = null and the first stage stands alone.
//
// WHERE IT STOPS PAYING: where the background's energy under the kernel reaches the target's response (heavy noise or
// texture, noise-only and flat windows: nothing is excluded and the pre-pass is paid for nothing).  launch_strips reads the
// kept / total counts this kernel publishes and stops running it on such batches (pawsome_dog.hip, "pruning policy").
//
// The ranges travel in LaunchGeo::part_mask: slot [b][s] holds (first block | one past the last block << 32) when the roll /
// thin kernels start (LaunchGeo::prune) and the strip's column mask, as ever, when they end.  A remainder column's word also
// carries the window's DC level (bits 24 … 31): dog_thin_kernel reads its range there and skips the DC samples.
//
// THE JOB LIST.  A launch of one wave per (window, strip) interleaves the kept strips, all of nearly one length, with as many
// waves that find an empty range and return at once, and the SIMDs stood empty for 45 % of the roll kernel (1.66 resident
// waves per SIMD where the dense kernel holds 2.8).  So the pre-pass appends every window's kept STRIPS to a list
// the tracker owns (PruneJob: window, strip, range, DC level; entry 0 is the header with the batch's count), a window's
// entries next to each other, and writes itself what the returning wave wrote: the initialised Peak of a strip with an empty
// hull (its range word, 0, is already its column mask).  The PRUNE instance of dog_roll_kernel takes entry
// prune_job_index(blockIdx.x) and needs neither the range word nor the DC samples.  No memset, no extra launch, no waiting
// on the device: one returning atomic per workgroup (the one that counted arrivals before) hands out the list positions, and
// the last workgroup to arrive publishes the count.  The list's order differs from run to run; results go to [b][s].
#pragma once
#include "dog_roll.hpp"
#include "dog_prune_words.hpp"
#include "dog_prune_publish.hpp"

namespace pdog {

struct PruneGeo {
    LaunchGeo g;              // frames, guesses, geometry, nstrips / nthin / thin_x0 / nslots, ex.T, part_mask (receives the ranges)
    double kinv;              // 255 / ‖K‖₂ with ‖K‖₂ rounded up
    float tmax;               // T_max (header comment)
    int darker;               // sign of the cell sums that point at a target
    unsigned long long *stat; // [0] kept, [1] total (slot, sub-chunk) pairs since the tracker was created, [2] of the batch in flight: arrivals, jobs appended, pairs kept (dog_prune_publish.hpp; PRUNE_FENCED_PUBLISH: arrivals | jobs appended << 32)
    uint64_t *host;           // Mailbox::prune_pub, one host-coherent word: the low half of [0] and ([1] << 32) as the last workgroup of a batch left them
    PruneJob *jobs;           // the job list: the header, then room for n · nstrips entries
    const uint32_t *wq;       // the second stage's weights (pdog_math.cpp, dog_refine_weights) as [NS][prune_refine_pitch(NS)], zeros behind each row, four more at the end; null: the first stage alone
};

constexpr int PRUNE_NT = 256;
constexpr int PRUNE_B = 8; // the L pixels: PRUNE_B × PRUNE_B outputs
constexpr int PRUNE_PHASES = 9; // phase stamps of the diagnostic build: stat[4 … 4 + PRUNE_PHASES), then the workgroups that stamped
// The segment sums (S) are dead once the energies are formed and the L block's buffers (R, patch) live only after that: they
// share one region.  The patch carries 8 bytes of slack: its row pass reads whole dwords, up to 3 bytes past a row's last pixel.
// The second stage adds the cells' roots (16 bits each, a zero row and a zero column behind them: an output cell reads at most one
// cell past the tile either way; what a zero weight of the padded table meets beyond that is never counted) and the refined hulls.
constexpr int PRUNE_REFINE_MAX_SPAN = 32; // a row of NS products Wq·r ≤ 4097·32640 stays below 2³² up to here (l ≤ 249)
__host__ __device__ inline int prune_refine_pitch(int NS) { return (NS + 3) / 4 * 4; } // a row of the weight table: whole groups of four
struct PruneLds { size_t cell, E, segd, strd, S, R, patch, root, hull2, total; };
__host__ __device__ inline PruneLds prune_lds(int n1, int n2, int L, int nslots, bool refine = false)
{
    const size_t NA = n1 + L - 1, nsub = (NA + ROLL_CH - 1) / ROLL_CH, ncx = (size_t)(n2 + L - 1 + 7) / 8;
    const size_t PH = PRUNE_B + L - 1, PP = (PH + 3) / 4 * 4, nseg = 2 * (size_t)nslots + 1;
    PruneLds o;
    o.cell = 0;
    o.E = o.cell + nsub * ncx * 4;
    o.segd = o.E + (size_t)nslots * nsub * 4;
    o.strd = o.segd + (2 * ncx * 2 + 3) / 4 * 4;
    o.S = (o.strd + 2 * (size_t)nslots * 2 + 7) / 8 * 8;
    o.R = o.S;
    o.patch = o.R + PH * PRUNE_B * sizeof(f2);
    const size_t endS = o.S + nsub * nseg * 8, endL = o.patch + PH * PP + 8;
    o.total = ((endS > endL ? endS : endL) + 15) / 16 * 16;
    o.root = o.hull2 = o.total;
    if (refine) {
        o.hull2 = o.root + ((nsub + 1) * (ncx + 1) * 2 + 8 + 3) / 4 * 4; // (8: the last group of a row reads up to three roots past the row's end)
        o.total = (o.hull2 + (size_t)nslots * 8 + 15) / 16 * 16;
    }
    return o;
}

#ifndef PDOG_ROLL_INST_ONLY
// One workgroup per window.
//
// HOW THE ENERGIES ARE FORMED (dog_prune_words.hpp has the arithmetic).  The slots' column ranges [c0, c1) cut the tile's columns
// into a handful of segments (cfg3: cuts at 0, 64, 128, 192, 256, 320, 321); column c lies in segment seg_id(c) = the number
// of cuts ≤ c.  The energy pass keeps the raw-pixel moments (Σ p², Σ p) per (band, segment), E[slot][band] is formed once at
// the end from the slot's segments, and the cell sums are Σ p − n·dc of two neighbouring dwords.
//   * One item = one 8 × 8-pixel cell: the 8 rows of a band × two dwords of columns, one 8-byte load per row.  The cells of
//     the whole tile are dealt out to the threads in order (consecutive lanes read consecutive cells of a row: coalesced;
//     94 % of the lanes busy at cfg3, where a lane per dword of ONE row left 17 of 64 busy in its second pass);
//     (band, cell) advance by the constant (NT ÷ ncx, NT mod ncx): no division in the loop.  A first version dealt out
//     single dwords and paired them by DPP: its per-item index, mask and segment work outweighed the 11 instructions per
//     dword of the sums themselves (1.81e4 VALU instructions per window); per cell that work is paid once per 16.
//   * How partial sums meet: the lane STORES its cell's sum (every cell has exactly one item: no atomic, no zeroing) and adds
//     the cell's moments to its (band, segment) with two LDS atomics — per wave-instruction 64 lanes on about nine
//     addresses.  A wave reduction per segment would need the lanes aligned to the cuts, which the in-order deal does not
//     give (a band is 41 cells), and a band per wave leaves the lanes idle as above; a cell whose dwords lie in different
//     segments adds per dword.
//   * A dword that straddles a cut (strips shifted to ncols − 64, remainder columns) adds nothing to the segments in the main
//     pass; the few such dwords are listed and a second, byte-masked pass adds them column by column.
// (Tried: 80 SGPRs at most, for eight resident workgroups per CU instead of six at 106: 35 SGPR spills, the kernel no faster.)
// REGISTERS.  The next cell's loads in flight cost sixteen VGPRs: 79, six waves per SIMD by the compiler's count.  (Tried:
// amdgpu_waves_per_eu(7) — 72 VGPRs, five spilled, scratch loads in the cell loop: slower in every run,
// profiles/prepass_latency_ab.txt.  A second cell in flight would be sixteen more.)  With the wave that files the job list at
// the kernel's end the allocator took 82, five waves per SIMD: amdgpu_waves_per_eu(6) holds it to 79 with nothing spilled
// (profiles/compact_kernel_regs.txt).  With the second stage: 80, still six waves and nothing in scratch; fifteen of its scalars
// pass through VGPR lanes (profiles/refine_kernel_regs.txt).
// NARROW: the instance for frames narrower than one clamped load (below), which keeps the byte path; every other frame runs
// the instance without it.
template <bool NARROW>
static __global__ __launch_bounds__(PRUNE_NT) __attribute__((amdgpu_waves_per_eu(6))) void dog_prune_kernel(const PruneGeo pg, const f2 *__restrict__ taps_row, const f2 *__restrict__ taps_col)
{
    constexpr int NT = PRUNE_NT, NW = NT / 64, CH = ROLL_CH, TW = ROLL_TW, PB = PRUNE_B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LaunchGeo &g = pg.g;
    const int L = g.L, hw = L / 2, H = L / 2;
    const int NA = g.n1 + L - 1, TWin = g.n2 + L - 1, nsub = (NA + CH - 1) / CH, ncx = (TWin + 7) / 8, TQ2 = 2 * ncx;
    const int nseg = 2 * g.nslots + 1;
    const bool refine = pg.wq != nullptr; // (workgroup-uniform: a kernel argument)
    const PruneLds lo = prune_lds(g.n1, g.n2, L, g.nslots, refine);
    int *cell = reinterpret_cast<int *>(smem + lo.cell);           // [nsub][ncx] Σ v over 8 × 8-pixel cells of the tile
    unsigned *E = reinterpret_cast<unsigned *>(smem + lo.E);       // [nslots][nsub]
    short *segd = reinterpret_cast<short *>(smem + lo.segd);       // [2ncx] a dword's segment; −1: it straddles a cut or lies past the tile
    unsigned short *strd = reinterpret_cast<unsigned short *>(smem + lo.strd); // the dwords that straddle a cut (at most one per cut)
    unsigned *S = reinterpret_cast<unsigned *>(smem + lo.S);       // [nsub][nseg] (Σ p², Σ p)
    f2 *R = reinterpret_cast<f2 *>(smem + lo.R);                   // [PB + l − 1][PB] row-pass outputs of the L pixels
    uint8_t *patch = smem + lo.patch;                              // their input pixels
    unsigned short *root = reinterpret_cast<unsigned short *>(smem + lo.root); // [nsub + 1][ncx + 1] ⌈16·√Ec⌉ of the cells (second stage)
    const int rp = ncx + 1;
    __shared__ int s_sum[NW], s_pmax[NW], s_pmin[NW], s_cv[NW], s_ci[NW], s_cellbest, s_nstr;
    __shared__ double s_emax;
    __shared__ long long s_tq;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int g1 = g.guesses[2 * b], g2 = g.guesses[2 * b + 1];
    const int fidx = g.frame_index ? g.frame_index[b] : b;
    const uint8_t *__restrict__ frame = g.frames + (long long)fidx * g.frame_stride;
    const int ti0 = g1 - g.r1 - 1 - hw, wj0 = g2 - g.r2 - 1 - hw; // frame row / column of the tile's first pixel
    const tap_ptr trow = as_taps(taps_row), tcol = as_taps(taps_col);
    const uint32_t fill4 = (uint32_t)g.fill * 0x01010101u;
#ifdef PDOG_ABLATIONS
    // Phase stamps (diagnostic build; tools/prune_phases.py): thread 0 of every workgroup adds the cycles since its last stamp
    // to stat[4 + phase] with an ordinary atomic, and counts itself in stat[4 + PRUNE_PHASES].
    unsigned long long stamp_prev = __builtin_readcyclecounter();
#define PRUNE_STAMP(i) do { if (tid == 0) { const unsigned long long now_ = __builtin_readcyclecounter(); atomicAdd(pg.stat + 4 + (i), now_ - stamp_prev); stamp_prev = now_; } } while (0)
#else
#define PRUNE_STAMP(i) do { } while (0)
#endif

    const int ncols = g.nthin ? g.thin_x0 : g.n2; // window columns the strips cover
    const int ws = min(TW, ncols);
    auto slot_cols = [&](int sl, int &c0, int &c1) { // the tile columns a slot's outputs read
        const bool strip = sl < g.nstrips;
        c0 = strip ? ((ncols >= TW) ? min(sl * TW, ncols - TW) : 0) : g.thin_x0 + (sl - g.nstrips);
        c1 = c0 + (strip ? ws + L - 1 : L);
    };
    auto seg_id = [&](int c) {
        int id = 0;
        for (int sl = 0; sl < g.nslots; ++sl) {
            int c0, c1;
            slot_cols(sl, c0, c1);
            id += (c0 <= c) + (c1 <= c);
        }
        return id;
    };
    // HOW THE FRAME IS READ.  Every address read lies in a row of the frame at a column of the frame, and no load stands behind
    // a branch that another load decides: a word of the tile is loaded at its row and start column CLAMPED into the frame, all
    // loads of an item are requested together, and the tile's word is rebuilt afterwards by a shift of the clamp distance
    // (dog_prune_words.hpp, "clamped loads"); the in-frame masks select the fill as before.  (Before: a cell on the frame's
    // edge read row by row, dword by dword and, over the left or right edge, byte by byte, each load behind its own wait —
    // 16 to 64 memory round trips where an interior cell takes one, and one such lane holds its whole wave.)  A frame
    // narrower than one load (fw < 8 for the cells, < 4 for single dwords) keeps the byte path, tile_word: that case is cold.
    auto row_in = [&](int gi) { return gi >= 0 && gi < g.fh; };
    const bool narrow8 = NARROW && g.fw < 8, narrow4 = NARROW && g.fw < 4;
    const unsigned rs = (unsigned)g.row_stride; // (at most PDOG_MAX_ROW_STRIDE: an offset inside a frame is a 32 × 32-bit product)
    auto frame_at = [&](int gi, int gjc) { return frame + ((unsigned long long)(unsigned)pw_clamp_row(gi, g.fh) * rs + (unsigned)gjc); };
    // One dword of the tile at frame row gi, frame column gj, byte by byte: the bytes inside the frame (`in`: pw_mask(gj, 0, fw)
    // in a row of the frame, else 0), 0 elsewhere.
    auto tile_word = [&](int gi, int gj, uint32_t in) -> uint32_t {
        uint32_t w = 0;
        if (in == 0xffffffffu) {
            __builtin_memcpy(&w, frame + (long long)gi * g.row_stride + gj, 4);
        } else if (in) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((in >> (8 * i)) & 1u) w |= (uint32_t)frame[(long long)gi * g.row_stride + gj + i] << (8 * i);
        }
        return w;
    };

    // ---- the energy pass's items and their loads (the pass itself: below) ----
    const int nitems = nsub * ncx;
    // the cell's sixteen dwords, row r in w[2r], w[2r + 1]: as loaded at the clamped address (narrow frame: the tile's words)
    auto cell_load = [&](int band, int cx, uint32_t (&w)[2 * CH]) {
        const int gj = wj0 + 8 * cx, gi0 = ti0 + band * CH;
        if (!narrow8) {
            const uint8_t *src = frame_at(gi0, pw_clamp_col(gj, g.fw, 8));
#pragma unroll
            for (int r = 0; r < CH; ++r) { // (the clamped row moves on from row gi0 + r iff 0 ≤ gi0 + r < fh − 1)
                __builtin_memcpy(&w[2 * r], src, 8);
                src += (unsigned)(gi0 + r) < (unsigned)(g.fh - 1) ? rs : 0u;
            }
        } else {
            const uint32_t in_a = pw_mask(gj, 0, g.fw), in_b = pw_mask(gj + 4, 0, g.fw);
            for (int r = 0; r < CH; ++r) {
                const bool rin = row_in(gi0 + r);
                w[2 * r] = tile_word(gi0 + r, gj, rin ? in_a : 0u);
                w[2 * r + 1] = tile_word(gi0 + r, gj + 4, rin ? in_b : 0u);
            }
        }
    };

    if (tid == 0) s_nstr = 0;
    // ---- the window's DC level: the strips' samples (dc_sample_sum's grid) and rounding.  A thread's samples are requested
    // together at clamped addresses and the fill is selected afterwards; the first cell's loads follow them at once — a
    // cell's moments do not depend on dc — so both are in flight while the segment sums are zeroed and the samples reduced ----
    int dc;
    uint32_t cur[2 * CH];
    {
        constexpr int DCN = 1024 / NT;
        const int tH = NA, tW = TWin;
        int sv[DCN];
        bool sin[DCN];
#pragma unroll
        for (int j = 0; j < DCN; ++j) {
            const int k = tid + j * NT;
            const int gi = ti0 + (int)(((long long)(k >> 5) * tH) >> 5), gj = wj0 + (int)(((long long)(k & 31) * tW) >> 5);
            sin[j] = row_in(gi) && gj >= 0 && gj < g.fw;
            sv[j] = *frame_at(gi, min(max(gj, 0), g.fw - 1));
        }
        {
            const int it0 = min(tid, nitems - 1), band0 = it0 / ncx; // (a thread without an item loads the last one, and drops it)
            cell_load(band0, it0 - band0 * ncx, cur);
        }
        for (int i = tid; i < nsub * nseg * 2; i += NT) S[i] = 0;
        if (refine) { // the zero row and column behind the cells' roots
            for (int i = tid; i <= nsub; i += NT) root[i * rp + ncx] = 0;
            for (int i = tid; i < ncx; i += NT) root[nsub * rp + i] = 0;
        }
        int sum = 0;
#pragma unroll
        for (int j = 0; j < DCN; ++j) sum += sin[j] ? sv[j] : g.fill;
        sum = wave_sum(sum);
        if (lane == 0) s_sum[wave] = sum;
        __syncthreads();
        int tot = 0;
        for (int w = 0; w < NW; ++w) tot += s_sum[w];
        dc = __builtin_amdgcn_readfirstlane(dc_from_sum(tot, g.fill)); // (workgroup-uniform, and live to the kernel's last lines: a scalar)
    }
    for (int d = tid; d < TQ2; d += NT) {
        int sd = -1;
        if (4 * d < TWin) {
            const int first = seg_id(4 * d), last = seg_id(min(4 * d + 3, TWin - 1));
            if (first == last) sd = first;
            else strd[atomicAdd(&s_nstr, 1)] = (unsigned short)d;
        }
        segd[d] = (short)sd;
    }
    __syncthreads();
    PRUNE_STAMP(0); // DC level, segment table

    // ---- energy pass (above).  Per dword: the two substituted words, two dots, two ands, four packed min / max.  The loads
    // of the thread's next cell are requested before the sums of this one (sixteen registers each) ----
    PwAcc ext = pw_init(); // (its extremes only: the thread's pixels of all its items)
    auto cell_sums = [&](int band, int cx, const uint32_t (&w)[2 * CH]) {
        const int col0 = 8 * cx, gj = wj0 + col0, a0 = band * CH, gi0 = ti0 + a0, nr = min(CH, NA - a0);
        const uint32_t cnt_a = pw_mask(col0, 0, TWin), cnt_b = pw_mask(col0 + 4, 0, TWin);
        uint32_t s2a = 0, s1a = 0, s2b = 0, s1b = 0; // the moments of the cell's two dwords
        if (nr == CH && gi0 >= 0 && gi0 + CH <= g.fh && gj >= 0 && gj + 8 <= g.fw) { // the cell inside the frame: nothing was clamped
#pragma unroll
            for (int r = 0; r < CH; ++r) {
                const PwWords xa = pw_words(w[2 * r], 0xffffffffu, cnt_a, fill4), xb = pw_words(w[2 * r + 1], 0xffffffffu, cnt_b, fill4);
                pw_moments(s2a, s1a, xa.wz);
                pw_extremes(ext, xa);
                pw_moments(s2b, s1b, xb.wz);
                pw_extremes(ext, xb);
            }
        } else {
            const uint32_t in_a = pw_mask(gj, 0, g.fw), in_b = pw_mask(gj + 4, 0, g.fw);
            if ((in_a | in_b) == 0u || gi0 >= g.fh || gi0 + nr <= 0) { // the cell outside the frame: nr rows of fill
                const PwWords xa = pw_words(0u, 0u, cnt_a, fill4), xb = pw_words(0u, 0u, cnt_b, fill4);
                pw_moments(s2a, s1a, xa.wz);
                pw_moments(s2b, s1b, xb.wz);
                s2a *= (uint32_t)nr; s1a *= (uint32_t)nr; s2b *= (uint32_t)nr; s1b *= (uint32_t)nr;
                pw_extremes(ext, xa);
                pw_extremes(ext, xb);
            } else { // the cell on the frame's edge: the words rebuilt, a row outside the frame all fill, a row at or past NA not counted
                const PwShift sh = narrow8 ? PwShift{0u, 0u} : pw_shift(pw_clamp_col(gj, g.fw, 8) - gj, 8);
#pragma unroll
                for (int r = 0; r < CH; ++r) {
                    const bool rin = row_in(gi0 + r), rc = r < nr;
                    const uint64_t v = pw_rebuild64((uint64_t)w[2 * r] | ((uint64_t)w[2 * r + 1] << 32), sh);
                    const PwWords xa = pw_words((uint32_t)v, rin ? in_a : 0u, rc ? cnt_a : 0u, fill4);
                    const PwWords xb = pw_words((uint32_t)(v >> 32), rin ? in_b : 0u, rc ? cnt_b : 0u, fill4);
                    pw_moments(s2a, s1a, xa.wz);
                    pw_extremes(ext, xa);
                    pw_moments(s2b, s1b, xb.wz);
                    pw_extremes(ext, xb);
                }
            }
        }
        const int npx = nr * min(TWin - col0, 8);
        cell[band * ncx + cx] = pw_sum(s1a + s1b, npx, dc);
        if (refine) root[band * rp + cx] = (unsigned short)pw_root16(pw_energy(s2a + s2b, s1a + s1b, npx, dc));
        const int sda = segd[2 * cx], sdb = segd[2 * cx + 1];
        unsigned *Sb = S + 2 * band * nseg;
        if (sda == sdb) {
            if (sda >= 0) { atomicAdd(Sb + 2 * sda, s2a + s2b); atomicAdd(Sb + 2 * sda + 1, s1a + s1b); }
        } else {
            if (sda >= 0) { atomicAdd(Sb + 2 * sda, s2a); atomicAdd(Sb + 2 * sda + 1, s1a); }
            if (sdb >= 0) { atomicAdd(Sb + 2 * sdb, s2b); atomicAdd(Sb + 2 * sdb + 1, s1b); }
        }
    };
    if (tid < nitems) {
        // the cells of the whole tile dealt out in order: (band, cell) advance by the constant (NT ÷ ncx, NT mod ncx)
        int band = tid / ncx, cx = tid - band * ncx;
        const int bstep = NT / ncx, cstep = NT - bstep * ncx;
        for (int it = tid + NT; it < nitems; it += NT) {
            int nband = band + bstep, ncell = cx + cstep;
            if (ncell >= ncx) { ncell -= ncx; ++nband; }
            uint32_t nxt[2 * CH];
            cell_load(nband, ncell, nxt);
            cell_sums(band, cx, cur);
#pragma unroll
            for (int i = 0; i < 2 * CH; ++i) cur[i] = nxt[i];
            band = nband;
            cx = ncell;
        }
        cell_sums(band, cx, cur); // the thread's last cell: nothing more to request
    }
    {
        const int pmax = wave_reduce_bits(pw_pmax(ext), [](int a, int c) { return a > c ? a : c; });
        const int pmin = wave_min(pw_pmin(ext));
        if (lane == 0) { s_pmax[wave] = pmax; s_pmin[wave] = pmin; }
    }
    __syncthreads();
    PRUNE_STAMP(1); // energy pass

    // ---- the dwords that straddle a cut, a column per task: the same words, masked to the one byte ----
    for (int j = 0, nstr = s_nstr; j < nstr; ++j) {
        const int d = strd[j], gj = wj0 + 4 * d;
        const uint32_t in_cols = pw_mask(gj, 0, g.fw);
        const int gjc = narrow4 ? 0 : pw_clamp_col(gj, g.fw, 4);
        const PwShift sh = narrow4 ? PwShift{0u, 0u} : pw_shift(gjc - gj, 4);
        for (int t = tid; t < 4 * nsub; t += NT) {
            const int band = t >> 2, col = 4 * d + (t & 3), a0 = band * CH, nr = min(CH, NA - a0);
            if (col >= TWin) continue;
            const uint32_t counted = pw_mask(4 * d, col, col + 1);
            uint32_t w[CH]; // the band's eight rows of the dword, requested together
            if (!narrow4) {
#pragma unroll
                for (int r = 0; r < CH; ++r) __builtin_memcpy(&w[r], frame_at(ti0 + a0 + r, gjc), 4);
            } else {
                for (int r = 0; r < CH; ++r) w[r] = tile_word(ti0 + a0 + r, gj, row_in(ti0 + a0 + r) ? in_cols & counted : 0u);
            }
            uint32_t s2 = 0, s1 = 0;
#pragma unroll
            for (int r = 0; r < CH; ++r) { // (a row at or past NA is not counted)
                const uint32_t in = row_in(ti0 + a0 + r) ? in_cols & counted : 0u;
                pw_moments(s2, s1, pw_words(pw_rebuild32(w[r], sh), in, r < nr ? counted : 0u, fill4).wz);
            }
            unsigned *Sb = S + 2 * (band * nseg + seg_id(col));
            atomicAdd(Sb, s2);
            atomicAdd(Sb + 1, s1);
        }
    }
    PRUNE_STAMP(2); // straddle pass

    // ---- where to take L: the cell whose direction-signed 3 × 3-cell sum is largest, the first such cell in row-major
    // order.  Separably: a thread walks a run of one cell column downwards, three reads per cell for the three-sum along x
    // and the three-sum along y sliding in registers ----
    {
        int bv = -0x7fffffff, bi = 0x7fffffff;
        const int nrun = ncx >= NT ? 1 : NT / ncx, rlen = (nsub + nrun - 1) / nrun;
        const int run = ncx >= NT ? 0 : tid / ncx;
        if (run < nrun)
            for (int cx = tid - run * ncx; cx < ncx; cx += NT) {
                const bool left = cx > 0, right = cx + 1 < ncx;
                auto h3 = [&](int y) {
                    if (y < 0 || y >= nsub) return 0;
                    const int *c = cell + y * ncx + cx;
                    return c[0] + (left ? c[-1] : 0) + (right ? c[1] : 0);
                };
                const int y0 = run * rlen, y1 = min(nsub, y0 + rlen);
                int above = h3(y0 - 1), here = h3(y0);
                for (int y = y0; y < y1; ++y) {
                    const int below = h3(y + 1);
                    int s = above + here + below;
                    if (pg.darker) s = -s;
                    const int c = y * ncx + cx;
                    if (s > bv || (s == bv && c < bi)) { bv = s; bi = c; }
                    above = here;
                    here = below;
                }
            }
        const int m = wave_reduce_bits(bv, [](int a, int c) { return a > c ? a : c; });
        const int mi = wave_min(bv == m ? bi : 0x7fffffff);
        if (lane == 0) { s_cv[wave] = m; s_ci[wave] = mi; }
    }
    __syncthreads();
    if (tid == 0) {
        int wv = s_cv[0], wi = s_ci[0];
        for (int w = 1; w < NW; ++w)
            if (s_cv[w] > wv || (s_cv[w] == wv && s_ci[w] < wi)) { wv = s_cv[w]; wi = s_ci[w]; }
        s_cellbest = wi;
    }
    // ---- E[slot][band] from the slot's segments: n is geometry, the band's rows × the slot's columns ----
    for (int sl = wave; sl < g.nslots; sl += NW) {
        int c0, c1;
        slot_cols(sl, c0, c1);
        const int sa = seg_id(c0), sb = seg_id(c1); // (c0 and c1 are cuts: exactly the columns [c0, c1) lie in segments sa … sb − 1)
        for (int band = lane; band < nsub; band += 64) {
            uint32_t s2 = 0, s1 = 0;
            for (int sg = sa; sg < sb; ++sg) { s2 += S[2 * (band * nseg + sg)]; s1 += S[2 * (band * nseg + sg) + 1]; }
            E[sl * nsub + band] = pw_energy(s2, s1, min(CH, NA - band * CH) * (c1 - c0), dc);
        }
    }
    int V;
    {
        int pmax = 0, pmin = 255;
        for (int w = 0; w < NW; ++w) { pmax = max(pmax, s_pmax[w]); pmin = min(pmin, s_pmin[w]); }
        V = pw_V(pmax, pmin, dc);
    }
    __syncthreads(); // (the segment sums are dead from here: R and the patch take their place)
    PRUNE_STAMP(3); // cell choice and E
    int *hull = cell; // [nslots] (first kept block, one past the last): the cell sums are dead from here too
    for (int sl = tid; sl < g.nslots; sl += NT) { hull[2 * sl] = 0x7fffffff; hull[2 * sl + 1] = 0; }
    const int cy = s_cellbest / ncx, cx = s_cellbest - cy * ncx;
    // the cell's centre is tile pixel (8cy + 4, 8cx + 4) = the centre input of output (8cy + 4 − l÷2, 8cx + 4 − l÷2)
    const int ny = min(PB, g.n1), nx = min(PB, g.n2);
    const int oy = min(max(CH * cy + 4 - hw - PB / 2, 0), g.n1 - ny), ox = min(max(8 * cx + 4 - hw - PB / 2, 0), g.n2 - nx);
    const int PH = ny + L - 1, PW = nx + L - 1, PP = (PB + L - 1 + 3) / 4 * 4, PQ = (PW + 3) / 4;
    {
        // the patch in dwords, fill substituted (the bytes of a row's last dword past PW are read and never used)
        // A thread's dwords are requested PU at a time (all six of l = 65 at once) before the first is stored; an element past
        // the patch's end lies in a row past PH, is loaded like any other at its clamped address and is not stored.
        constexpr int PU = 6;
        uint32_t *pw32 = reinterpret_cast<uint32_t *>(patch);
        int a = tid / PQ, q = tid - a * PQ;
        const int astep = NT / PQ, qstep = NT - astep * PQ;
        // The patch lies around the target: unless that is within about l ÷ 2 of the frame's edge, all its rows and whole
        // dwords lie inside the frame (workgroup-uniform: scalars) and the words go to LDS as loaded.
        const int pi0 = ti0 + oy, pj0 = wj0 + ox;
        const bool patch_in = !NARROW && __builtin_amdgcn_readfirstlane((int)(pi0 >= 0 && pi0 + PH <= g.fh && pj0 >= 0 && pj0 + 4 * PQ <= g.fw));
        if (patch_in) {
            const uint8_t *src = frame + ((unsigned long long)(unsigned)pi0 * rs + (unsigned)pj0);
            for (int e0 = tid; e0 < PH * PQ; e0 += PU * NT) {
                int at[PU];
                uint32_t w[PU];
#pragma unroll
                for (int j = 0; j < PU; ++j) { // (an element past the patch's end is loaded at element 0's address and not stored)
                    const bool on = e0 + j * NT < PH * PQ;
                    at[j] = on ? a * (PP / 4) + q : -1;
                    __builtin_memcpy(&w[j], src + (on ? (uint32_t)a * rs + 4u * (uint32_t)q : 0u), 4);
                    q += qstep;
                    a += astep;
                    if (q >= PQ) { q -= PQ; ++a; }
                }
#pragma unroll
                for (int j = 0; j < PU; ++j)
                    if (at[j] >= 0) pw32[at[j]] = w[j];
            }
        } else {
            for (int e0 = tid; e0 < PH * PQ; e0 += PU * NT) {
                int pa[PU], pq[PU];
                uint32_t w[PU];
#pragma unroll
                for (int j = 0; j < PU; ++j) {
                    pa[j] = a;
                    pq[j] = q;
                    q += qstep;
                    a += astep;
                    if (q >= PQ) { q -= PQ; ++a; }
                }
                if (!narrow4) {
#pragma unroll
                    for (int j = 0; j < PU; ++j) __builtin_memcpy(&w[j], frame_at(ti0 + oy + pa[j], pw_clamp_col(wj0 + ox + 4 * pq[j], g.fw, 4)), 4);
                } else {
                    for (int j = 0; j < PU; ++j) {
                        const int gi = ti0 + oy + pa[j], gj = wj0 + ox + 4 * pq[j];
                        w[j] = tile_word(gi, gj, row_in(gi) ? pw_mask(gj, 0, g.fw) : 0u);
                    }
                }
#pragma unroll
                for (int j = 0; j < PU; ++j) {
                    const int gi = ti0 + oy + pa[j], gj = wj0 + ox + 4 * pq[j];
                    const uint32_t in = row_in(gi) ? pw_mask(gj, 0, g.fw) : 0u;
                    const PwShift sh = narrow4 ? PwShift{0u, 0u} : pw_shift(pw_clamp_col(gj, g.fw, 4) - gj, 4);
                    if (e0 + j * NT < PH * PQ) pw32[pa[j] * (PP / 4) + pq[j]] = pw_words(pw_rebuild32(w[j], sh), in, 0xffffffffu, fill4).wz;
                }
            }
        }
    }
    __syncthreads();
    PRUNE_STAMP(4); // patch
    // Row pass in the strips' order, per output: pairs k ascending, centre last, the taps of four pairs as one scalar load.
    // A thread is (input row, NC = 4 neighbouring outputs x0 … x0 + 3).  The outputs of a row read the same pixels, so a pixel
    // is centred ONCE, (float)p − fdc (pw_centred: two instructions), and a pair's input is one add of two centred pixels
    // (pw_pair_input), bit-equal to the (float)(p[k] + p[l−1−k] − 2·dc) this pass formed before, per output and pair, from
    // two byte extractions, an integer sum and a conversion.  Only a sliding window of centred pixels is held: the four
    // pairs k0 … k0 + 3 of the four outputs read pixels x0 + k0 … + 6 at the low end and T − 6 … T, T = x0 + l + 2 − k0, at
    // the high end — eight floats each, as two quads; a group later the window has moved by one quad, which alone is
    // loaded (low end: an aligned LDS dword; high end: v_alignbyte_b32 over the new aligned dword and the one before) and
    // converted.  Two groups per loop pass, so that the quads change roles and are never copied.
    // READS OUTSIDE THE ROW, all inside this workgroup's LDS, converted and never used: the high end's first aligned pair
    // (dprev = dn[1]) ends up to 3 bytes past the row's pitch where (l − 1) mod 4 = 0 and x0 = 4 — the next row, or for the last
    // row the 8 bytes of slack behind the patch (prune_lds; the pass before this one read the same dword); the high end's
    // read-ahead reaches at most two dwords below the row's start and the low end's one dword past its pitch where l < 17
    // (row 0: the end of R, which lies before the patch).
    {
        constexpr int NC = 4;
        const uint32_t *pw32 = reinterpret_cast<const uint32_t *>(patch);
        const float fdc = (float)dc;
        const unsigned sh_dn = (unsigned)(L - 1) & 3u; // (x0 is a multiple of 4)
        auto quad = [&](uint32_t w, float (&c)[4]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) c[i] = pw_centred((w >> (8 * i)) & 0xffu, fdc);
        };
        for (int it = tid; it < PH * (PB / NC); it += NT) {
            const int a = it / (PB / NC), x0 = (it - a * (PB / NC)) * NC;
            if (x0 >= nx) continue;
            const uint32_t *up = pw32 + a * (PP / 4) + (x0 >> 2), *dn = pw32 + a * (PP / 4) + ((x0 + L - 1) >> 2);
            uint32_t dprev = dn[1];
            auto next_lo = [&](float (&c)[4]) { quad(*up++, c); };
            auto next_hi = [&](float (&c)[4]) {
                const uint32_t d = *dn--;
                quad(__builtin_amdgcn_alignbyte(dprev, d, sh_dn), c);
                dprev = d;
            };
            // np ≤ 4 pairs from k0 on: the low window is l0 | l1 (pixels x0 + k0 … + 7), the high one h0 | h1 (T − 7 … T)
            auto group = [&](f2 (&acc)[NC], const float (&l0)[4], const float (&l1)[4], const float (&h0)[4], const float (&h1)[4], int k0, int np) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < np) {
                        const f2 t = trow[k0 + i];
#pragma unroll
                        for (int o = 0; o < NC; ++o) {
                            const int li = i + o, hi = 4 + o - i;
                            acc[o] = fma_bcast(pw_pair_input(li < 4 ? l0[li] : l1[li - 4], hi < 4 ? h0[hi] : h1[hi - 4]), t, acc[o]);
                        }
                    }
            };
            float lA[4], lB[4], hA[4], hB[4];
            next_lo(lA);
            next_lo(lB);
            next_hi(hB);
            next_hi(hA);
            f2 acc[NC];
#pragma unroll
            for (int o = 0; o < NC; ++o) acc[o] = f2{0.f, 0.f};
            int k0 = 0;
            for (; k0 + 8 <= H; k0 += 8) { // (whole groups without a test per pair)
                group(acc, lA, lB, hA, hB, k0, 4);
                next_lo(lA);
                next_hi(hB);
                group(acc, lB, lA, hB, hA, k0 + 4, 4);
                next_lo(lB);
                next_hi(hA);
            }
            if (k0 < H) { // l ÷ 2 mod 8 pairs more
                group(acc, lA, lB, hA, hB, k0, min(H - k0, 4));
                if (k0 + 4 < H) {
                    next_lo(lA);
                    next_hi(hB);
                    group(acc, lB, lA, hB, hA, k0 + 4, H - k0 - 4);
                }
            }
#pragma unroll
            for (int o = 0; o < NC; ++o) {
                acc[o] = fma_bcast(pw_centred(patch[a * PP + x0 + o + H], fdc), trow[H], acc[o]);
                if (x0 + o < nx) R[a * PB + x0 + o] = acc[o];
            }
        }
    }
    __syncthreads();
    PRUNE_STAMP(5); // row pass of L
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
            const bool can = thr > 0.0 && pg.tmax < __builtin_huge_valf();
            s_emax = can ? q * q * (1.0 - 0x1p-30) : -1.0; // −1: nothing can be excluded
            // the second stage's threshold on Σ Wq·r, whose unit is ‖K‖₂ / 2¹⁶: rounded down, the same hair low
            s_tq = can ? (long long)(q * 65536.0 * (1.0 - 0x1p-30)) : -1ll;
        }
    }
    __syncthreads();
    PRUNE_STAMP(6); // column pass of L, threshold

    // ---- per slot: the hull of the blocks that cannot be excluded.  A lane per (slot, block): the block's sub-chunks summed
    // in exact integers (any order gives the same sum), the first and one past the last kept block of a slot met by LDS
    // minimum / maximum.  (Before: a thread per slot slid the sum down the blocks, 33 dependent steps in 5 threads.) ----
    const int nblk = (g.n1 + CH - 1) / CH, NS = prune_span(L);
    {
        const double emax = s_emax;
        for (int t = tid; t < g.nslots * nblk; t += NT) {
            const int sl = t / nblk, j = t - sl * nblk;
            const unsigned *Es = E + sl * nsub + j;
            unsigned long long sum = 0;
            for (int k = 0, n = min(NS, nsub - j); k < n; ++k) sum += Es[k];
            if ((double)sum >= emax) { atomicMin(&hull[2 * sl], j); atomicMax(&hull[2 * sl + 1], j + 1); }
        }
    }
    __syncthreads();
    PRUNE_STAMP(7); // hulls
    // ---- the second stage (header comment, "the cell bound"): inside a slot's hull, a lane per (block, output cell that meets the
    // slot's columns) sums the NS × NS weighted roots, in integers; a block with a cell at or above the threshold stays, and the
    // refined range is the hull of those.  A PASS is four blocks of a strip, sixteen lanes each (nine cells at most, where the
    // strip is shifted off the cells' grid), or 64 blocks of a remainder column (one cell); the window's passes are dealt out to
    // its four waves in turn (cfg3: two kept strips of eight blocks, a pass per wave).  The weights are wave-uniform and come
    // four at a time as one scalar load, the next group requested before this one is used (a load per term, waited for at
    // once, left l = 109 at −29.5 % of the parent's step where this form reaches −38.4 %, profiles/refine_ab.txt); their rows are padded to whole groups with zeros, which meet the roots of the next
    // row.  A row's products fit 32 bits (PRUNE_REFINE_MAX_SPAN) and Wq, r fit 24 ----
    int *hull2 = hull;
    if (refine && s_tq >= 0) {
        hull2 = reinterpret_cast<int *>(smem + lo.hull2);
        for (int sl = tid; sl < g.nslots; sl += NT) { hull2[2 * sl] = 0x7fffffff; hull2[2 * sl + 1] = 0; }
        __syncthreads();
        const unsigned long long tq = (unsigned long long)s_tq;
        const uint4 *__restrict__ wq4 = reinterpret_cast<const uint4 *>(pg.wq);
        const int Q = prune_refine_pitch(NS) / 4;
        int turn = 0;
        for (int sl = 0; sl < g.nslots; ++sl) {
            const int bb = __builtin_amdgcn_readfirstlane(hull[2 * sl + 1]), ba = bb == 0 ? 0 : __builtin_amdgcn_readfirstlane(hull[2 * sl]);
            if (bb <= ba) continue;
            int c0, c1;
            slot_cols(sl, c0, c1);
            const int xb0 = c0 >> 3, ncell = ((c0 + (sl < g.nstrips ? ws : 1) - 1) >> 3) - xb0 + 1;
            const bool one = ncell == 1;
            const int c = one ? 0 : (lane & 15), jj = one ? lane : lane >> 4;
            for (int j0 = ba; j0 < bb; j0 += one ? 64 : 4, ++turn) {
                if ((turn & (NW - 1)) != wave) continue;
                const int j = j0 + jj;
                if (j < bb && c < ncell) {
                    const unsigned short *rr = root + j * rp + xb0 + c;
                    unsigned long long B = 0;
                    uint4 w = wq4[0];
                    for (int dy = 0; dy < NS; ++dy, rr += rp) {
                        uint32_t row = 0;
                        for (int q = 0; q < Q; ++q) {
                            const uint4 wn = wq4[dy * Q + q + 1]; // (the table ends with a group of zeros)
                            row += pw_mul24(w.x, rr[4 * q]) + pw_mul24(w.y, rr[4 * q + 1]) + pw_mul24(w.z, rr[4 * q + 2]) + pw_mul24(w.w, rr[4 * q + 3]);
                            w = wn;
                        }
                        B += row;
                    }
                    if (B >= tq) { atomicMin(&hull2[2 * sl], j); atomicMax(&hull2[2 * sl + 1], j + 1); }
                }
            }
        }
        __syncthreads();
    }
    // ---- the window's slots are filed by its first wave, 64 at a time: the range words, the finished partial of a strip with
    // an empty hull, and the window's kept strips as consecutive entries of the job list (header comment) ----
    if (wave == 0) {
        int kept = 0, njobs = 0;
        // (what the strips run is the refined range; `kept`, the count the policy reads, stays the first stage's)
        auto slot_hull = [&](int sl, int &ba, int &bb) {
            ba = bb = 0;
            if (sl < g.nslots) {
                bb = hull2[2 * sl + 1];
                ba = bb == 0 ? 0 : hull2[2 * sl];
            }
            return sl < g.nstrips && bb > ba; // a job
        };
        for (int sl0 = 0; sl0 < g.nslots; sl0 += 64) {
            const int sl = sl0 + lane;
            int ba, bb;
            const bool job = slot_hull(sl, ba, bb);
            if (sl < g.nslots) {
                const long long o = (long long)b * g.nslots + sl;
                // (a remainder column's word carries the DC level: dog_thin_kernel skips its samples.  A strip's word stays
                // as it was: the word of an empty strip is its column mask, 0)
                const unsigned lo = (unsigned)ba | (sl < g.nstrips ? 0u : (unsigned)dc << 24);
                g.part_mask[o] = (unsigned long long)lo | ((unsigned long long)(unsigned)bb << 32);
                if (sl < g.nstrips && !job) { // what the strip's wave would have left: an initialised Peak
                    Peak pk;
                    peak_init(pk);
                    g.part_val[o] = pk.best;
                    g.part_idx[o] = pk.idx;
                    g.part_sec[o] = pk.second;
                }
                const int b1 = hull[2 * sl + 1], a1 = b1 == 0 ? 0 : hull[2 * sl];
                kept += prune_sc_hi(a1, b1, L, nsub) - a1;
            }
            njobs += __builtin_popcountll(__builtin_amdgcn_ballot_w64(job));
        }
        kept = wave_sum(kept);
        // ONE returning atomic per workgroup, relaxed: stat[2] is the packed word of dog_prune_publish.hpp (arrivals, jobs
        // appended, pairs kept) and the add returns the state before this workgroup — how many arrived before it, the place of
        // this window's entries in the list, and what the earlier windows kept.  The last workgroup of the batch so holds the
        // batch's job count and kept pairs in registers (the returned fields plus its own; the batch's total is geometry,
        // n · nslots · nsub) and reads nobody else's memory: it alone adds the two sums to the cumulative stat[0] and stat[1],
        // publishes what those adds return plus the sums where the host sees it without a copy or a wait (the way
        // dog_finish_kernel publishes its flagged count: one plain store per batch), writes the batch's job count to the
        // list's header, where the strips read it, and zeroes stat[2] for the next batch.
        // WHY NO ORDERING IS NEEDED.  The read-modify-writes on one address have a single total order whatever their memory
        // order, so every workgroup sees the exact sum of those before it and exactly one sees n − 1 arrivals.  The list
        // entries, part_mask and the empty strips' Peak are read by later kernels in the stream, and stat[0] / stat[1] by
        // pdog_get_prune_counts after a drain: the kernel boundary orders them.  The zeroing store follows the same thread's
        // add on the same address, and nobody adds after the last arriver.
        // (Before: every workgroup added its counts to stat[0] and stat[1] and the arrival was acquire-release at agent scope,
        // so that the last one might load those two words.  On this part that ordering is cache maintenance — a write-back of
        // the XCD's L2 ahead of the atomic and an invalidate after it, once per workgroup, 4096 times per cfg3 step, under
        // everybody else's tile loads; profiles/publish_ab.txt.  That form remains behind PRUNE_FENCED_PUBLISH for batches
        // whose counts do not fit the packed fields (pp_fits) and for pdog_set_tuning "fenced_publish".  Tried there: arrival
        // and kept pairs in one atomic instead of three on neighbouring words, the fence kept: the kernel's time did not move.
        // A separate running job count, a second returning atomic per workgroup: the kernel 5 % slower.)
        unsigned base = 0;
        if (lane == 0) {
            if (g.prune & PRUNE_FENCED_PUBLISH) {
                __hip_atomic_fetch_add(pg.stat, (unsigned long long)kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(pg.stat + 1, (unsigned long long)(g.nslots * nsub), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long v = __hip_atomic_fetch_add(pg.stat + 2, 1ull | ((unsigned long long)njobs << 32), __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                base = (unsigned)(v >> 32);
                if ((unsigned)v == gridDim.x - 1) {
                    __hip_atomic_store(pg.stat + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long k = __hip_atomic_load(pg.stat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), tt = __hip_atomic_load(pg.stat + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(pg.host, pp_host_word(k, tt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(&pg.jobs[0].b, (int)(base + (unsigned)njobs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                const unsigned long long v = __hip_atomic_fetch_add(pg.stat + 2, (unsigned long long)pp_increment((uint32_t)njobs, (uint32_t)kept), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const PpArrival a = pp_arrive(v, (uint32_t)njobs, (uint32_t)kept, gridDim.x);
                base = a.base;
                if (a.last) {
                    __hip_atomic_store(pg.stat + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long total = (unsigned long long)gridDim.x * (unsigned long long)(g.nslots * nsub);
                    const unsigned long long k = __hip_atomic_fetch_add(pg.stat, (unsigned long long)a.kept, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + a.kept;
                    const unsigned long long tt = __hip_atomic_fetch_add(pg.stat + 1, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + total;
                    __hip_atomic_store(pg.host, pp_host_word(k, tt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(&pg.jobs[0].b, (int)a.jobs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        base = __builtin_amdgcn_readfirstlane(base);
        if (njobs)
            for (int sl0 = 0; sl0 < g.nstrips; sl0 += 64) {
                const int sl = sl0 + lane;
                int ba, bb;
                const bool job = slot_hull(sl, ba, bb);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(job);
                // (1 + …: entry 0 is the header.  A batch appends at most n · nstrips jobs, the list's room; the test holds a
                // count that an aborted batch left behind inside it)
                const unsigned at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if (job && at < (unsigned)(g.n * g.nstrips)) pg.jobs[1 + at] = PruneJob{b, sl | (dc << 16), ba, bb};
                base += (unsigned)__builtin_popcountll(m);
            }
    }
    PRUNE_STAMP(8); // publish
#ifdef PDOG_ABLATIONS
    if (tid == 0) atomicAdd(pg.stat + 4 + PRUNE_PHASES, 1ull);
#endif
#undef PRUNE_STAMP
}
#endif // PDOG_ROLL_INST_ONLY

} // namespace pdog
