// dog_roll.hpp — barrier-free "rolling accumulator" DoG + argmax kernel for gfx950.
//
// Same arithmetic contract as dog_kernels.hpp (reference functor
// /root/reference/src/PawsomeTracker.jl:55-62), different execution shape:
//
//   * one WAVE (64 lanes, one workgroup) owns a strip of 64 window columns for the
//     whole window height; nothing is shared between waves, so there is no
//     s_barrier anywhere and the only LDS is a wave-private 8 KB staging area;
//   * input rows stream through in sub-chunks of CH = 8 rows:
//       stage   8 rows × 128 u8 (16 B per lane, prefetched one sub-chunk ahead)
//               → (pixel − dc) as f32 in LDS
//       row pass  lane = (row r, group of P = 8 consecutive outputs), sliding register
//               window, symmetric taps: Σ_k g[k]·(a[x−k] + a[x+k]) — one v_add + one
//               v_pk_fma_f32 (both Gaussians) per tap pair instead of two FMAs
//       column pass  lane = column; the l partial sums a column has in flight live in
//               REGISTERS (S = l−1+CH f32 accumulator slots, output y in slot y mod S, two
//               adjacent outputs per register pair / v_pk_fma_f32), so each
//               R row is read from LDS exactly once (8 ds_read_b64 per sub-chunk per lane)
//               instead of (Q+l−1)/Q times from a 64+ row LDS ring.  The slot ↔ tap
//               mapping rotates by CH per sub-chunk; S/CH statically unrolled bodies are
//               selected by a wave-uniform switch, so every register index is a constant.
//   * completed outputs feed a running (max, first column-major index) per lane;
//     wave-shuffle reduction at the end, one partial per strip.
//
//   * PADDING ROWS.  The reference pads the frame with `fill` (PaddedView, src/PawsomeTracker.jl:48), so a window near the
//     frame's edge has sub-chunks — 8 tile rows of a strip — that hold padding only: all 8 rows above or below the frame, or a
//     strip whose staged columns all lie left or right of it.  When the window's DC level equals the fill (dc_from_sum snaps
//     to it within 8 levels) every input of such a sub-chunk is fill − dc = +0, and the sub-chunk skips the u8 → f32
//     conversion and its LDS stores, the row pass with both fence / barrier pairs, the R reads and the column FMAs
//     (roll_col_zero instead of roll_col_body); the prefetch of the next sub-chunk, the emit part and the peak tracking
//     stay.  The test is wave-uniform (kernel arguments and readfirstlane(dc), kept as two sub-chunk numbers per strip:
//     padding above pad_top, padding from pad_bot on): the translation units are built with
//     -structurizecfg-skip-uniform-regions and rely on it.  Rows past the tile's end (a ≥ n1 + l − 1) already read as fill,
//     but a last sub-chunk that mixes them with in-frame rows is NOT padding: the test looks at frame rows only.
//     Why the bits do not change:
//       row pass      v = +0 for every input: each pair sum is +0, every Gaussian tap is positive, fma(+0, g, +0) = +0,
//                     so R = (+0, +0).
//       first term    of an output: the multiply gives (+0)·(s·g₊[0]) = ±0, the next FMA adds (+0)·(−s·g₋[0]) = ∓0: +0 for
//                     either sign of s.  The odd output of the register pair starts from (+0)·T[−1] = +0.  "slot := +0" is
//                     what the full body computes.
//       later terms   fma(+0, t, a) = a for every a ≠ −0, and a = −0 cannot stand in an accumulator at a row boundary: a
//                     finished (+, −) pair of zero products cancels to +0 under round-to-nearest, sums of non-zero terms that
//                     cancel give +0 too, and the values do not underflow.  Taps are finite: no 0·inf.
//     (tests/test_pad_rows_cpu.py states this in float32; tests/test_gpu_pad_rows.py compares the maps with the skip off.)
//     Out of scope, on purpose: dc ≠ fill (R is a non-zero constant there, only the row pass could go, and the case is
//     rare); rows inside the frame that happen to equal the fill; partially padded sub-chunks (in the row pass rows are
//     lanes: nothing would be saved); dog_thin_kernel (it runs beside the strips and is shorter than they are); the ring,
//     two-pass, fused and tiled kernels.  pdog_set_tuning "no_pad_skip" pins the full path.
//
// On gfx950 v_pk_fma_f32 issues at the same FLOP rate as v_fma_f32 (4 vs 2 cycles per
// wave64, tools/ubench_valu.hip), so what counts is the number of lane-operations, and one
// wave per SIMD already reaches ≈84 % of the packed-FMA rate: occupancy 2 waves/SIMD
// (≤ 256 VGPRs) is enough once there are no barriers.
#pragma once
#include "dog_kernels.hpp"
#include "dog_exact.hpp"
#include "pdog_predict.hpp"
#include "dog_roll_range.hpp" // ROLL_CH, ROLL_QB, the tap-block counts, prune_sc_hi and the range-end rule: host-testable
#include <type_traits>

namespace pdog {

#ifndef PDOG_ROLL_LMAX
#define PDOG_ROLL_LMAX 149
#endif
// (ROLL_P, ROLL_TW, ROLL_PR and ROLL_LMIN are dog_layout.hpp's.)
constexpr int ROLL_LMAX = PDOG_ROLL_LMAX;     // kernel lengths with a roll instance (l = 4m+1): the (l + 7 rounded up to 8)
                                              // accumulator slots, the row-pass windows and the loop state fit 168 VGPRs up to l = 81 (three waves
                                              // per SIMD) and 256 from there to l = 149 (two; roll_lengths.def builds every length, none spills:
                                              // profiles/pad_skip_kernel_regs.txt); longer kernels go to dog_twopass.hpp
__host__ __device__ constexpr int roll_waves(int L) { return L <= 81 ? 3 : 2; } // waves per SIMD the instance is compiled for
// Kernel lengths whose instances can FOLD a single remainder column into the last strip (LaunchGeo::fold_r).  The second
// row-pass variant costs ≈18 VGPRs: l = 65 (the reference's default target_width) absorbs them inside its three-waves budget
// (163 of 168); the neighbouring lengths would lose a wave per SIMD to it and keep dog_thin_kernel instead.
__host__ __device__ constexpr bool roll_folds(int L) { return L == 65; }

// accumulator slots: the l outputs in flight plus the sub-chunk being emitted, rounded so that the
// slot ↔ tap mapping repeats after a whole number of sub-chunks
__host__ __device__ constexpr int roll_slots(int L) { return (L - 1 + ROLL_CH + ROLL_CH - 1) / ROLL_CH * ROLL_CH; }
// (staging: roll_sb, roll_rs and roll_lds_bytes are dog_layout.hpp's; a row's base carries the skew described there.)
__host__ __device__ constexpr int roll_row_base(int r, int L) { return r * roll_rs(L) + 4 * (((r & 1) ? 1 : 0) + ((r & 2) ? 8 : 0)); }

// (KEPT RANGES: prune_span, prune_tail and prune_sc_hi are dog_roll_range.hpp's.)

// Which entry of the job list workgroup `blk` of a PRUNE launch takes.  Consecutive workgroups go to consecutive XCDs, so
// blk & 7 is the XCD and blk >> 3 the workgroup's turn on it: the list is dealt out in groups of G = 2^k consecutive entries
// (LaunchGeo::prune), group after group over all eight XCDs — a list of any length is spread evenly, and with G > 1 a
// window's neighbouring entries mostly share an L2.  A bijection on [0, grid) for a grid that is a multiple of 8·G.
__host__ __device__ constexpr int prune_job_index(int blk, int G)
{
    const unsigned turn = (unsigned)blk >> 3, xcd = (unsigned)blk & 7u, g = (unsigned)G;
    return (int)((turn / g * 8u + xcd) * g + turn % g);
}

// Re-derive a tap pointer through an empty asm: the scalar loads that use it cannot be hoisted above
// this point (hoisted, every block's taps are live at once and the SGPRs spill through v_writelane).
// A fake use + redefinition of an accumulator pair: the FMAs that feed it cannot be sunk below this
// point and later ones cannot be hoisted above it (keeps each tap block's FMAs next to its taps).
__device__ __forceinline__ void pin_acc(f2 &a) { asm volatile("" : "+v"(a)); }

__device__ __forceinline__ tap_ptr pin_taps(tap_ptr p)
{
    unsigned long long u = (unsigned long long)p;
    asm volatile("" : "+s"(u));
    return (tap_ptr)u;
}

// Row pass for one lane: P = 8 outputs, symmetric taps, everything in 4-cycle packed ops
// (a lone wave issues one VALU instruction per ≈4.8 cycles whatever its width, so 2-cycle
// scalar ops would leave the pipe half empty at few waves per SIMD):
//   s2      = (a[o+k], a[o+1+k]) + (a[o+L-1-k], a[o+L-k])                 v_pk_add_f32
//   acc[o]  += s2.x · (g+[k], g−[k]);  acc[o+1] += s2.y · (g+[k], g−[k])   v_pk_fma_f32 (op_sel broadcast)
// VGPR pairs must be even-aligned and L − 1 is a multiple of 4, so o + k must be even: EVEN taps pair the outputs
// (0,1) (2,3) (4,5) (6,7), ODD taps pair (−1,0) (1,2) (3,4) (5,6) (7,8) — a fifth v_pk_add_f32 whose outer halves
// are not used, instead of the ≈50 v_pk_mov_b32 / v_mov_b32 per sub-chunk that assembled odd-aligned register pairs
// in round 2.  Every operand is then an even pair E[p] = (a[2p], a[2p+1]) of the lane's 16-byte aligned span: the
// inputs arrive as ds_read_b128 quads, each read once, and the sliding windows shrink to 3 + 3 quads (24 VGPRs
// instead of 40 + 16 staged) — what lets the kernel run three waves per SIMD.
//   tap k = 4J+u, block J:  lo pairs E[2J … 2J+5] = quads J … J+2,  hi pairs E[H−2J−2 … H−2J+3] = quads H/2−J−1 … H/2−J+1
// a = &A[r][P*gx] (16-byte aligned); inputs a[0 .. P+L-2].  Taps ascending k = 0..H-1, centre last: same order for
// every output, so equal inputs give bit-equal outputs.
typedef float f4 __attribute__((ext_vector_type(4)));
// NOUT = 9: the lane also computes output 8 — for the last lane group of a FOLDED strip that is window column 64·k of a
// window 64·k + 1 columns wide (257, 513, …), the column round 2 gave to dog_thin_kernel.  The odd taps already hold its
// pair sums (the outer half of their fifth v_pk_add_f32), the even taps add one: +49 packed instructions per sub-chunk
// in the one strip per window that folds, instead of a second kernel re-reading a 65-column patch per window.
// NOUT = 4: four outputs per lane (pairs (0,1) (2,3) / (−1,0) (1,2) (3,4), two-quad windows) for the latency kernels' small tiles,
// where tasks of 8 outputs leave most of a 1024-thread workgroup without one (dog_tiled.hpp).
template <int L, int NOUT = ROLL_P>
__device__ __forceinline__ void roll_row_pass(f2 (&acc)[NOUT == 9 ? ROLL_P + 2 : NOUT], const float *a, tap_ptr taps)
{
    constexpr int P = (NOUT == 9) ? 8 : NOUT, H = L / 2, U = 4, NB = (H + U - 1) / U, HQ = H / 2;
    constexpr int NLO = P / 4 + 1;                       // lo-window quads: pairs 2J … 2J + P/2 + 1
    constexpr int NHI = NLO + (NOUT == 9 ? 1 : 0);       // hi-window quads
    constexpr int ME = P / 2 + (NOUT == 9 ? 1 : 0);      // pair sums per even tap
    constexpr int MO = P / 2 + 1;                        // pair sums per odd tap
    static_assert((P == 8 || P == 4) && (NOUT == 4 || NOUT == 8 || NOUT == 9) && H % 2 == 0, "the pairing below is written for 4 or 8 (+1) outputs and L = 4m + 1");
    auto quad = [&](int q) { return *reinterpret_cast<const f4 *>(a + 4 * q); };
    auto half = [](const f4 &v, int h) { return h ? __builtin_shufflevector(v, v, 2, 3) : __builtin_shufflevector(v, v, 0, 1); };
    f4 lw[NLO], hw[NHI]; // quads J … J+NLO−1 and HQ−J−1 … HQ−J−2+NHI
#pragma unroll
    for (int j = 0; j < NLO; ++j) lw[j] = quad(j);
#pragma unroll
    for (int j = 0; j < NHI; ++j) hw[j] = quad(HQ - 1 + j);
    f2 tn[U];
    tap_ptr tb = pin_taps(taps); // ONE base re-pinned in place per block: the loads below keep constant offsets from it
#pragma unroll                   // (an opaque pointer per block made 9 loop-invariant address pairs, all spilled to VGPR lanes)
    for (int j = 0; j < U; ++j) tn[j] = tb[j];
#pragma unroll
    for (int J = 0; J < NB; ++J) {
        const int k0 = U * J;
        const int nu = (H - k0 < U) ? (H - k0) : U; // the last block holds two taps when H is not a multiple of 4
        const bool more = (J + 1 < NB);
        f2 t[U];
#pragma unroll
        for (int j = 0; j < U; ++j) t[j] = tn[j];
        f4 nl = lw[NLO - 1], nh = hw[0];
        tb = pin_taps(tb);
        const tap_ptr tnext = tb + (more ? k0 + U : H);
        if (more) {
#pragma unroll
            for (int j = 0; j < U; ++j) tn[j] = tnext[j]; // may run past tap H−1 on the last full load: those entries are never used
            nl = quad(J + NLO);    // new upper quad of the next lo window
            nh = quad(HQ - J - 2); // new lower quad of the next hi window
        } else {
            tn[0] = tnext[0]; // centre tap
        }
        auto LO = [&](int p) { return half(lw[(p >> 1) - J], p & 1); };
        auto HI = [&](int p) { return half(hw[(p >> 1) - (HQ - J - 1)], p & 1); };
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < nu) {
                const int k = k0 + u;
                if ((k & 1) == 0) {
#pragma unroll
                    for (int m = 0; m < ME; ++m) {
                        const f2 s2 = LO(k / 2 + m) + HI(H - k / 2 + m);
                        acc[2 * m] = fma_bcast(s2.x, t[u], acc[2 * m]);
                        if (m < P / 2) acc[2 * m + 1] = fma_bcast(s2.y, t[u], acc[2 * m + 1]);
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < MO; ++m) {
                        const f2 s2 = LO((k - 1) / 2 + m) + HI(H - (k + 1) / 2 + m);
                        if (m >= 1) acc[2 * m - 1] = fma_bcast(s2.x, t[u], acc[2 * m - 1]);
                        if (m < P / 2 || NOUT == 9) acc[2 * m] = fma_bcast(s2.y, t[u], acc[2 * m]);
                    }
                }
            }
        }
        if (more) {
#pragma unroll
            for (int j = 0; j + 1 < NLO; ++j) lw[j] = lw[j + 1];
            lw[NLO - 1] = nl;
#pragma unroll
            for (int j = NHI - 1; j > 0; --j) hw[j] = hw[j - 1];
            hw[0] = nh;
        } else {
            // centre tap: a[o + H], the pairs E[HQ … HQ + P/2 − 1 (+1)] — inside the last hi window whatever H mod 4 is
#pragma unroll
            for (int m = 0; m < ME; ++m) {
                const f2 c2 = HI(HQ + m);
                acc[2 * m] = fma_bcast(c2.x, tn[0], acc[2 * m]);
                if (m < P / 2) acc[2 * m + 1] = fma_bcast(c2.y, tn[0], acc[2 * m + 1]);
            }
        }
#pragma unroll
        for (int o = 0; o < NOUT; ++o) pin_acc(acc[o]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Column-pass tap table for the rolling kernel (built on the host, pawsome_dog.hip): the f32
// accumulators of two adjacent outputs (slots j, j+1, j even) share one register pair and one
// v_pk_fma_f32 whose tap operand is the SGPR pair (T[t], T[t-1]).  Which t a row needs depends on
// its parity p = a & 1 (t ≡ p mod 2), so there are two pairings; T[-1] = T[l] = 0.
//   table[((qb*2 + p)*2 + c)*ROLL_QB + m] = (Tc[t], Tc[t-1]),  t = p + 2*(ROLL_QB*qb + m),
//   c = 0: s·g+, c = 1: −s·g−
// (ROLL_QB = 2 tap pairs per block and roll_col_blocks: dog_roll_range.hpp)
__host__ __device__ constexpr int roll_col_table_len(int L) { return roll_col_blocks(L) * 4 * ROLL_QB; } // in f2

// Column pass body for sub-chunk phase SC (rows a ≡ CH*SC + i mod S).  rv[i] = (R+, R−)[row i][x].
// Loop order (tap block, row, channel): every output receives its terms as t = 0: (+,−), 1: (+,−), …
// whatever its alignment to blocks and sub-chunks, so equal inputs give bit-equal outputs.
// QHI < roll_col_blocks(L): a prologue body.  The first input rows a < l−1 have no output above row 0 to feed: rows
// a … a+7 of sub-chunk sc only need taps t ≤ a+7, i.e. tap blocks 0 … 2sc+1 — the rest of the scatter would land in
// slots whose outputs do not exist (20 % of the column pass's FMAs over the first and last l−1 rows).  Up there the
// phase equals the sub-chunk number, so the shortened bodies are static instances with no branch inside.
// (roll_prologue_blocks(sc) = 2 sc + 2, roll_prologue_len: dog_roll_range.hpp)
// Bottom edge: rows a = 8 sc … need tap blocks qb ≥ qlo(sc) = 2 sc − c0, c0 = (n1 + 2) ÷ 4.  With the phase sc mod NBODY
// the pair (phase, qlo) of every epilogue sub-chunk is fixed by c0 mod 2·NBODY: the window's height class.
__host__ __device__ constexpr int roll_epi_c0(int n1) { return (n1 + 2) / 4; }
__host__ __device__ constexpr int roll_epi_class(int n1, int L) { return roll_epi_c0(n1) % (2 * (roll_slots(L) / ROLL_CH)); }
// The shortened bodies at the START of a run of sub-chunks (a window's top; a kept range's first sub-chunk, roll_strip):
// sub-chunk j of the run, rows a = 8j … 8j + 7 counted from its first row, runs tap blocks 0 … roll_prologue_blocks(j) − 1
// (all of them from j = roll_prologue_len on).  True iff those blocks hold every tap t of every output y = a − t ≥ 0 of the
// run, i.e. of every output at or below the run's first row.  Row a (parity p) meets tap t in the pair (T[tt], T[tt − 1]),
// tt = t or t + 1 with tt ≡ p mod 2, which lies in block (tt − p) ÷ 2 ÷ ROLL_QB (roll_col_body).
__host__ __device__ constexpr bool roll_start_covers(int L)
{
    for (int j = 0; j < roll_prologue_len(L); ++j) {
        const int nblk = roll_prologue_blocks(j) < roll_col_blocks(L) ? roll_prologue_blocks(j) : roll_col_blocks(L);
        for (int i = 0; i < ROLL_CH; ++i) {
            const int a = ROLL_CH * j + i, p = a & 1;
            for (int t = 0; t <= a && t <= L - 1; ++t) {
                const int tt = ((t ^ p) & 1) ? t + 1 : t;
                if ((tt - p) / 2 / ROLL_QB >= nblk) return false;
            }
        }
    }
    return true;
}
#define PDOG_ROLL_L(LT) static_assert(roll_start_covers(LT), "a shortened prologue body leaves out a tap of an output inside the range");
#include "roll_lengths.def"
#undef PDOG_ROLL_L
// … and at the END of a kept range (dog_roll_range.hpp): entering a body at block roll_end_qlo leaves out no tap of an output
// the loop still emits, and a prologue body that is entered late keeps at least one block.
#define PDOG_ROLL_L(LT)                                                                                                     \
    static_assert(roll_end_covers(LT), "the range-end entry leaves out a tap of an emitted output, or enters too early");   \
    static_assert(roll_end_meets_prologue(LT), "a prologue body would be entered at or past its own last block");
#include "roll_lengths.def"
#undef PDOG_ROLL_L
// QLO > 0: an EPILOGUE body, blocks QLO … only: the last input rows a > n1−1 have no output below row n1−1 to feed,
// rows a … a+7 only need taps t ≥ a − (n1−1).  Down there sub-chunk and phase are tied through the window height, so
// these bodies exist per HEIGHT CLASS (roll_epi_class) — instances for the common window sizes only.
// ENTRY: the body of a PRUNE instance, entered at the wave-uniform RUN-TIME block qlo < QHI (the END of a kept range,
// dog_roll_range.hpp: blocks below roll_end_qlo only feed outputs past the last one the loop emits; qlo is roll_end_entry's,
// a multiple of roll_entry_step(L) — one entry point per 4 or 8 blocks, for the compile time's sake).  A switch jumps into the
// unrolled block sequence and falls through: a skipped block has no FMAs, no tap loads, no pin_acc and no sched_barrier, and
// every block from qlo on is the code it is without the entry — the entry block's taps are loaded by the run-time index
// ahead of the switch into the registers the block before it would have filled.  Skipping block 0 skips the tt == 0
// multiply that restarts slots: those slots belong to outputs past y_end, and nothing reads them again.
template <int L, int SC, int QHI = roll_col_blocks(L), int QLO = 0, bool ENTRY = false>
__device__ __forceinline__ void roll_col_body(f2 (&acc2)[roll_slots(L) / 2], const f2 (&rv)[ROLL_CH], tap_ptr table, int qlo = 0)
{
    constexpr int S = roll_slots(L), CH = ROLL_CH, QB = ROLL_QB, NQB = QHI;
    static_assert(QHI >= 1 && QHI <= roll_col_blocks(L) && QLO >= 0 && QLO < QHI, "tap-block bounds out of range");
    static_assert(S % 2 == 0 && (CH * SC) % 2 == 0, "pairing needs even slot counts");
    static_assert(!ENTRY || QLO == 0, "a run-time entry replaces the static first block");
    f2 tn[4 * QB];
    tap_ptr tb = pin_taps(table);
#pragma unroll
    for (int j = 0; j < 4 * QB; ++j) tn[j] = tb[(ENTRY ? qlo : QLO) * 4 * QB + j];
    // ENTRY: the R values as a copy that every block re-derives through an empty asm.  fma_bcast's (r, r) operand is an op_sel
    // broadcast only where the splat and the FMA share a basic block; with the entry a body is several blocks, the splats
    // of the 16 R values were built once ahead of them — 32 v_mov_b32 per sub-chunk and 32 VGPRs held, 2.4 % of the headline
    // step with qlo pinned to 0.  A value that is new in every block keeps its splat there.  (Every other instance reads rv
    // itself: with the copy the response-writing instances of l = 17 … 29 took two VGPRs more.)
    f2 rw[ENTRY ? CH : 1];
    if constexpr (ENTRY) {
#pragma unroll
        for (int i = 0; i < CH; ++i) rw[i] = rv[i];
    }
    auto block = [&](const int qb) __attribute__((always_inline)) {
        if constexpr (ENTRY) {
#pragma unroll
            for (int i = 0; i < CH; ++i) pin_acc(rw[i]);
        }
        f2 t[4 * QB];
#pragma unroll
        for (int j = 0; j < 4 * QB; ++j) t[j] = tn[j];
        if (qb + 1 < NQB) {
            tb = pin_taps(tb);
            const tap_ptr tnext = tb + (qb + 1) * 4 * QB;
#pragma unroll
            for (int j = 0; j < 4 * QB; ++j) tn[j] = tnext[j];
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int par = i & 1;
            const int amod = CH * SC + i;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int m = 0; m < QB; ++m) {
                    const int tt = par + 2 * (QB * qb + m); // taps (tt, tt-1)
                    if (tt - 1 <= L - 1) {
                        const int slot = ((amod - tt) % S + S) % S; // even
                        float r;
                        if constexpr (ENTRY) r = c ? rw[i].y : rw[i].x;
                        else r = c ? rv[i].y : rv[i].x;
                        // An even row's pair (T[0], T[−1] = 0) is the FIRST term of outputs (a, a+1) — the slots the
                        // sub-chunk S rows earlier emitted: a multiply starts them from scratch (no reset instructions;
                        // output a+1 starts at ±0 and meets its own first term, row a+1's T[0], later in this block).
                        if (tt == 0 && c == 0)
                            acc2[slot / 2] = f2{r, r} * t[(par * 2 + c) * QB + m];
                        else
                            acc2[slot / 2] = fma_bcast(r, t[(par * 2 + c) * QB + m], acc2[slot / 2]);
                    }
                }
            }
        }
        // pin exactly the pairs this block touched (pinning idle ones makes the allocator copy them)
#pragma unroll
        for (int i = 0; i < CH; ++i) {
#pragma unroll
            for (int m = 0; m < QB; ++m) {
                const int tt = (i & 1) + 2 * (QB * qb + m);
                if (tt - 1 <= L - 1) pin_acc(acc2[(((CH * SC + i - tt) % S + S) % S) / 2]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (ENTRY) {
        static_assert(roll_col_blocks(ROLL_LMAX) <= 38, "extend the entry switch");
#define PDOG_BLK(k)                                                                                                          \
    if constexpr ((k) < NQB) block(k);
#define PDOG_BLK4(k) PDOG_BLK(k) PDOG_BLK((k) + 1) PDOG_BLK((k) + 2) PDOG_BLK((k) + 3)
#define PDOG_ENT4(k)                                                                                                         \
    [[fallthrough]];                                                                                                          \
    case k:                                                                                                                   \
        PDOG_BLK4(k)
#define PDOG_ENT8(k) PDOG_ENT4(k) PDOG_BLK4((k) + 4)
        // one case per roll_entry_step(L) blocks; qlo is a multiple of it (roll_end_entry)
        if constexpr (roll_entry_step(L) == 4) {
            switch (qlo) {
            case 0:
                PDOG_BLK4(0)
                PDOG_ENT4(4) PDOG_ENT4(8) PDOG_ENT4(12) PDOG_ENT4(16) PDOG_ENT4(20)
                break;
            default: break; // (never taken: qlo is a multiple of the step, roll_end_entry, and lies below QHI, roll_end_meets_prologue)
            }
            static_assert(roll_entry_step(L) != 4 || roll_col_blocks(L) <= 24, "extend the entry switch");
        } else {
            static_assert(roll_entry_step(L) == 4 || roll_entry_step(L) == 8, "one case per 4 or 8 blocks");
            switch (qlo) {
            case 0:
                PDOG_BLK4(0) PDOG_BLK4(4)
                PDOG_ENT8(8) PDOG_ENT8(16) PDOG_ENT8(24) PDOG_ENT8(32)
                break;
            default: break; // (never taken, as above)
            }
        }
#undef PDOG_ENT8
#undef PDOG_ENT4
#undef PDOG_BLK4
#undef PDOG_BLK
    } else {
#pragma unroll
        for (int qb = QLO; qb < NQB; ++qb) block(qb);
    }
}

// Column pass of a PADDING-ONLY sub-chunk (roll_strip, "padding rows"): every R value is (+0, +0), so all the body would do
// is restart the slot pairs of the even rows' first term (the tt == 0 multiply) at (+0, +0) and add exact zeros elsewhere.
template <int L, int SC>
__device__ __forceinline__ void roll_col_zero(f2 (&acc2)[roll_slots(L) / 2])
{
    constexpr int S = roll_slots(L), CH = ROLL_CH;
#pragma unroll
    for (int i = 0; i < CH; i += 2) acc2[((CH * SC + i) % S) / 2] = f2{0.f, 0.f};
}

// ABL: timing-only ablation bits (tools/tune): 1 = no column FMAs, 2 = no row pass, 4 = no staging
// conversion/LDS writes, 8 = no global loads.  ABL != 0 gives wrong results by design.
// One strip of one window, executed by ONE wave with wave-private LDS at `smem`: everything from the DC
// level to the wave-level peak reduction.  (best, best_idx) are valid in lane 0 on return.
// EPI ≥ 0: the instance for windows of height class EPI (roll_epi_class): statically shortened epilogue bodies too.
// PRUNE: the instance that honours a kept range (dog_prune.hpp).  A template flag, not a run-time branch: the two more uniform
// values cost the l = 65 height-class instances, which sit at their 168-VGPR budget, 27 … 166 spilled VGPRs.  With the flag
// the height-class instances compile as before, figure for figure; the other dense instances and the chain instances share
// the loop's new start and the skipped-strip test with constant operands and move by at most 2 VGPRs and 2 SGPR spills
// (l = 65 without a height class: 22 → 24 SGPR spills; three chain instances from l = 121 on spill one VGPR more) — all
// inside their budgets (profiles/prune_kernel_regs.txt).  The PRUNE instances exist for EPI = −1 only (a kept range seldom
// reaches the window's last rows, where the shortened epilogue bodies pay).
template <int LT, bool RESP, int ABL, int EPI = -1, bool PRUNE = false>
__device__ __forceinline__ void roll_strip(const LaunchGeo &g, const f2 *__restrict__ taps_row, const f2 *__restrict__ taps_col,
                                           unsigned char *smem, const uint8_t *__restrict__ frame, int g1, int g2, int s,
                                           int b, int logical, Peak &peak_out, unsigned long long &mask_out, int job_ba = 0, int job_bb = 0,
                                           int job_dc = 0)
{
    constexpr int L = LT, hw = L / 2, S = roll_slots(L), CH = ROLL_CH, P = ROLL_P, TW = ROLL_TW;
    constexpr int NBODY = S / CH;
    constexpr int NPRO = (ABL == 0) ? roll_prologue_len(L) : 0; // sub-chunks at the top that run shortened column-pass bodies
    static_assert(S % CH == 0, "slot count must be a multiple of the sub-chunk");
    static_assert(CH == 8 && L % 4 == 1 && L >= ROLL_LMIN && L <= ROLL_LMAX, "roll kernel instance out of range");
    constexpr int SB = roll_sb(L);     // staged bytes per lane per sub-chunk (16 for l = 65)
    constexpr int SEGS = 64 / CH;      // lanes per row
    constexpr int RS = roll_rs(L);     // A row pitch in floats
    constexpr int RPASS = CH / 8;      // row-pass rounds: 8 rows × 8 groups of P = 8 outputs per round

    float *A = reinterpret_cast<float *>(smem);
    f2 *Rb = reinterpret_cast<f2 *>(smem + CH * RS * 4);

    const int lane = threadIdx.x & 63;
    // strips are 64 wide; the last one is shifted left to stay inside the window (overlap
    // recomputes a few columns bit-identically), or is partial when the window is < 64 wide
    const int ncols = g.nthin ? g.thin_x0 : g.n2; // columns covered by 64-wide strips
    const int x0 = (ncols >= TW) ? min(s * TW, ncols - TW) : 0;
    const int ws = min(TW, ncols);
    const int ti0 = g1 - g.r1 - 1 - hw;
    const int wj0 = g2 - g.r2 - 1 - hw; // frame col of the window tile's col 0
    const int tj0 = wj0 + x0;
    const int NA = g.n1 + L - 1;

    // ---- kept range (dog_prune.hpp): the strip's job carries it (never empty: the pre-pass itself leaves the partial and
    // mask 0 of a strip with an empty hull) ----
    const int prune_ba = PRUNE ? job_ba : 0, prune_bb = PRUNE ? job_bb : 0;

    // ---- per-window DC level (see dog_kernels.hpp): same samples in every strip; a job carries the pre-pass's, which is
    // dc_from_sum of the same samples ----
    int dc;
    if constexpr (PRUNE) {
        dc = job_dc;
    } else {
        int sum = dc_sample_sum(g, frame, ti0, wj0, L, lane, 64);
        sum = wave_sum(sum);
        dc = dc_from_sum(sum, g.fill);
    }

    // ---- staging geometry: lane → (row lane / SEGS, SB-byte segment lane % SEGS) ----
    const int srow = lane / SEGS, sseg = lane % SEGS;
    const int scol = tj0 + SB * sseg;            // frame col of this lane's first byte
    const bool cols_in = (scol >= 0) && (scol + SB <= g.fw);
    auto load16 = [&](int a_row, uint32_t (&w)[SB / 4]) {
        const int gi = ti0 + a_row;
        const bool rowok = (a_row < NA) && (gi >= 0) && (gi < g.fh);
        const uint32_t fill4 = (uint32_t)g.fill * 0x01010101u;
#pragma unroll
        for (int q = 0; q < SB / 4; ++q) w[q] = fill4;
        if (rowok) {
            const uint8_t *src = frame + (long long)gi * g.row_stride + scol;
            if (cols_in) {
                __builtin_memcpy(w, src, SB);
            } else {
#pragma unroll
                for (int i = 0; i < SB; ++i) {
                    const int gj = scol + i;
                    if (gj >= 0 && gj < g.fw) {
                        const uint32_t v = src[i];
                        w[i >> 2] = (w[i >> 2] & ~(0xffu << (8 * (i & 3)))) | (v << (8 * (i & 3)));
                    }
                }
            }
        }
    };

    // ---- folded remainder column (LaunchGeo::fold_r): the last strip's row pass also produces window column 64·nstrips.
    // Its last input is strip column TW + L − 1; where the 8·SB staged columns end one short of it (l = 33, 65, 97, 129)
    // the lanes of the last segment stage that one byte more, into the slack of the A row ----
    constexpr bool FOLD_OK = !RESP && ABL == 0 && !PRUNE && roll_folds(L); // (a pruned launch never folds; LaunchGeo::fold_r is its job list)
    constexpr bool FOLD_EXTRA = (8 * SB < TW + L);
    const bool fold = FOLD_OK && g.fold_r != nullptr && s == g.nstrips - 1; // wave-uniform
    const int xcol = tj0 + 8 * SB;                                          // frame col of the extra byte
    // (unconditional load at an address clamped into the frame, validity applied when the byte is used: a load inside a branch
    // is waited for where the branch ends — a full memory latency per sub-chunk in the folding waves)
    const int xcol_c = min(max(xcol, 0), g.fw - 1);
    auto load_extra = [&](int a_row) -> uint32_t {
        const int gi = min(max(ti0 + a_row, 0), g.fh - 1);
        return frame[(long long)gi * g.row_stride + xcol_c];
    };
    auto extra_ok = [&](int a_row) { const int gi = ti0 + a_row; return a_row < NA && gi >= 0 && gi < g.fh && xcol >= 0 && xcol < g.fw; };

    f2 acc2[S / 2];
#pragma unroll
    for (int j = 0; j < S / 2; ++j) acc2[j] = f2{0.f, 0.f};
    float best = -__builtin_huge_valf(), second = -__builtin_huge_valf();
    int best_y = 0;

    const tap_ptr trow = as_taps(taps_row);
    const tap_ptr tcol = as_taps(taps_col);

    unsigned long long stamp_c0 = 0, stamp_r0 = 0;
    if (ABL & 16) { stamp_c0 = __builtin_amdgcn_s_memtime(); stamp_r0 = __builtin_amdgcn_s_memrealtime(); }
    // (Tried: a fast staging path for strips wholly inside the frame — one running pointer per lane instead of load16's row
    // tests, fill pre-load and 64-bit row multiply, ≈10 VALU instructions fewer per sub-chunk: 0.4–0.6 % SLOWER in a three-way
    // same-session comparison.  The kernel does not feel a handful of VALU instructions beside its 900 packed ones.)
    const int nsub = (NA + CH - 1) / CH;
    // ---- padding rows (header comment): the per-sub-chunk test as two wave-uniform sub-chunk numbers — sc holds padding only
    // when sc < pad_top (ti0 + 8·sc + 7 < 0) or sc >= pad_bot (ti0 + 8·sc >= fh); with the row test itself in the loop the
    // folding l = 65 instances spilled 11 VGPRs ----
    const bool pad_ok = (ABL & 15) == 0 && !g.no_pad_skip && __builtin_amdgcn_readfirstlane(dc) == g.fill;
    // (a folding strip also stages frame column tj0 + 8·SB for its ninth output: that column must lie outside as well)
    const bool strip_cols_out = tj0 + 8 * SB + ((FOLD_EXTRA && fold) ? 1 : 0) <= 0 || tj0 >= g.fw;
    const int pad_top = !pad_ok ? 0 : strip_cols_out ? nsub : max(0, -ti0) / CH;
    const int pad_bot = !pad_ok ? nsub : max(0, (g.fh - ti0 + CH - 1) >> 3);
    // a folding strip owes the finishing kernel the R values of its ninth column for EVERY input row: the padding-only
    // sub-chunks' (+0, +0) are stored here, ahead of the loop (inside it the store cost the l = 65 instances 5 VGPRs and spills)
    if (FOLD_OK && fold)
        for (int a = lane; a < NA; a += 64)
            if (a < pad_top * CH || a >= pad_bot * CH) g.fold_r[(long long)b * NA + a] = f2{0.f, 0.f};
    // ---- kept range (dog_prune.hpp): two more wave-uniform sub-chunk numbers.  The loop runs over the sub-chunks
    // [sc_lo, sc_hi) that hold the input rows of the kept output blocks.  Outputs above row y_lo = 8·sc_lo lack their first
    // terms and are not fed to the peak; every output from y_lo on that the loop emits is complete (its last input row,
    // y + l − 1, lies in the sub-chunk that emits it), so the few rows it may emit past the range's end are the window's own
    // values and harmless.  Starting late needs no reset (every output's first term is a multiply).
    // BODIES THAT MATCH THE RANGE'S START.  A PRUNE instance numbers its sub-chunks from sc_lo on (`rel`): the phase, the
    // prologue switch, the slot rotation of the emit part and roll_col_zero all take the relative number, so output y sits in
    // slot (y − y_lo) mod S and the first sub-chunks of EVERY kept range run the shortened prologue bodies — in sub-chunk
    // sc_lo + j only tap blocks 0 … 2j + 1 feed outputs at or below y_lo, the rest would scatter into slots whose outputs are
    // withheld from the peak anyway (the triangle the prologue bodies leave out at a window's top; roll_start_covers above
    // checks the blocks for every length).  The bits do not change: every output from y_lo on still receives its terms
    // t = 0, 1, … in order, in another register.  ybase, pad_sc, the staging rows and the counts keep the absolute number.
    // BODIES THAT MATCH THE RANGE'S END (dog_roll_range.hpp).  The last output the loop emits is y_end = min(8·sc_hi − l, n1 − 1)
    // and no slot is read after it, so in sub-chunk sc only the taps t ≥ 8·sc − y_end + i of row i have an emitted output to
    // feed: the column-pass bodies of a PRUNE instance — the NBODY full ones and the shortened prologue bodies, which a short
    // range meets in the same sub-chunks — are entered at the wave-uniform run-time block roll_end_qlo(8·sc − y_end), rounded
    // down to the entry step (roll_end_entry; roll_col_body, ENTRY): most of the triangle the height-class instances leave
    // out statically at a window's bottom (at l = 17 and 21 the step leaves a range inside the window nothing to skip).  The dead blocks are those of the last
    // ⌊(l − 3) / 8⌋ sub-chunks of every range, and more of one that the window's bottom cuts off.  The bits do not
    // change: every emitted output still receives all its terms in order (roll_end_covers, asserted per length above;
    // tests/range_end_main.cpp counts the pairs one by one), the rows past 8·bb the loop emits included; the slots that lose
    // terms — or their restarting multiply, with block 0 — belong to outputs past y_end.  Padding-only sub-chunks
    // (roll_col_zero) have nothing to skip.  pdog_set_tuning "no_range_end" pins qlo = 0 through y_end (LaunchGeo::prune). ----
    static_assert(!PRUNE || (!RESP && ABL == 0 && EPI < 0), "kept ranges: the plain instances only");
    int sc_lo = 0, sc_hi = nsub, y_lo = 0, y_end = 0;
    if constexpr (PRUNE) {
        sc_lo = prune_ba;
        sc_hi = prune_sc_hi(prune_ba, prune_bb, L, nsub);
        y_lo = prune_ba * CH;
        y_end = (g.prune & PRUNE_NO_RANGE_END) ? CH * nsub : roll_end_y(sc_hi, L, g.n1); // (8·nsub: tm ≤ 0 for every sub-chunk)
    }
    uint32_t pre[SB / 4];
    load16(sc_lo * CH + srow, pre);
    uint32_t pre_x = 0;
    if (FOLD_EXTRA && fold) pre_x = load_extra(sc_lo * CH + srow);
    const int rr = lane & 7, rgx = lane >> 3; // row-pass task: row rr, output group rgx
    const long long resp_base = (long long)b * g.n1 * g.n2;

    for (int sc = sc_lo; sc < sc_hi; ++sc) {
        // padding rows (see above): all 8 rows outside the frame, or a strip whose staged columns all are — wave-uniform
        const bool pad_sc = sc < pad_top || sc >= pad_bot;
        // ---- stage this sub-chunk from the prefetched registers, request the next ----
        if (!(ABL & 4)) {
            if (!pad_sc) {
                float *dst = A + roll_row_base(srow, L) + SB * sseg; // 16-byte aligned: ds_write_b128
                const f2 ndc = f2{-(float)dc, -(float)dc};
#pragma unroll
                for (int q = 0; q < SB / 4; ++q) { // two pixels per v_pk_add_f32 (v_cvt_f32_ubyteN each): exact integers either way
                    const uint32_t word = pre[q];
                    const f2 v01 = f2{(float)(word & 0xffu), (float)((word >> 8) & 0xffu)} + ndc;
                    const f2 v23 = f2{(float)((word >> 16) & 0xffu), (float)(word >> 24)} + ndc;
                    *reinterpret_cast<f4 *>(dst + 4 * q) = f4{v01.x, v01.y, v23.x, v23.y};
                }
                if (FOLD_EXTRA && fold && sseg == SEGS - 1)
                    A[roll_row_base(srow, L) + 8 * SB] = (float)(extra_ok(sc * CH + srow) ? (int)pre_x : g.fill) - (float)dc;
            }
            if (!(ABL & 8)) { // (also from a padding-only sub-chunk: the next one may be real)
                load16((sc + 1) * CH + srow, pre);
                if (FOLD_EXTRA && fold) pre_x = load_extra((sc + 1) * CH + srow);
            }
        }
        f2 rv[CH];
        if (!pad_sc) { // (a padding-only sub-chunk touches no LDS)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier(); // the LDS traffic is wave-private: the fences' waits are all the ordering needed
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // ---- row pass: rounds of 8 rows × 8 groups of 8 outputs ----
            if (!(ABL & 2)) {
                static_assert(RPASS == 1, "one row-pass round per sub-chunk");
                const float *arow = A + roll_row_base(rr, L) + rgx * P;
                f2 *dst = Rb + rr * ROLL_PR + rgx * P;
                if (FOLD_OK && fold) {
                    f2 racc[P + 2];
#pragma unroll
                    for (int o = 0; o < P + 2; ++o) racc[o] = f2{0.f, 0.f};
                    roll_row_pass<L, P + 1>(racc, arow, trow);
#pragma unroll
                    for (int o = 0; o < P; ++o) dst[o] = racc[o];
                    // the last lane group's ninth output is window column 64·nstrips of input row sc·8 + rr
                    if (rgx == TW / P - 1 && sc * CH + rr < NA) g.fold_r[(long long)b * NA + sc * CH + rr] = racc[P];
                } else {
                    f2 racc[P];
#pragma unroll
                    for (int o = 0; o < P; ++o) racc[o] = f2{0.f, 0.f};
                    roll_row_pass<L>(racc, arow, trow);
#pragma unroll
                    for (int o = 0; o < P; ++o) dst[o] = racc[o];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // ---- column pass: 8 new R rows into the rolling accumulators ----
#pragma unroll
            for (int i = 0; i < CH; ++i) rv[i] = Rb[i * ROLL_PR + lane];
        }
        const int rel = PRUNE ? sc - sc_lo : sc; // the number that picks the body (kept ranges: above)
        const int phase = rel % NBODY;
        const int sc_e = roll_epi_c0(g.n1) / 2 + 1; // first sub-chunk whose rows need no tap of the first block(s)
        auto emit = [&](auto SCc, auto QHIc, auto QLOc) {
            constexpr int SC = decltype(SCc)::value, QHI = decltype(QHIc)::value, QLO = decltype(QLOc)::value;
            if (pad_sc) roll_col_zero<L, SC>(acc2); // (harmless in a shortened body: the slots it resets there have no output)
            else if (!(ABL & 1)) roll_col_body<L, SC, QHI, QLO, PRUNE>(acc2, rv, tcol, PRUNE ? roll_end_entry(roll_end_qlo(roll_end_tm(sc, y_end)), L) : 0);
            // outputs y = a − (l−1) for the 8 rows of this sub-chunk are complete.  A lane owns ONE
            // column and meets its rows in increasing y (= increasing column-major index), so a strict
            // '>' keeps the first maximum of the lane (findmax, :59); ties between lanes and strips
            // are settled by index in the reductions.  Column validity is applied once at the end.
            const int ybase = sc * CH - (L - 1);
            if (ybase + CH > y_lo && ybase < g.n1) { // (y_lo = 0 unless a kept range says otherwise)
                const bool full = (ybase >= y_lo) && (ybase + CH <= g.n1); // wave-uniform
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int slot = ((CH * SC + i - (L - 1)) % S + S) % S;
                    const float v = (slot & 1) ? acc2[slot / 2].y : acc2[slot / 2].x;
                    const bool rowok = full || ((ybase + i >= y_lo) && (ybase + i < g.n1));
                    if (RESP && rowok && lane < ws) g.resp[resp_base + (long long)(x0 + lane) * g.n1 + ybase + i] = v;
                    if (rowok) {
                        second = __builtin_amdgcn_fmed3f(v, best, second); // runner-up of the lane's column (exact mode)
                        if (v > best) { best = v; best_y = ybase + i; }
                    }
                }
            }
            // (no reset: the emitted slots are reused S rows later, and their first term is a multiply, see roll_col_body)
        };
        static_assert(NBODY <= 20 && NPRO < NBODY && NPRO <= 20, "extend the phase switches");
#define PDOG_FULL(k) case k: emit(std::integral_constant<int, (k) % NBODY>{}, std::integral_constant<int, roll_col_blocks(L)>{}, std::integral_constant<int, 0>{}); break;
#define PDOG_PRO(k)                                                                                                   \
    case k:                                                                                                           \
        if constexpr ((k) < NPRO) emit(std::integral_constant<int, (k) % NBODY>{}, std::integral_constant<int, ((k) < NPRO ? roll_prologue_blocks(k) : 1)>{}, std::integral_constant<int, 0>{}); \
        break;
        if (EPI >= 0 && sc >= sc_e) { // the last rows of a window of this height class: shortened bodies
            if constexpr (EPI >= 0) {
                // first epilogue sub-chunk sc_e = c0 ÷ 2 + 1: phase (EPI ÷ 2 + 1) mod NBODY (even class) …, qlo = 2 − (c0 mod 2), +2 per sub-chunk
                constexpr int PH0 = (EPI / 2 + 1) % NBODY, Q0 = 2 - (EPI & 1);
#define PDOG_EPI(e)                                                                                                          \
    case e:                                                                                                                  \
        if constexpr (Q0 + 2 * (e) < roll_col_blocks(L))                                                                     \
            emit(std::integral_constant<int, (PH0 + (e)) % NBODY>{}, std::integral_constant<int, roll_col_blocks(L)>{},      \
                 std::integral_constant<int, (Q0 + 2 * (e) < roll_col_blocks(L) ? Q0 + 2 * (e) : 0)>{});                     \
        break;
                switch (sc - sc_e) {
                    PDOG_EPI(0) PDOG_EPI(1) PDOG_EPI(2) PDOG_EPI(3) PDOG_EPI(4) PDOG_EPI(5) PDOG_EPI(6) PDOG_EPI(7)
                    PDOG_EPI(8) PDOG_EPI(9) PDOG_EPI(10) PDOG_EPI(11) PDOG_EPI(12) PDOG_EPI(13)
                default: break;
                }
#undef PDOG_EPI
            }
        } else if (rel < NPRO) { // the first rows: shortened bodies (sub-chunk = phase)
            switch (rel) {
                PDOG_PRO(0) PDOG_PRO(1) PDOG_PRO(2) PDOG_PRO(3) PDOG_PRO(4) PDOG_PRO(5) PDOG_PRO(6) PDOG_PRO(7)
                PDOG_PRO(8) PDOG_PRO(9) PDOG_PRO(10) PDOG_PRO(11) PDOG_PRO(12) PDOG_PRO(13) PDOG_PRO(14) PDOG_PRO(15)
                PDOG_PRO(16) PDOG_PRO(17) PDOG_PRO(18) PDOG_PRO(19)
            default: break;
            }
        } else {
            switch (phase) {
                PDOG_FULL(0) PDOG_FULL(1) PDOG_FULL(2) PDOG_FULL(3) PDOG_FULL(4) PDOG_FULL(5) PDOG_FULL(6) PDOG_FULL(7)
                PDOG_FULL(8) PDOG_FULL(9) PDOG_FULL(10) PDOG_FULL(11) PDOG_FULL(12) PDOG_FULL(13) PDOG_FULL(14) PDOG_FULL(15)
                PDOG_FULL(16) PDOG_FULL(17) PDOG_FULL(18)
            default: emit(std::integral_constant<int, 19 % NBODY>{}, std::integral_constant<int, roll_col_blocks(L)>{}, std::integral_constant<int, 0>{}); break;
            }
        }
#undef PDOG_FULL
#undef PDOG_PRO
        __builtin_amdgcn_wave_barrier(); // A / Rb are rewritten by the next sub-chunk
    }

    if (ABL & 16) { // diagnostic build only: shader cycles and 100 MHz ticks of the main loop, per wave
        const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if (lane == 0 && g.resp) { g.resp[2 * logical] = (float)(c1 - stamp_c0); g.resp[2 * logical + 1] = (float)(r1 - stamp_r0); }
    }
    Peak pk;
    pk.best = best;
    pk.second = second;
    pk.idx = (x0 + lane) * g.n1 + best_y;
    const bool skipped = sc_lo >= sc_hi; // an empty kept range: the partial is an initialised Peak and mask 0
    if (lane >= ws || skipped) peak_init(pk);
    const float colbest = pk.best;
    peak_wave_reduce(pk);
    peak_out = pk;         // valid in lane 0
    // exact mode: which columns of the strip can hold a pixel within T of the window's maximum (≥ the strip's): the
    // refinement rescans only those
    const float sb = __shfl(pk.best, 0, 64);
    mask_out = skipped ? 0ull : __builtin_amdgcn_ballot_w64(colbest >= sb - g.ex.T);
}


// The strip as an out-of-line function with a register allocation of its own.  The persistent chain kernel calls it
// (inlined into that kernel's frame loop the accumulators, the row-pass windows and the loop state did not fit:
// 18–64 VGPRs went to scratch inside the hot loop, and the l = 105 instance returned wrong rows in round 1 while
// the batch kernel of the same length, compiled separately, was correct).  Arguments arrive in VGPRs by the calling
// convention: everything uniform goes back to SGPRs with readfirstlane (tap tables are read with scalar loads).
__device__ __forceinline__ unsigned long long uniform_u64(const void *p)
{
    const unsigned long long u = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
template <int LT>
__device__ __attribute__((noinline)) void roll_strip_call(const LaunchGeo *gp, const f2 *taps_row, const f2 *taps_col, unsigned char *smem,
                                                          const uint8_t *frame, int g1, int g2, int s, int b, Peak *out, unsigned long long *mask)
{
    LaunchGeo g;
    __builtin_memcpy(&g, (const void *)uniform_u64(gp), sizeof g);
    Peak pk;
    unsigned long long m;
    roll_strip<LT, false, 0>(g, (const f2 *)uniform_u64(taps_row), (const f2 *)uniform_u64(taps_col), smem, (const uint8_t *)uniform_u64(frame),
                             __builtin_amdgcn_readfirstlane(g1), __builtin_amdgcn_readfirstlane(g2), __builtin_amdgcn_readfirstlane(s),
                             __builtin_amdgcn_readfirstlane(b), 0, pk, m);
    *out = pk;
    *mask = m;
}

// One strip per workgroup (one wave).  Tried in round 3: up to four strips of ONE window per workgroup, a wave each (still no
// barrier), so that the strips of a window — which read each other's halo columns — run on one CU at one time.  The HBM
// traffic did not move (553.6 vs 557.6 MB per cfg3 step: the 1.31× over the algorithmic bytes is the fetch granularity on
// unaligned 321-byte rows, not re-fetched halos) and cfg3 ran 2 % slower (cfg4 0.6 % faster): dropped.
template <int LT, bool RESP, int ABL = 0, int EPI = -1, bool PRUNE = false>
__global__ __launch_bounds__(64, roll_waves(LT)) void dog_roll_kernel(const LaunchGeo g, const f2 *__restrict__ taps_row,
                                                                      const f2 *__restrict__ taps_col)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int logical, b, s, ba = 0, bb = 0, dc = 0;
    if constexpr (PRUNE) {
        // THE JOB LIST (dog_prune.hpp): the workgroup takes one kept strip of the pre-pass's list.  The grid is the host's
        // upper bound; the workgroups past the list's end return, and they all sit at the END of the grid — the kept waves,
        // all of nearly one length, start back to back and fill the SIMDs, where one wave per (window, strip) in index
        // order interleaved them with as many waves that returned at once.  Results go to [b][s] whatever the list's order.
        logical = prune_job_index((int)blockIdx.x, g.prune & PRUNE_GROUP_MASK);
        const int count = min(g.jobs[0].b, g.nblocks);
        if (logical >= count) return;
        const PruneJob job = g.jobs[1 + logical];
        b = job.b;
        s = job.s_dc & 0xffff;
        dc = (job.s_dc >> 16) & 0xff;
        ba = job.ba;
        bb = job.bb;
    } else {
        // XCD-aware block → (window, strip), see dog_kernels.hpp
        const int per_xcd = (g.nblocks + 7) >> 3;
        logical = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
        if (logical >= g.nblocks) return;
        b = logical / g.nstrips;
        s = logical - b * g.nstrips;
    }
    const int g1 = g.guesses[2 * b], g2 = g.guesses[2 * b + 1];
    const int fidx = g.frame_index ? g.frame_index[b] : b;
    const uint8_t *__restrict__ frame = g.frames + (long long)fidx * g.frame_stride;
    Peak pk;
    unsigned long long mask;
    roll_strip<LT, RESP, ABL, EPI, PRUNE>(g, taps_row, taps_col, smem, frame, g1, g2, s, b, logical, pk, mask, ba, bb, dc);
    if (threadIdx.x == 0) {
        g.part_mask[b * g.nslots + s] = mask;
        g.part_val[b * g.nslots + s] = pk.best;
        g.part_idx[b * g.nslots + s] = pk.idx;
        g.part_sec[b * g.nslots + s] = pk.second;
    }
}

// ---- persistent serial chain (src/PawsomeTracker.jl:163-169, the intended loop :167) ----
// One workgroup per clip, one wave per strip of the search window; the workgroup walks the clip's frames,
// each frame searched around the previous frame's clamped answer, with no host round trip and no launch
// per frame.  Strips meet through 2 LDS words per wave and one workgroup barrier per frame.  Thin remainder
// columns are not used here: the last strip overlaps instead (bit-identical values either way).
struct ChainGeo {
    LaunchGeo g;                         // frames = first frame of clip 0; guesses/frame_index unused
    const RefineParams *rp;              // exact mode's constants in device memory (dog_exact.hpp); null = off
    int ref_cbw, ref_rows;               // refinement inside the kernel: window columns per block; tile rows resident at a time (the strips' LDS is its scratch)
    const f2 *taps_col_plain;            // (s·g₊[k], −s·g₋[k]) per tap: the refinement's column taps (taps_col is the roll kernel's paired table)
    const int *__restrict__ start;       // n_clips x 2, 1-based (row, col)
    int *__restrict__ out_ij;            // n_clips x n_frames x 2
    int n_frames;                        // per clip; clip c's frame k is frame c*n_frames + k
};
// A frame table for the kernels that walk a clip themselves (pdog_detect_chains_indexed): step k of clip c looks at frame
// index[c*n_steps + k] of ONE stack, for k < len[c] — checked on the host before the launch, so every entry a kernel reads
// names a frame of the stack.  Every workgroup (wave) of a clip reads the same len[c] and leaves the frame loop with the others.
struct ClipTable {
    const int32_t *index; // [n_clips][n_steps]
    const int32_t *len;   // [n_clips] steps of each clip: the count of its row's leading non-negative entries
    int first;            // 1: row 0 of a clip that has one receives its start guess as given, the loop begins at step 1 (:104, :161)
};
struct ChainTableGeo : ChainGeo { ClipTable tab; };
// The predicted chain (include/pawsome_predict.h): what the lane that files a clip's positions needs beside the table.
struct PredictCtl {
    float m;            // (float)min_response: a frame whose FP32 maximum does not exceed it is HELD
    int coast;          // held steps a clip keeps its velocity for
    int32_t *out_state; // [n_clips][n_steps]: 1 assigned, -1 held (0: the start filed as given, first = 1)
    int32_t *mstate;    // [n_clips][4] in (v_row, v_col, n_held, -), out after a clip's last step (word 3 = 0); null: at rest, dropped
};
struct ChainPredictGeo : ChainTableGeo { PredictCtl pred; };
template <bool TABLE, bool PRED>
using chain_geo_t = std::conditional_t<PRED, ChainPredictGeo, std::conditional_t<TABLE, ChainTableGeo, ChainGeo>>;
// TABLE: the instances that walk a frame table.  A template flag and a kernel argument of their own, not a run-time branch
// on a wider ChainGeo: the existing instances compile exactly as before (the branch cost them SGPR spills, the wider
// argument 16 bytes of scratch).
// PRED: the TABLE instances of the predicted chain — again a flag and an argument of their own.  Thread 0, which files the
// position, carries the clip's p, v and n_held in LDS beside `cur` and applies pdog_predict.hpp's step: `cur` is then the
// PREDICTION the next window is centred on.  A held frame's position is not used, so a held frame is never refined and
// g.ex.stat does not count it.
template <int LT, bool TABLE = false, bool PRED = false>
__global__ __launch_bounds__(512) void dog_chain_kernel(const chain_geo_t<TABLE, PRED> cg,
                                                        const f2 *__restrict__ taps_row, const f2 *__restrict__ taps_col)
{
    static_assert(TABLE || !PRED, "the predicted chain walks a frame table");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int cur[2];
    __shared__ float pv[8], ps[8];
    __shared__ int pi[8];
    __shared__ unsigned long long pm[8];
    __shared__ int s_refine;
    __shared__ float s_max, s_sec2;
    __shared__ int s_idx2;
    const LaunchGeo &g = cg.g;
    const int tid = threadIdx.x, wave = tid >> 6, nst = blockDim.x >> 6;
    const int c_ = blockIdx.x;
    const int32_t *table = nullptr;
    int len = 0, k_first = 0;
    if constexpr (TABLE) {
        table = cg.tab.index + (long long)c_ * cg.n_frames;
        len = cg.tab.len[c_];
        k_first = cg.tab.first;
    }
    int *walk = nullptr; // PRED, thread 0 only: p (2), v (2), n_held
    if constexpr (PRED) {
        __shared__ int s_walk[5];
        walk = s_walk;
    }
    // PRED, thread 0: one step of the rule on the frame at prediction (ci, cj) — files position and state, after the clip's
    // last step the state it ends in, and makes the next prediction the current guess
    auto file_predicted = [&](int k, bool hit, int ci, int cj, int qi, int qj) {
        if constexpr (PRED) {
            predict::Walk w{walk[0], walk[1], {walk[2], walk[3], walk[4]}};
            const predict::Filed f = predict::step(w, hit, ci, cj, qi, qj, cg.pred.coast, g.fh, g.fw);
            const long long o = (long long)c_ * cg.n_frames + k;
            cg.out_ij[2 * o] = f.i; cg.out_ij[2 * o + 1] = f.j;
            cg.pred.out_state[o] = f.state;
            cur[0] = f.gi; cur[1] = f.gj;
            walk[0] = w.pi; walk[1] = w.pj; walk[2] = w.c.vi; walk[3] = w.c.vj; walk[4] = w.c.n_held;
            if (k == len - 1 && cg.pred.mstate) {
                int32_t *ms = cg.pred.mstate + 4 * (long long)c_;
                ms[0] = w.c.vi; ms[1] = w.c.vj; ms[2] = w.c.n_held; ms[3] = 0;
            }
        }
    };
    if constexpr (PRED) {
        if (tid == 0) {
            const int si = cg.start[2 * c_], sj = cg.start[2 * c_ + 1];
            const int32_t *ms = cg.pred.mstate ? cg.pred.mstate + 4 * (long long)c_ : nullptr;
            walk[0] = si; walk[1] = sj;
            walk[2] = ms ? ms[0] : 0; walk[3] = ms ? ms[1] : 0; walk[4] = ms ? ms[2] : 0;
            cur[0] = predict::predict(si, walk[2], g.fh); // the first window is centred on clamp(start + v)
            cur[1] = predict::predict(sj, walk[3], g.fw);
            if (len > k_first) range_check(g.ex, cur[0], cur[1], LT / 2, g.fh, g.fw);
            if (k_first && len >= 1) { // the start, stored as given, with state 0
                cg.out_ij[2 * (long long)c_ * cg.n_frames] = si;
                cg.out_ij[2 * (long long)c_ * cg.n_frames + 1] = sj;
                cg.pred.out_state[(long long)c_ * cg.n_frames] = 0;
            }
        }
    } else if (tid == 0) {
        cur[0] = cg.start[2 * c_];
        cur[1] = cg.start[2 * c_ + 1];
        if (!TABLE || len > k_first) range_check(g.ex, cur[0], cur[1], LT / 2, g.fh, g.fw); // (a start that no step uses raises nothing)
        if (k_first && len >= 1) { // the bootstrap's position, stored as given (:161)
            cg.out_ij[2 * (long long)c_ * cg.n_frames] = cur[0];
            cg.out_ij[2 * (long long)c_ * cg.n_frames + 1] = cur[1];
        }
    }
    __syncthreads();
    for (int k = k_first; k < (TABLE ? len : cg.n_frames); ++k) { // (len: TABLE instances only — the plain ones read cg.n_frames where they did)
        const int g1 = cur[0], g2 = cur[1];
        const long long fidx = TABLE ? (long long)table[k] : (long long)c_ * cg.n_frames + k;
        const uint8_t *__restrict__ frame = g.frames + fidx * g.frame_stride;
        Peak pk;
        unsigned long long mask;
        roll_strip_call<LT>(&g, taps_row, taps_col, smem + wave * roll_lds_bytes(LT), frame, g1, g2, wave, 0, &pk, &mask);
        if ((tid & 63) == 0) { pv[wave] = pk.best; pi[wave] = pk.idx; ps[wave] = pk.second; pm[wave] = mask; }
        __syncthreads();
        if (tid == 0) {
            Peak w;
            peak_init(w);
            for (int q = 0; q < nst; ++q) peak_merge(w, pv[q], pi[q], ps[q]);
            const int x = w.idx / g.n1, y = w.idx - x * g.n1;
            const int i = min(max(g1 - g.r1 + y, 1), g.fh);   // :60-61
            const int j = min(max(g2 - g.r2 + x, 1), g.fw);
            if constexpr (PRED) {
                const bool hit = predict::assigned(w.best, cg.pred.m);
                s_refine = hit && cg.rp && (w.best - w.second <= g.ex.T);
                if (!s_refine) file_predicted(k, hit, g1, g2, i, j); // (a near-tie is filed once the refinement has decided)
            } else {
                int *o = cg.out_ij + 2 * ((long long)c_ * cg.n_frames + k);
                o[0] = i; o[1] = j;
                cur[0] = i; cur[1] = j;
                s_refine = cg.rp && (w.best - w.second <= g.ex.T);
            }
            s_max = w.best;
            s_sec2 = w.second;
            s_idx2 = w.idx;
            if (s_refine) atomicAdd(g.ex.stat, 1ull);
        }
        __syncthreads();
        if (s_refine) {
            // near-tie: the chain cannot go on before the reference's own arithmetic has decided (dog_exact.hpp);
            // the strips' LDS is free between frames and is the refinement's scratch
            RefineCtx c;
            c.trow = as_taps(taps_row);
            c.tcol = as_taps(cg.taps_col_plain);
            const refine_params_ptr rp = (refine_params_ptr)(unsigned long long)cg.rp;
            c.K = (k64_ptr)(unsigned long long)rp->K64;
            c.g64 = (k64_ptr)(unsigned long long)rp->g64;
            c.dir = rp->dir;
            c.T64 = rp->T64;
            c.T = g.ex.T;
            c.T_rescan = g.ex.T_rescan;
            c.second = s_sec2;
            c.fp32_idx = s_idx2;
            c.cbw = cg.ref_cbw;
            c.tile_rows = cg.ref_rows;
            c.lds = smem;
            auto may = [&](int x0, int x1, float thr) { // strip s covers 64 columns from min(64 s, n2 − 64) (one partial strip when n2 < 64)
                bool any = false;
                for (int q = 0; q < nst; ++q) {
                    const int lo = g.n2 >= ROLL_TW ? min(q * ROLL_TW, g.n2 - ROLL_TW) : 0, hi = lo + ROLL_TW;
                    if (lo < x1 && hi > x0 && pv[q] >= thr && (pm[q] & column_bits(x0 - lo, x1 - lo))) any = true;
                }
                return any;
            };
            const int idx = refine_window<8>(blockDim.x, g, frame, g1, g2, s_max, c, may);
            if (tid == 0) {
                const int x = idx / g.n1, y = idx - x * g.n1;
                const int i = min(max(g1 - g.r1 + y, 1), g.fh);
                const int j = min(max(g2 - g.r2 + x, 1), g.fw);
                if constexpr (PRED) {
                    file_predicted(k, true, g1, g2, i, j);
                } else {
                    int *o = cg.out_ij + 2 * ((long long)c_ * cg.n_frames + k);
                    o[0] = i; o[1] = j;
                    cur[0] = i; cur[1] = j;
                }
            }
            __syncthreads();
        }
    }
}

#ifndef PDOG_ROLL_INST_ONLY
// Chains over a frame table run as ordinary batches (pdog_detect_chains_indexed; the step between two batches is
// dog_step.hpp's): clip c has len[c] steps.
// Before the first step: a clip with a step to compute starts from its start guess, any other from (1, 1) — its window is
// still part of every batch, its result is never stored, and a start that no step uses must raise nothing; with first = 1
// row 0 of a clip that has one receives the start as given (src/PawsomeTracker.jl:104, :161).
static __global__ void dog_chain_table_init_kernel(const int *__restrict__ start, const int *__restrict__ len, int *__restrict__ cur,
                                                   int *__restrict__ out_ij, int n_clips, int n_steps, int first)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_clips) return;
    const int i = start[2 * c], j = start[2 * c + 1], n = len[c];
    cur[2 * c] = n > first ? i : 1;
    cur[2 * c + 1] = n > first ? j : 1;
    if (first && n >= 1) {
        out_ij[2 * (long long)c * n_steps] = i;
        out_ij[2 * (long long)c * n_steps + 1] = j;
    }
}

#endif // PDOG_ROLL_INST_ONLY

// (dynamic LDS of dog_thin_kernel: thin_lds_bytes, dog_layout.hpp)
static_assert(sizeof(f2) == 8, "thin_lds_bytes counts the R column's f2 elements as 8 bytes");

// ---- thin remainder ----
// A window whose width is 64·k + r with small r (257 = 4·64 + 1) would need a whole extra strip for
// r columns.  Instead those columns are done here, one 256-thread workgroup per (window, column):
// thread = input row for the row pass (l contiguous pixels, symmetric taps), then thread = output row
// for the column pass over the R column in LDS.  The arithmetic replays dog_roll_kernel's operation
// order exactly (row: k ascending pairs then centre, both Gaussians per v_pk_fma_f32; column: per tap
// t ascending, the g+ term then the g− term into one f32), so a pixel computed here is bit-identical
// to what a strip would have produced and flat windows still tie exactly.
template <int LT, bool RESP>
__global__ __launch_bounds__(256) void dog_thin_kernel(const LaunchGeo g, const f2 *__restrict__ taps_row,
                                                       const f2 *__restrict__ taps_col)
{
    constexpr int L = LT, hw = L / 2, H = L / 2, NT = 256, NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f2 *Rc = reinterpret_cast<f2 *>(smem);            // NA entries
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware block → (window, column) like the strips (dog_kernels.hpp): the kernel runs BESIDE the roll kernel, and a
    // window's remainder column then meets its strips in one L2 — the patch it reads is the last strip's
    const int nb = g.n * g.nthin, per_xcd = (nb + 7) >> 3;
    const int logical = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (logical >= nb) return;
    const int b = logical / g.nthin;
    const int rc = logical - b * g.nthin;
    const int x = g.thin_x0 + rc;                     // window column
    const int g1 = g.guesses[2 * b], g2 = g.guesses[2 * b + 1];
    const int fidx = g.frame_index ? g.frame_index[b] : b;
    const uint8_t *__restrict__ frame = g.frames + (long long)fidx * g.frame_stride;
    const int ti0 = g1 - g.r1 - 1 - hw;
    const int wj0 = g2 - g.r2 - 1 - hw;
    const int NA = g.n1 + L - 1;
    const tap_ptr trow = as_taps(taps_row);
    const tap_ptr tcol = as_taps(taps_col);

    __shared__ int ssum[NW];
    __shared__ float sval[NW], ssec[NW];
    __shared__ int sidx[NW];
    // ---- kept range (dog_prune.hpp), read ahead of the DC level: output rows [y_lo, y_hi) and the input rows [a_lo, a_hi)
    // they read; an empty range (the same for the whole workgroup) leaves an initialised Peak at once ----
    int a_lo = 0, a_hi = NA, y_lo = 0, y_hi = g.n1;
    int dc = 0;
    const bool pruned = !RESP && g.prune;
    if (pruned) {
        const unsigned long long rng = g.part_mask[(long long)b * g.nslots + g.nstrips + rc];
        const int ba = (int)((unsigned)rng & 0xffffffu), bb = (int)(unsigned)(rng >> 32);
        dc = (int)(((unsigned)rng >> 24) & 0xffu); // the pre-pass's dc_from_sum of the same samples: no sampling here
        if (bb <= ba) {
            if (tid == 0) {
                Peak pk;
                peak_init(pk);
                g.part_val[b * g.nslots + g.nstrips + rc] = pk.best;
                g.part_idx[b * g.nslots + g.nstrips + rc] = pk.idx;
                g.part_sec[b * g.nslots + g.nstrips + rc] = pk.second;
            }
            return;
        }
        y_lo = ba * ROLL_CH;
        y_hi = min(g.n1, bb * ROLL_CH);
        a_lo = y_lo;
        a_hi = y_hi + L - 1;
    }
    if (!pruned) {
        int sum = dc_sample_sum(g, frame, ti0, wj0, L, tid, NT);
        sum = wave_sum(sum);
        if (lane == 0) ssum[wave] = sum;
        __syncthreads();
        int tot = 0;
        for (int w = 0; w < NW; ++w) tot += ssum[w];
        dc = dc_from_sum(tot, g.fill);
    }
    const float fdc = (float)dc;
    const int na = a_hi - a_lo; // input rows to stage

    // ---- the column's input patch, NA rows × l pixels, → LDS bytes: a dword per item, loaded unconditionally at an
    // address clamped into the frame (a clamped dword still holds every in-frame byte its item needs, at a shifted
    // position), PaddedView fill (:48) selected afterwards — coalesced along the rows, no per-pixel branches (the old
    // row pass read its own row straight from memory, 64 cache lines per load instruction, and its border path spilled
    // 360 SGPRs) ----
    constexpr int TP = (L + 3) / 4 * 4, TQ = TP / 4;  // tile pitch in bytes / dwords
    uint8_t *tile = smem + ((size_t)NA * sizeof(f2) + 15) / 16 * 16;
    const int gj0 = wj0 + x; // frame col of input k = 0
    if (ti0 >= 0 && ti0 + NA <= g.fh && gj0 >= 0 && gj0 + TP <= g.fw) { // the whole patch inside the frame (workgroup-uniform): a plain copy
#pragma unroll 4
        for (int e = tid; e < na * TQ; e += NT) {
            const int a = a_lo + e / TQ, q = e - (a - a_lo) * TQ;
            uint32_t w;
            __builtin_memcpy(&w, frame + (long long)(ti0 + a) * g.row_stride + gj0 + 4 * q, 4);
            *reinterpret_cast<uint32_t *>(tile + a * TP + 4 * q) = w;
        }
    } else if (g.fw >= 4) {
#pragma unroll 4
        for (int e = tid; e < na * TQ; e += NT) {
            const int a = a_lo + e / TQ, q = e - (a - a_lo) * TQ;
            const int gi = ti0 + a, gj = gj0 + 4 * q;
            const int gjc = min(max(gj, 0), g.fw - 4);
            uint32_t w;
            __builtin_memcpy(&w, frame + (long long)min(max(gi, 0), g.fh - 1) * g.row_stride + gjc, 4);
            const bool rowok = gi >= 0 && gi < g.fh;
            uint32_t o = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int gjj = gj + i;
                const uint32_t px = (rowok && gjj >= 0 && gjj < g.fw) ? ((w >> (8 * ((gjj - gjc) & 3))) & 0xffu) : (uint32_t)g.fill;
                o |= px << (8 * i);
            }
            *reinterpret_cast<uint32_t *>(tile + a * TP + 4 * q) = o;
        }
    } else {
        for (int e = tid; e < na * TP; e += NT) {
            const int a = a_lo + e / TP, cc = e - (a - a_lo) * TP;
            const int gi = ti0 + a, gj = gj0 + cc;
            tile[a * TP + cc] = (gi >= 0 && gi < g.fh && gj >= 0 && gj < g.fw) ? frame[(long long)gi * g.row_stride + gj] : (uint8_t)g.fill;
        }
    }
    __syncthreads();
    // ---- row pass: R[a] for input rows a = tid, tid + 256, … (same operation order as the strips: pairs k ascending, centre last) ----
    for (int a = a_lo + tid; a < a_hi; a += NT) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(tile + a * TP);
        float v[L];
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
            const uint32_t w = src[q];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * q + i < L) v[4 * q + i] = (float)((w >> (8 * i)) & 0xffu) - fdc;
        }
        f2 acc = f2{0.f, 0.f};
        tap_ptr tb = trow;
#pragma unroll
        for (int k0 = 0; k0 < H; k0 += 8) { // taps in blocks of 8 behind a base pointer re-pinned per block (not hoisted out of the row loop)
            tb = pin_taps(tb);
#pragma unroll
            for (int k = k0; k < k0 + 8; ++k)
                if (k < H) acc = fma_bcast(v[k] + v[L - 1 - k], tb[k], acc);
        }
        tb = pin_taps(tb);
        acc = fma_bcast(v[H], tb[H], acc);
        Rc[a] = acc;
    }
    __syncthreads();
    // ---- column pass + argmax: outputs y = tid, tid + 256, … ----
    Peak pk;
    peak_init(pk);
    for (int y = y_lo + tid; y < y_hi; y += NT) {
        float acc = 0.f;
#pragma unroll 13
        for (int t = 0; t < L; ++t) {
            const f2 r = Rc[y + t];
            const f2 w = tcol[t];
            acc = __builtin_fmaf(r.x, w.x, acc);
            acc = __builtin_fmaf(r.y, w.y, acc);
        }
        const int lin = x * g.n1 + y;
        if (RESP) g.resp[(long long)b * g.n1 * g.n2 + lin] = acc;
        peak_push(pk, acc, lin);
    }
    peak_wave_reduce(pk);
    if (lane == 0) { sval[wave] = pk.best; sidx[wave] = pk.idx; ssec[wave] = pk.second; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) peak_merge(pk, sval[w], sidx[w], ssec[w]);
        g.part_val[b * g.nslots + g.nstrips + rc] = pk.best;
        g.part_idx[b * g.nslots + g.nstrips + rc] = pk.idx;
        g.part_sec[b * g.nslots + g.nstrips + rc] = pk.second;
    }
}

} // namespace pdog
