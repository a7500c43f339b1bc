// dog_layout.hpp — the kernels' size formulas (LDS pitches and byte counts, ring and slot counts, the constants they are made
// of), free of HIP so that the host compiler takes them alone: the kernel headers include this header and use the formulas
// in device code, pdog_plan.hpp derives the tracker's plan from them on the host, and tests/plan_main.cpp holds that plan on a
// machine without a GPU.  Each block names the kernel header it belongs to; that header says what the numbers mean.  Where a
// formula counts f2 elements it writes 8 bytes, and the owning kernel header asserts sizeof(f2) == 8.
#pragma once
#include <cstddef>

#include "dog_roll_range.hpp" // ROLL_CH

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LAYOUT_HD __host__ __device__ constexpr
#else
#define LAYOUT_HD constexpr
#endif

namespace pdog {

// ---- dog_kernels.hpp: the ring kernels ----
LAYOUT_HD int round_up(int v, int m) { return (v + m - 1) / m * m; }
// LDS row pitches.  A (f32 input tile) is read by lanes that sit in consecutive
// rows (ds_read_b32, 32 banks): an odd pitch spreads them over all banks.
LAYOUT_HD int pitch_a(int cols) { return cols | 1; }
// R ring (f2 per element) is written row-per-lane (ds_write_b64) and read
// column-per-lane (ds_read_b64, conflict free for any pitch); pitch in f2 units
// with 2*pitch ≡ 2 (mod 32) would be ideal for the writes; odd is a good compromise.
LAYOUT_HD int pitch_r(int tw) { return tw | 1; }
LAYOUT_HD int ring_rows(int CH, int L, int Q)
{
    // rows a col-pass span can touch: CH new + L-1 halo + (Q-1) slack when the
    // chunk cadence leaves a partial Q-group behind; multiple of 4 for the wrap logic
    return round_up(CH + L - 1 + (((CH % Q) == 0 && ((L - 1) % Q) == 0) ? 0 : Q - 1), 4);
}

// ---- dog_roll.hpp: the roll kernels and their thin-remainder kernel ----
constexpr int ROLL_P = 8;    // row-pass outputs per lane
constexpr int ROLL_TW = 64;  // strip width = lanes
constexpr int ROLL_PR = 65;  // R pitch (f2)
constexpr int ROLL_LMIN = 17; // the shortest kernel length with a roll instance (dog_roll.hpp: ROLL_LMAX, the longest)
// staging: 8 lanes per input row, each SB (multiple of 4) bytes.  A rows are 16-byte aligned and their bases are
// skewed by {0,1,8,9} 16-byte slots (row & 3) on a pitch that is a multiple of 256 B: the row pass reads ds_read_b128
// quads at (row base + 8·group + 4·q) floats, and with that skew the 16 lanes of every b128 lane group
// (MI355X_MICROARCH.md, LDS) land on 16 distinct slots of the 256-B bank row — conflict-free.
LAYOUT_HD int roll_sb(int L) { return ((ROLL_TW + L - 1 + 7) / 8 + 3) / 4 * 4; }
LAYOUT_HD int roll_rs(int L) { return (8 * roll_sb(L) + 40 + 63) / 64 * 64; } // A row pitch in floats (36 of skew + the 129th column of a folded strip)
LAYOUT_HD size_t roll_lds_bytes(int L) { return (size_t)ROLL_CH * roll_rs(L) * 4 + (size_t)ROLL_CH * ROLL_PR * 8; }
// dynamic LDS of dog_thin_kernel: the R column (f2 per input row) and the column's input patch as bytes
LAYOUT_HD size_t thin_lds_bytes(int n1, int L) { return ((size_t)(n1 + L - 1) * 8 + 15) / 16 * 16 + (size_t)(n1 + L - 1) * ((L + 3) / 4 * 4); }

// ---- dog_fused.hpp: the fused kernel (and the tiled kernel's sub-windows, dog_tiled.hpp) ----
constexpr int FUSED_NT = 1024, FUSED_PMAX = 8, FUSED_U = 8;
// LDS pitches (odd ⇒ conflict-free strided reads) with room for the sliding windows of the last, partly masked
// output group of up to FUSED_PMAX outputs and their one-block prefetch
LAYOUT_HD int fused_pitch_a(int n2, int L) { return ((n2 + FUSED_PMAX - 1) / FUSED_PMAX * FUSED_PMAX + L + FUSED_U + 1) | 1; }
LAYOUT_HD int fused_pitch_v(int n1, int L) { return ((n1 + FUSED_PMAX - 1) / FUSED_PMAX * FUSED_PMAX + L + 24 + 1) | 1; } // + 24: the compile-time-l column pass reads whole 16-tap blocks
LAYOUT_HD size_t fused_a_bytes(int n1, int n2, int L) { return ((size_t)(n1 + L - 1) * fused_pitch_a(n2, L) * 4 + 15) / 16 * 16; }
LAYOUT_HD size_t fused_lds_bytes(int n1, int n2, int L) { return fused_a_bytes(n1, n2, L) + (size_t)n2 * fused_pitch_v(n1, L) * 8; }
// the compile-time-l instances (dog_fused.hpp, "compile-time kernel length"): the tile in the roll kernel's layout
LAYOUT_HD bool fused_has_instance(int L) { return L % 4 == 1 && L >= 29 && L <= 101; } // lat_lengths.def
LAYOUT_HD int fusedc_pitch_a(int n2, int L) { return (8 * ((n2 + 7) / 8) + L + 39 + 63) / 64 * 64; }
LAYOUT_HD size_t fusedc_a_bytes(int n1, int n2, int L) { return ((size_t)(n1 + L - 1) * fusedc_pitch_a(n2, L) + 64) * 4; }
LAYOUT_HD size_t fusedc_lds_bytes(int n1, int n2, int L) { return fusedc_a_bytes(n1, n2, L) + (size_t)n2 * fused_pitch_v(n1, L) * 8; }
// outputs per row-pass task of the compile-time-l instances: 8, or 4 where that loads the busiest SIMD less (waves of 64 tasks,
// four SIMDs; ≈51 / ≈53 instructions per output)
LAYOUT_HD int fusedc_row_outputs(int NA, int n2)
{
    const int w8 = (NA * ((n2 + 7) / 8) + 63) / 64, w4 = (NA * ((n2 + 3) / 4) + 63) / 64;
    return ((w4 + 3) / 4) * 212 < ((w8 + 3) / 4) * 408 ? 4 : 8;
}

// ---- dog_tiled.hpp ----
constexpr int TILED_SLOT_CAP = 256; // sub-windows per window the combining wave handles (4 per lane)

// ---- dog_exact.hpp: the refinement's scratch ----
constexpr int REFINE_CAP = 512;    // candidate list entries
constexpr int REFINE_BLKCAP = 256; // column blocks listed for the rescan (more ⇒ every block is rescanned)
LAYOUT_HD int refine_tile_pitch(int ncol, int L) { return (ncol + L - 1 + 3) / 4 * 4; }
// dynamic LDS of a refinement: fixed part (table p/255.0, candidate list, reductions), row-pass block (f2 for stage 1,
// reused as 2 doubles per element for stage 2), optional pixel tile
LAYOUT_HD size_t refine_fixed_bytes() { return 256 * 8 + REFINE_CAP * 12 + 16 * 8 + 16 * 4 + 32 + REFINE_BLKCAP * 4 + 32; }
LAYOUT_HD size_t refine_r_bytes(int n1, int L, int cbw) { return (size_t)(n1 + L - 1) * cbw * 16; }
LAYOUT_HD size_t refine_tile_bytes(int rows, int L, int cbw) { return ((size_t)rows * refine_tile_pitch(cbw, L) + 15) / 16 * 16; }
// tile_rows: rows of the block's pixel tile resident at a time (n1 + l − 1 = all of them)
LAYOUT_HD size_t refine_lds_bytes(int n1, int L, int cbw, int tile_rows)
{
    return refine_fixed_bytes() + refine_r_bytes(n1, L, cbw) + refine_tile_bytes(tile_rows, L, cbw);
}

// ---- dog_twopass.hpp ----
constexpr int TWOPASS_FLUSH_L = 101; // kernel lengths from here on run the blocked-accumulation instances
LAYOUT_HD int twopass_ring(int P, int U) { return ((P + 2 * U - 1 + U - 1) / U) * U; } // register-ring slots = taps per trip
constexpr int HP_ROWS = 16; // rows per workgroup in both passes
// LDS row pitches of the two-pass kernels: the sliding windows (and their one-block prefetch) of the last,
// partly masked group of 13 outputs must stay inside the zero-padded row.  nout outputs, l taps.
// `quantum` = outputs one round of a workgroup covers (groups × outputs per task); + l rounded up to a block of 16 taps + one block of prefetch
LAYOUT_HD int twopass_pitch_q(int nout, int L, int quantum) { return (round_up(nout, quantum) + L + 48) | 1; }
LAYOUT_HD int twopass_pitch(int nout, int L, int rows = HP_ROWS) { return twopass_pitch_q(nout, L, rows == 8 ? 32 * 7 : 16 * 13); }

} // namespace pdog
