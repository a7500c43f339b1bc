// dog_roll_range.hpp — which column-pass tap blocks a sub-chunk of a KEPT RANGE needs (dog_roll.hpp, roll_strip), free of HIP
// so that a host program can hold the rule against the row-tap pairs counted one by one (tests/range_end_main.cpp).
//
// A kept range [ba, bb) of 8-row output blocks runs the sub-chunks sc_lo = ba … sc_hi − 1, sc_hi = prune_sc_hi(ba, bb, l, nsub).
// Sub-chunk sc emits the outputs 8·sc − (l − 1) … 8·sc − (l − 1) + 7 that lie inside the window, so the last output the loop
// ever emits is
//     y_end = min(8·sc_hi − l, n1 − 1)                                                              (roll_end_y)
// and nothing reads an accumulator slot after it.  Row a of the tile feeds output y = a − t through tap t: in sub-chunk sc,
// rows a = 8·sc + i, only the taps t ≥ tm + i with
//     tm = 8·sc − y_end                                                                             (roll_end_tm)
// still have an emitted output.  Row i (parity p = i & 1) meets its taps in pairs (T[tt], T[tt − 1]), tt ≡ p mod 2, and block
// qb of roll_col_body holds tt = p + 4·qb and p + 4·qb + 2: the taps 4·qb − 1 … 4·qb + 2 of an even row, 4·qb … 4·qb + 3 of an
// odd one.  Every tap of block qb is dead for every row of the sub-chunk iff its largest tap is: 4·qb + 2 < tm for i = 0,
// 4·qb + 3 < tm + 1 for i = 1, and the later rows ask for less.  Both say 4·qb + 3 ≤ tm, so the first block that holds a live tap is
//     qlo = (tm + 1) >> 2   (tm > 0),   0 otherwise                                                  (roll_end_qlo)
// — exact, not a bound: block qlo holds tap tm of row 0 or one above it.  tm ≤ l − 1 for every sub-chunk of every range
// (sc ≤ nsub − 1 and 8·nsub < n1 + l + 7), so qlo ≤ (l − 1) ÷ 4 < roll_col_blocks(l): a body always has a block to enter at.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ROLL_HD __host__ __device__ constexpr
#else
#define ROLL_HD constexpr
#endif

namespace pdog {

constexpr int ROLL_CH = 8;   // rows per sub-chunk (16 measured equal on cfg3: the kernel is VALU-bound, not latency-bound)
constexpr int ROLL_QB = 2;   // tap pairs per block (2 parities x 2 channels x QB pairs = 16 SGPRs, double-buffered)
ROLL_HD int roll_col_blocks(int L) { return ((L + 1) / 2 + ROLL_QB - 1) / ROLL_QB; }
ROLL_HD int roll_prologue_blocks(int sc) { return 2 * sc + 2; }
ROLL_HD int roll_prologue_len(int L) { return (roll_col_blocks(L) - 2 + 1) / 2; } // sub-chunks with fewer blocks than the full body

// KEPT RANGES (dog_prune.hpp; LaunchGeo::prune): a slot's pre-pass leaves the range [ba, bb) of 8-row output blocks that can
// hold the window's peak or a near-tie.  Block j reads the input rows of sub-chunks j … j + prune_span(l) − 1; the range
// needs sub-chunks ba … prune_sc_hi − 1.
ROLL_HD int prune_span(int L) { return (ROLL_CH + L - 1 + ROLL_CH - 1) / ROLL_CH; }
ROLL_HD int prune_tail(int L) { return (L - 1 + ROLL_CH - 1) / ROLL_CH; }
ROLL_HD int prune_sc_hi(int ba, int bb, int L, int nsub) { return bb > ba ? (bb + prune_tail(L) < nsub ? bb + prune_tail(L) : nsub) : ba; }

// ---- the range's end (header comment) ----
ROLL_HD int roll_end_y(int sc_hi, int L, int n1) { return ROLL_CH * sc_hi - L < n1 - 1 ? ROLL_CH * sc_hi - L : n1 - 1; }
ROLL_HD int roll_end_tm(int sc, int y_end) { return ROLL_CH * sc - y_end; }
ROLL_HD int roll_end_qlo(int tm) { return tm > 0 ? (tm + 1) >> 2 : 0; }
// THE ENTRY the kernel takes: roll_end_qlo rounded DOWN to a multiple of roll_entry_step(l) — conservative on purpose (up to
// step − 1 blocks run for nothing).  One entry per block gave every column-pass body of every PRUNE instance as many basic
// blocks as it has tap blocks, each a join of all accumulator registers, and the roll translation units compiled 3.5 times as
// long (l = 149 alone: eleven minutes); the cost grows faster than the length, so the two-waves lengths take a coarser step.
// One entry per four blocks: the last seven sub-chunks of a range at l = 65 skip 12 + 12 + 8 + 8 + 4 + 4 + 0 = 48 of their 56
// dead blocks.  Per eight: a range at l = 109 skips 144 of its 182.
ROLL_HD int roll_entry_step(int L) { return L <= 81 ? 4 : 8; }
ROLL_HD int roll_end_entry(int qlo, int L) { return qlo & ~(roll_entry_step(L) - 1); }
// the block of roll_col_body that holds tap t of a row of parity p
ROLL_HD int roll_tap_block(int t, int p) { return ((((t ^ p) & 1) ? t + 1 : t) - p) / 2 / ROLL_QB; }

// The mirror of roll_start_covers (dog_roll.hpp).  True iff, for every tm a sub-chunk can meet (1 … l − 1: above), every row
// i of the sub-chunk and every tap t ≥ tm + i (every tap that still has an emitted output), the tap's pair lies in a block
// ≥ roll_end_qlo(tm) — entering the body at that block leaves out no term of an emitted output — and the block below qlo
// holds no such tap — and no later entry would do.
ROLL_HD bool roll_end_covers(int L)
{
    for (int tm = 1; tm <= L - 1; ++tm) {
        const int qlo = roll_end_qlo(tm);
        if (qlo >= roll_col_blocks(L)) return false;
        bool entry_block_live = qlo == 0;
        for (int i = 0; i < ROLL_CH; ++i)
            for (int t = tm + i; t <= L - 1; ++t) {
                if (roll_tap_block(t, i & 1) < qlo) return false;
                if (roll_tap_block(t, i & 1) == qlo) entry_block_live = true;
            }
        if (!entry_block_live) return false;
    }
    return true;
}
// Prologue and end in ONE sub-chunk (a range shorter than roll_prologue_len + prune_tail sub-chunks): the shortened body of
// sub-chunk j of the range runs blocks qlo … roll_prologue_blocks(j) − 1, which must not be empty.  Sub-chunk ba + j of a range
// that is not cut off by the window's bottom has tm = l − 8·(n − j), n = bb − ba + prune_tail ≥ prune_tail + 1 sub-chunks;
// one of a range that is cut off has tm = 8·(ba + j) − (n1 − 1) ≤ 8·j, since block ba holds a row of the window
// (8·ba ≤ n1 − 1).  True iff qlo < roll_prologue_blocks(j) for every prologue body j and every such tm.
// (The first family alone gives qlo ≤ 2·j − 2; the cut-off ranges reach qlo = 2·j.)
ROLL_HD bool roll_end_meets_prologue(int L)
{
    for (int j = 0; j < roll_prologue_len(L); ++j) {
        const int tm_open = L - ROLL_CH * (prune_tail(L) + 1 - j), tm_cut = ROLL_CH * j;
        for (int tm = 1; tm <= tm_open || tm <= tm_cut; ++tm)
            if (tm <= L - 1 && roll_end_qlo(tm) >= roll_prologue_blocks(j)) return false;
    }
    return true;
}

} // namespace pdog
