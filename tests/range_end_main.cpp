// range_end_main.cpp — the range-end rule of the roll kernel's PRUNE instances (csrc/dog_roll_range.hpp) against the row-tap
// pairs counted one by one.  Host program, no HIP: tests/test_range_end_cpu.py builds and runs it.
//
// For every kernel length of roll_lengths.def, every window height n1 of a small set (40 … 47: every n1 mod 8; 2 l + 29: the
// height of tests/prune_length_scenes.py, long enough for full bodies between a range's prologue and its end) and every kept
// range [ba, bb) of such a window, the program walks the sub-chunks sc = ba … prune_sc_hi − 1 as roll_strip does and
//   * finds the last output the loop emits by listing the emitted rows, and compares roll_end_y;
//   * lists every pair (row a = 8·sc + i, tap t) whose output y = a − t is one the loop emits whole, 8·ba ≤ y ≤ y_end, and
//     the tap block roll_col_body meets it in: none may lie below roll_end_qlo (nothing needed is skipped), none at or past
//     the sub-chunk's last block (the shortened prologue bodies, roll_prologue_blocks), and the lowest of them must BE
//     roll_end_qlo — the header's tm and qlo are the exact ones, so a rule that skips less than it could fails here too;
//   * holds the block the kernel ENTERS at, roll_end_entry, to that: it is conservative ON PURPOSE — qlo rounded down to a
//     multiple of roll_entry_step(l), for the compile time's sake (the header says why) — so it must be a multiple of the
//     step, not above the lowest needed block and less than one step below it;
//   * holds the prologue / end property: a prologue body is entered below its own last block.
// It also counts the tap blocks the entry saves, per length, for the record.  Exit status: the number of violations, capped.
#include <cstdio>
#include <cstdlib>

#include "dog_roll_range.hpp"

using namespace pdog;

#define PDOG_ROLL_L(l) static_assert(roll_end_covers(l) && roll_end_meets_prologue(l), "range-end rule");
#include "roll_lengths.def"
#undef PDOG_ROLL_L
// (a rule one block too eager must not pass the header's own check: the check is not vacuous)
constexpr bool eager_rule_is_caught()
{
    for (int tm = 3; tm <= 64; ++tm)
        if (roll_tap_block(tm, 0) < roll_end_qlo(tm) + 1) return true;
    return false;
}
static_assert(eager_rule_is_caught(), "tap tm of row 0 lies in block roll_end_qlo(tm): entering one block later drops it");

static const int LENGTHS[] = {
#define PDOG_ROLL_L(l) l,
#include "roll_lengths.def"
#undef PDOG_ROLL_L
};

static long long bad = 0;
static void fail(const char *what, int L, int n1, int ba, int bb, int sc, int got, int want)
{
    if (bad++ < 20) std::printf("MISMATCH %s: l=%d n1=%d range [%d, %d) sub-chunk %d: %d, expected %d\n", what, L, n1, ba, bb, sc, got, want);
}

int main()
{
    long long ranges = 0, subchunks = 0, pairs = 0;
    for (int L : LENGTHS) {
        const int NQB = roll_col_blocks(L), NPRO = roll_prologue_len(L);
        long long blocks_run = 0, blocks_saved = 0, blocks_dead = 0;
        int heights[9];
        for (int r = 0; r < 8; ++r) heights[r] = 40 + r;
        heights[8] = 2 * L + 29;
        for (int n1 : heights) {
            const int NA = n1 + L - 1, nsub = (NA + ROLL_CH - 1) / ROLL_CH, nblk = (n1 + ROLL_CH - 1) / ROLL_CH;
            for (int ba = 0; ba < nblk; ++ba)
                for (int bb = ba + 1; bb <= nblk; ++bb) {
                    ++ranges;
                    const int sc_hi = prune_sc_hi(ba, bb, L, nsub), y_lo = ROLL_CH * ba;
                    // the last row the loop emits, by listing them (roll_strip's emit: rows of sub-chunk sc inside the window)
                    int y_last = -1;
                    for (int sc = ba; sc < sc_hi; ++sc)
                        for (int i = 0; i < ROLL_CH; ++i) {
                            const int y = ROLL_CH * sc - (L - 1) + i;
                            if (y >= y_lo && y < n1 && y > y_last) y_last = y;
                        }
                    const int y_end = roll_end_y(sc_hi, L, n1);
                    if (y_end != y_last) fail("y_end", L, n1, ba, bb, -1, y_end, y_last);
                    if (y_last < ROLL_CH * bb - 1 && y_last < n1 - 1) fail("the range's own rows are not all emitted", L, n1, ba, bb, -1, y_last, ROLL_CH * bb - 1);
                    for (int sc = ba; sc < sc_hi; ++sc) {
                        ++subchunks;
                        const int j = sc - ba;
                        const int qhi = (j < NPRO && roll_prologue_blocks(j) < NQB) ? roll_prologue_blocks(j) : NQB;
                        const int qlo = roll_end_qlo(roll_end_tm(sc, y_end));
                        int lowest = NQB, highest = -1;
                        for (int i = 0; i < ROLL_CH; ++i) {
                            const int a = ROLL_CH * sc + i;
                            for (int t = 0; t <= L - 1; ++t) {
                                const int y = a - t;
                                if (y < y_lo || y > y_last) continue; // not an output the loop emits whole
                                ++pairs;
                                const int blk = roll_tap_block(t, a & 1);
                                if (blk < lowest) lowest = blk;
                                if (blk > highest) highest = blk;
                            }
                        }
                        if (highest < 0) { fail("a sub-chunk of the range feeds no emitted output", L, n1, ba, bb, sc, highest, 0); continue; }
                        if (lowest < qlo) fail("a needed pair lies in a skipped block", L, n1, ba, bb, sc, qlo, lowest);
                        if (lowest > qlo) fail("the entry skips less than it could", L, n1, ba, bb, sc, qlo, lowest);
                        if (highest >= qhi) fail("a needed pair lies past the body's last block", L, n1, ba, bb, sc, qhi, highest);
                        if (qlo >= qhi) fail("a body entered at or past its own last block", L, n1, ba, bb, sc, qlo, qhi);
                        const int step = roll_entry_step(L), entry = roll_end_entry(qlo, L);
                        if (entry % step != 0 || entry > lowest || lowest - entry >= step) fail("the entry is not the lowest needed block rounded down to the step", L, n1, ba, bb, sc, entry, lowest / step * step);
                        if (n1 == 2 * L + 29) { blocks_run += qhi - entry; blocks_saved += entry; blocks_dead += qlo; }
                    }
                }
        }
        std::printf("l=%3d: %2d blocks, prologue %2d, step %d; over every range of a %d-row window the entry saves %lld of %lld tap blocks (%.1f %%; dead: %lld)\n", L, NQB,
                    NPRO, roll_entry_step(L), 2 * L + 29, blocks_saved, blocks_run + blocks_saved, 100.0 * (double)blocks_saved / (double)(blocks_run + blocks_saved), blocks_dead);
    }
    std::printf("%lld ranges, %lld sub-chunks, %lld row-tap pairs; %lld mismatches\n", ranges, subchunks, pairs, bad);
    return bad ? 1 : 0;
}
