// pdog_plan.hpp — the tracker's PLAN as a host-only value: everything pawsome_dog.hip derives from the geometry (fh, fw, n1,
// n2, l), the switches and a pinned variant id — which kernel variant, how many strips and the thin remainder, the refinement's
// block geometry, the fused kernel's tile and LDS, the tiled kernel's sub-windows, the two-pass task sizes, part_slots — and
// the rules that read it: path_for_batch, chain_path, the exact-mode thresholds.  Integer and double arithmetic only: no HIP,
// no tracker, no function pointer, so the host compiler takes this header alone and tests/plan_main.cpp replays the recorded
// plans (tests/golden/dispatch_paths.json) on a machine without a GPU.  pawsome_dog.hip makes a Plan (make_plan), raises the
// LDS limits it lists and asks the device's occupancy questions (apply_plan), and only then keeps it; the kernels a variant's
// shape stands for are that unit's table (kVariants), row for row beside kVariantShapes.
#pragma once
#include "../../include/pawsome_dog.h" // PDOG_OK, PDOG_E_ARG
#include "dog_layout.hpp"
#include "dog_roll_range.hpp"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <string>
#include <vector>

namespace pdog {

// Run-time configuration.  The PRODUCT build reads four RESOURCE limits from the environment, once, when a tracker is
// created (never on the launch path: a functor call's whole budget is ≈23 µs).  Everything that selects a code path is
// either API (pdog_set_exact, pdog_set_variant, pdog_set_tuning — explicit, per tracker) or exists only in the diagnostic
// build (make diag, -DPDOG_ABLATIONS), which also reads the tuning switches from the environment for tools/.
struct Switches {
    // resource limits (environment, product build)
    size_t scratch_cap = (size_t)6 << 30; // PDOG_SCRATCH_MB: HBM scratch of the two-pass intermediate; larger batches go in chunks
    size_t map_cap = (size_t)4 << 30;     // PDOG_MAP_MB: largest FP32 response map the two-pass path keeps for exact mode (beyond: candidates are recomputed)
    int host_threads = 0;                 // PDOG_HOST_THREADS (0: min(16, cores))
    int ingest_chunk = 0;                 // PDOG_INGEST_CHUNK (0: ≈32 MB of tiles)
    // path selection (pdog_set_tuning; the tests exercise every alternative path of the product through it)
    bool host_copy = false;               // functor: upload the tile with copy commands and synchronise the stream instead of the in-place tile + ticket
    bool host_sync = false;               // functor: in-place tile, but wait with hipStreamSynchronize instead of polling the ticket
    bool twopass_4l = false;              // two-pass path always in its four-launch form
    bool no_tiled = false;                // single large windows stay on the two-pass launches
    bool no_roll_map = false;             // hard batches on the roll / ring kernels keep recomputing their candidates
    bool no_fold = false;                 // a single remainder column always goes to dog_thin_kernel
    bool fold_always = false;             // … always into the last strip, also below 8 strips per window
    bool no_pad_skip = false;             // roll kernels: sub-chunks that hold padding only run the full path (dog_roll.hpp, "padding rows")
    bool no_prune = false;                // roll batches stay dense: no pre-pass, no kept ranges (dog_prune.hpp)
    bool no_refine = false;               // pruned roll batches: the first-stage hulls as they are, no bound per output cell (dog_prune.hpp, "the cell bound")
    bool no_range_end = false;            // pruned roll batches: full-length column-pass bodies to the end of a kept range (dog_roll_range.hpp)
    bool fenced_publish = false;          // pre-pass: per-workgroup counts and an acquire-release arrival also where the packed word fits (dog_prune.hpp, the publish block)
    bool no_fused_c = false;              // the fused kernel's runtime-length instance also where a compile-time-l instance exists
    bool measure_global = false;          // pdog_measure reads the frame itself instead of staging each position's pixel tile in LDS
    bool fault_inject = false;            // tests: one sub-window of a tiled chain never delivers its second frame's partial (the device-side waits must give up)
    // tuning and diagnosis (diagnostic build only)
    bool host_trace = false, hpass16 = false, ingest_no_nt = false, ingest_trace = false, fused_diag = false;
    bool tiled_force = false;             // the tiled kernel also for windows the fused kernel serves
    bool no_host_dc = false;              // the functor's kernels sample the DC level themselves
    int tiled_sub = 0;                    // sub-window edge of the tiled kernel (0: chosen per geometry)
    int tp_ph1 = 0, tp_php = 0;           // outputs per task of the two-pass kernels (0: per geometry)
    int v_after = 64;                     // exact mode, map path: first-scan candidates beyond which the window's own |pixel − dc| bound is computed
    int h1_u = 4;                         // taps per block of the two-pass row pass (4, or 8)
    int hp_u = 8;                         // taps per block of the two-pass column pass (8 or 16)
    int tiled_batch = 2;                  // windows per batch up to which the tiled kernel is used
    int fused_pr = 0, fused_pc = 0;       // outputs per task of the fused kernel (0: chosen per geometry)
    int lds_pad = 0;                      // occupancy experiments
};

// frame size, window size (both odd) and kernel length
struct Geometry {
    int fh = 0, fw = 0, n1 = 0, n2 = 0, L = 0;
};

// ---- compiled kernel specialisations: their shapes (the kernels themselves: kVariants, pawsome_dog.hip) ----
// path ids that pdog_kernel_for_batch reports beside the variant ids: the fused, two-pass and tiled kernel families
constexpr int kPathFused = 300, kPathTwoPass = 200, kPathTiled = 400;
constexpr size_t kMaxLds = 160 * 1024;
constexpr int kThinMax = 6; // remainder columns done by dog_thin_kernel instead of one more strip
// Ring: dog_kernels.hpp (a workgroup per strip); Roll: dog_roll.hpp (one wave per 64-column strip); TwoPass: dog_twopass.hpp
// (vertical pass → HBM → horizontal pass); Fused: dog_fused.hpp (one workgroup per window, whole tile in LDS)
enum class Family { Ring, Roll, TwoPass, Fused };
struct VariantShape {
    int id;
    Family family;
    int P, XG, Q, CH, LT, NT;
    bool full_set; // a roll row of roll_lengths.def: beside the strip kernels the thin-remainder, chain, table, PRUNE and predicted-chain instances
    constexpr int tw() const { return P * XG; }
    constexpr int ring(int L) const { return LT ? ring_rows(CH, LT, Q) : ring_rows(CH, L, Q); }
    constexpr int pa(int L) const { return pitch_a(tw() + L - 1); }
    constexpr size_t lds(int L) const
    {
        if (family == Family::TwoPass || family == Family::Fused) return 0; // sized per window at launch
        if (family == Family::Roll) return roll_lds_bytes(LT);
        return (size_t)round_up(CH * pa(L) * 4, 16) + (size_t)ring(L) * pitch_r(tw()) * 8;
    }
};
#define PDOG_RING_SHAPE(id, P, XG, Q, CH, LT, NT) VariantShape { id, Family::Ring, P, XG, Q, CH, LT, NT, false }
#define PDOG_ROLL_SHAPE(id, LT) VariantShape { id, Family::Roll, ROLL_P, ROLL_TW / ROLL_P, ROLL_CH, ROLL_CH, LT, 64, true }
#define PDOG_ABLATION_SHAPE(id) VariantShape { id, Family::Roll, ROLL_P, 8, ROLL_CH, ROLL_CH, 65, 64, false }
inline constexpr VariantShape kVariantShapes[] = {
    // runtime-L (any target_width)
    PDOG_RING_SHAPE(0, 4, 8, 8, 32, 0, 256),
    PDOG_RING_SHAPE(1, 8, 8, 8, 32, 0, 256),
    PDOG_RING_SHAPE(2, 11, 8, 8, 32, 0, 256),
    // l = 65 (target_width 25, the reference default)
    PDOG_RING_SHAPE(10, 11, 8, 16, 32, 65, 256),
    PDOG_RING_SHAPE(11, 11, 8, 8, 24, 65, 256),
    PDOG_RING_SHAPE(12, 8, 8, 16, 32, 65, 256),
    PDOG_RING_SHAPE(13, 8, 8, 8, 32, 65, 256),
    PDOG_RING_SHAPE(14, 11, 8, 8, 32, 65, 256),
    // rolling-accumulator kernel: one instance per kernel length l = 4m+1 of roll_lengths.def (target_width ≈ 5 … 39); id = 100 + l, l = 65 → 100
#define PDOG_ROLL_L(LT) PDOG_ROLL_SHAPE((LT) == 65 ? 100 : 100 + (LT), LT),
#include "roll_lengths.def"
#undef PDOG_ROLL_L
    // any l: two launches with the intermediate in HBM (long kernels, target_width ≳ 40)
    VariantShape { kPathTwoPass, Family::TwoPass, 13, 16, 16, 16, 0, 256, false },
    // any l, windows whose padded tile fits in LDS: one workgroup per window, one launch (latency path)
    VariantShape { kPathFused, Family::Fused, 1, 1, 1, 1, 0, FUSED_NT, false },
#ifdef PDOG_ABLATIONS
    PDOG_ABLATION_SHAPE(101), PDOG_ABLATION_SHAPE(102), PDOG_ABLATION_SHAPE(103), PDOG_ABLATION_SHAPE(104), PDOG_ABLATION_SHAPE(105), PDOG_ABLATION_SHAPE(106),
#endif
    // l = 29 (target_width 10, the reference test default)
    PDOG_RING_SHAPE(20, 8, 8, 4, 32, 29, 256),
};
#undef PDOG_RING_SHAPE
#undef PDOG_ROLL_SHAPE
#undef PDOG_ABLATION_SHAPE
constexpr int kNumVariants = sizeof(kVariantShapes) / sizeof(kVariantShapes[0]);

constexpr bool has_roll_instance(int L)
{
    for (int i = 0; i < kNumVariants; ++i)
        if (kVariantShapes[i].family == Family::Roll && kVariantShapes[i].LT == L && kVariantShapes[i].id >= 100 && kVariantShapes[i].id < 300) return true;
    return false;
}

constexpr const VariantShape *find_variant(int id)
{
    for (int i = 0; i < kNumVariants; ++i)
        if (kVariantShapes[i].id == id) return &kVariantShapes[i];
    return nullptr;
}

// ---- what make_plan derives ----
// what the fused and tiled kernels share: the instance and, for the tile one workgroup works on, pitches and task sizes (plan_tile)
struct TilePlan {
    bool c = false; // the compile-time-l instance (lat_lengths.def) and its wider tile layout
    int pitchA = 0, pitchV = 0, pr = 0, pc = 0, cshift = 0;
};
// fused kernel (dog_fused.hpp): one workgroup per window, the whole tile in LDS
struct FusedPlan : TilePlan {
    bool ok = false;               // the window's tile fits in LDS: the fused kernel takes small batches and short chains
    size_t lds = 0;                // dynamic LDS: the tile + RT, or the scratch of the refinement it may run in the same memory
    int ref_cbw = 1, ref_rows = 8; // refinement geometry inside the kernel (its scratch is the kernel's own LDS)
};
// tiled kernel (dog_tiled.hpp): one large window cut into sub-windows, a workgroup each, one launch per batch / clip
struct TiledPlan : TilePlan {
    bool ok = false;
    int sn1 = 0, sn2 = 0, ns1 = 0, ns2 = 0;
    int ref_cbw = 1, ref_rows = 8; // refinement scratch geometry
    size_t lds = 0;
};
// The dynamic-LDS limit the plan wants raised per kernel family, in the order apply_plan raises them (0: that family is not
// set up, nothing is raised): the fused and the tiled kernel's instances, the two-pass column pass in its 16-row and 8-row
// forms and the row pass, the thin-remainder kernel, the batch kernel, the finishing kernel (the refinement's block).
struct PlanLds {
    size_t fused = 0, tiled = 0, tp_col16 = 0, tp_col8 = 0, tp_row = 0, thin = 0, batch = 0, finish = 0;
};
struct Plan {
    Geometry geo;
    const VariantShape *shape = nullptr; // the tracker's batch kernel
    int nstrips = 0;
    int nthin = 0, thin_x0 = 0;          // window columns handled by the thin-remainder kernel
    bool forced = false;                 // pdog_set_variant pinned the kernel: no batch-size switching
    bool small_twopass = false;          // two-pass kernels are set up and may take over small batches
    int ref_cbw = 1, ref_rows = 8;       // refinement: window columns per block; rows of the block's pixel tile resident in LDS at a time
    int tp_ph1 = 13, tp_php = 7;         // outputs per task of the two-pass row / column pass (pick_h1_outputs, pick_hpass_outputs)
    // the kernels' partials are [n][part_slots]: the most slots per window any variant or the tiled kernel writes, so that a
    // later pdog_set_variant never reallocates
    int part_slots = 1;
    FusedPlan fused;
    TiledPlan tiled;
    PlanLds lds;
};

// Outputs per task (P) of the two-pass ROW pass, per geometry.  A workgroup covers 16 × P outputs per round: a 257-wide
// window on P = 13 (208 per round) ran a second round 24 % full.  Measured per launch (4096 windows, same session):
//   257 wide, l = 109:  P = 5 1.94 ms, 7 1.83, 9 1.84, 11 2.20, 13 2.39, 17 2.18   (96 VGPRs at P = 9, 155 at 13)
//   205 wide, l = 293:  P = 5 4.35 ms, 7 4.17, 9 4.11, 11 4.61, 13 3.97            (13: one round, 98 % full)
// ⇒ P = 9 unless P = 13 fills its rounds better.  4-tap blocks (70 / 96 VGPRs instead of 94 / 155) gave another 2–5 %:
//   257 wide, l = 109:  P = 9 1.80 ms, 11 1.94, 13 2.17, 17 1.86;   205 wide, l = 293:  P = 9 4.20 ms, 13 3.95, 17 4.64
// COLUMN pass (32 × P outputs per round, 8 taps per block: 76 VGPRs against 125 with 16-tap blocks, −8 % on every config):
//   257 tall, l = 109:  P = 5 2.13 ms, 7 2.36, 9 1.96, 13 2.37
//   205 tall, l = 293:  P = 5 3.44 ms, 7 2.50, 9 2.57, 13 3.45
// ⇒ P = 7 unless P = 9 fills its rounds better.
inline int pick_h1_outputs(int nout)
{
    auto fill = [&](int p) { return (double)nout / (double)(round_up(nout, 16 * p)); };
    return fill(13) > fill(9) + 0.05 ? 13 : 9;
}
inline int pick_hpass_outputs(int nout)
{
    auto fill = [&](int p) { return (double)nout / (double)(round_up(nout, 32 * p)); };
    return fill(9) > fill(7) + 0.05 ? 9 : 7;
}
inline int refine_slice_rows(int NA, int L, int cbw, size_t budget)
{
    return (int)std::max<size_t>(8, std::min<size_t>((size_t)NA, budget / (size_t)refine_tile_pitch(cbw, L)));
}

// Outputs per task of the fused / tiled kernels: fewest rounds of 1024 tasks, then least work per task (≈ P outputs + a fixed cost)
inline int pick_outputs_per_task(int lines, int nout, std::initializer_list<int> ps, double fixed)
{
    int best = 0;
    double best_cost = 0;
    for (int p : ps) {
        const long long tasks = (long long)lines * ((nout + p - 1) / p);
        const double cost = (double)((tasks + FUSED_NT - 1) / FUSED_NT) * (p + fixed);
        if (!best || cost < best_cost) { best = p; best_cost = cost; }
    }
    return best;
}

// Pitches and task sizes of a tile of n1 × n2 outputs (the window, or a sub-window of it) under the instance p.c names.
inline void plan_tile(TilePlan &p, int n1, int n2, int L)
{
    p.pitchA = p.c ? fusedc_pitch_a(n2, L) : fused_pitch_a(n2, L);
    p.pitchV = fused_pitch_v(n1, L);
    for (p.cshift = 0; (1 << p.cshift) < (n2 + L - 1 + 3) / 4;) ++p.cshift;
    p.pr = p.c ? fusedc_row_outputs(n1 + L - 1, n2) : pick_outputs_per_task(n1 + L - 1, n2, {3, 4, 5, 6, 8}, 2.0);
    p.pc = pick_outputs_per_task(n2, n1, {2, 3, 4, 6, 8}, 1.5);
}

// The fused kernel for this geometry: its instance, its LDS and the refinement's share of it, whether it fits (the one place
// that decides), and what a launch copies into FusedGeo.
inline FusedPlan plan_fused(const Geometry &g, const Switches &sw)
{
    const int NA = g.n1 + g.L - 1, TWin = g.n2 + g.L - 1;
    FusedPlan f;
    f.c = fused_has_instance(g.L) && fusedc_lds_bytes(g.n1, g.n2, g.L) <= kMaxLds - 1024 && !sw.no_fused_c;
    // inside the fused kernel the refinement's scratch is that kernel's own LDS (tile + RT, free by then): the widest block that
    // fits it with the whole pixel tile resident (a window whose tile fits as floats has room for it as bytes)
    const size_t tile = f.c ? fusedc_lds_bytes(g.n1, g.n2, g.L) : fused_lds_bytes(g.n1, g.n2, g.L);
    f.ref_cbw = 1;
    f.ref_rows = NA;
    for (int cbw = std::min(8, g.n2); cbw >= 1; --cbw)
        if (refine_lds_bytes(g.n1, g.L, cbw, NA) <= tile) { f.ref_cbw = cbw; break; }
    if (refine_lds_bytes(g.n1, g.L, 1, NA) > kMaxLds - 1024) f.ref_rows = refine_slice_rows(NA, g.L, 1, 24576);
    f.lds = std::max(tile, refine_lds_bytes(g.n1, g.L, f.ref_cbw, f.ref_rows));
    f.ok = f.lds <= kMaxLds - 1024 && TWin <= 4 * FUSED_NT && g.fw >= 4;
    plan_tile(f, g.n1, g.n2, g.L);
    if (sw.fused_pr) { f.pr = sw.fused_pr; f.pc = sw.fused_pc; } // tuning switch PDOG_FUSED_P
    return f;
}

// A kernel whose own LDS (`base` bytes, at least the refinement's smallest form) doubles as the refinement's scratch: the
// widest block of window columns (at most cbw_max, the plan's ref_cbw) whose fixed part plus 8 tile rows fits, then the
// tallest slice of its pixel tile (the whole tile if possible) — exact mode then costs the kernel no occupancy.
inline void fit_refine_scratch(const Geometry &g, int cbw_max, size_t base, int *ref_cbw, int *ref_rows)
{
    const int NA = g.n1 + g.L - 1;
    *ref_cbw = 1;
    *ref_rows = 8;
    for (int cbw = std::min(g.n2, cbw_max); cbw >= 1; --cbw) {
        const size_t fixed_r = refine_lds_bytes(g.n1, g.L, cbw, 0);
        if (fixed_r + (size_t)8 * refine_tile_pitch(cbw, g.L) > base) continue;
        *ref_cbw = cbw;
        *ref_rows = (int)std::min<size_t>((size_t)NA, (base - fixed_r) / (size_t)refine_tile_pitch(cbw, g.L));
        while (*ref_rows > 8 && refine_lds_bytes(g.n1, g.L, cbw, *ref_rows) > base) --*ref_rows;
        return;
    }
}
// Tiled kernel (dog_tiled.hpp): windows too large for the fused kernel, cut into sub-windows of ≈48 rows/columns (a
// 257×257 window: 6×6 of 43×43, each a tile of 107×107 like the default 45×45 window of the fused kernel).
// Fills p.tiled, p.lds.tiled and p.part_slots; reads p.fused and p.ref_cbw.
inline void plan_tiled(Plan &p, const Switches &sw)
{
    const Geometry &g = p.geo;
    TiledPlan &t = p.tiled = TiledPlan();
    // partial slots per window: the most over all variants, so that a later pdog_set_variant never reallocates …
    p.part_slots = (g.n2 + 7) / 8;
    for (const VariantShape &v : kVariantShapes)
        if (v.family != Family::Fused) p.part_slots = std::max(p.part_slots, (g.n2 + v.tw() - 1) / v.tw() + kThinMax);
    if ((p.fused.ok && !sw.tiled_force) || sw.no_tiled || g.fw < 4) return;
    // Sub-window edge: ≈32 measured best for a 257×257 window (81 workgroups: 13.9 µs per frame; 48: 15.3), but beyond
    // ≈128 workgroups the partial exchange costs more than smaller tiles save (513×513: 121 workgroups of 47 → 17.8 µs,
    // 169 of 40 → 21.9); long kernels need smaller sub-windows for their halo to fit LDS.
    int sn1 = 0, sn2 = 0, ns1 = 0, ns2 = 0;
    size_t need = 0;
    bool found = false;
    const int user = sw.tiled_sub;
    t.c = fused_has_instance(g.L) && !sw.no_fused_c;
    // (round 3, with the one-round-trip exchange: 129×129 at 24 → 36 workgroups 8.6–8.8 µs against 9.2–9.7 at 32 → 25; 257×257 at 20 / 24 /
    // 32: 9.8–10.1 / 10.2 / 10.2–10.5 — kept at 32 so that three clips stay resident; 513×513 at 36 → 225 workgroups 12.2–12.6 against 13.0 at 48)
    bool small_first = true;
    for (int target : {24, 32, 40, 48, 56, 64, 24, 16}) {
        const bool probe24 = small_first && target == 24; // small windows first try 24: only while that keeps the clip at ≤ 48 workgroups
        small_first = false;
        if (user) target = user;
        ns1 = (g.n1 + target - 1) / target;
        ns2 = (g.n2 + target - 1) / target;
        sn1 = (g.n1 + ns1 - 1) / ns1;
        sn2 = (g.n2 + ns2 - 1) / ns2;
        ns1 = (g.n1 + sn1 - 1) / sn1;
        ns2 = (g.n2 + sn2 - 1) / sn2;
        need = t.c ? fusedc_lds_bytes(sn1, sn2, g.L) : fused_lds_bytes(sn1, sn2, g.L);
        const bool fits = need <= kMaxLds - 1024 && sn2 + g.L - 1 <= 4 * FUSED_NT && (long long)g.n1 * g.n2 < (1 << 24) && // (a partial's index shares a word with 8 tag bits)
                          (long long)ns1 * ns2 <= (target >= 32 && !user ? 128 : TILED_SLOT_CAP);
        if (fits && !(probe24 && !user && (long long)ns1 * ns2 > 48)) { found = true; break; }
        if (user) break;
    }
    if (!found) return;
    // the refinement's scratch is the kernel's own LDS: at least its smallest form must fit; then the widest block that does
    const size_t base = std::max(need, refine_lds_bytes(g.n1, g.L, 1, 8));
    if (base > kMaxLds - 1024) return;
    fit_refine_scratch(g, p.ref_cbw, base, &t.ref_cbw, &t.ref_rows);
    t.sn1 = sn1; t.sn2 = sn2; t.ns1 = ns1; t.ns2 = ns2;
    t.lds = base;
    plan_tile(t, sn1, sn2, g.L);
    p.lds.tiled = base;
    p.part_slots = std::max(p.part_slots, 2 * ns1 * ns2); // … and the tiled kernel's partials: two sets per window
    t.ok = true;
}

// Everything the tracker derives from its geometry, its switches and the pinned variant id (`forced`, or -1): the batch kernel
// and its strips, the refinement's geometry, the fused and tiled kernels' plans, the two-pass task sizes, part_slots — and the
// LDS limit of every kernel those may launch.  pdog_create, pdog_set_variant and the pdog_set_tuning keys that change an input
// call this, then apply_plan (pawsome_dog.hip), and nothing else; no caller patches a derived field.  A variant that does not
// fit is refused (PDOG_E_ARG, the text in *why) and *out stays as it was.
// Kernel lengths with a roll instance: l = 17 … 149 (dog_roll.hpp, roll_lengths.def; l = 101 … 149 at two waves per SIMD,
// without spills); longer kernels take the two-pass path.
inline int make_plan(const Geometry &g, const Switches &sw, int forced, Plan *out, std::string *why)
{
    Plan p;
    p.geo = g;
    p.fused = plan_fused(g, sw);
    const VariantShape *best = nullptr;
    double best_cost = 0;
    for (const VariantShape &v : kVariantShapes) {
        if (forced >= 0 && v.id != forced) continue;
        if (v.family == Family::Fused) { // never the tracker's batch kernel unless forced; small batches and chains reach it below
            if (forced == v.id && p.fused.ok) best = &v;
            continue;
        }
        if (v.LT != 0 && v.LT != g.L) continue;
        if (v.lds(g.L) > kMaxLds) continue;
        const bool roll_serves = has_roll_instance(g.L);
        if (forced < 0 && g.L >= ROLL_LMIN && !roll_serves && v.family != Family::TwoPass) continue; // long kernels without a roll instance: two-pass path (measured 1.7× the ring kernel at l = 293)
        if (v.family == Family::TwoPass) {
            const size_t hl = (size_t)HP_ROWS * twopass_pitch(g.n1, g.L) * 8;
            if (hl > kMaxLds - 1024) continue;
            if (forced < 0 && (roll_serves || g.L < ROLL_LMIN)) continue; // the ring/roll kernels win where a spill-free roll instance exists
            if (!best || forced >= 0) { best = &v; best_cost = 0.0; }
            continue;
        }
        // crude cost: columns computed × per-column efficiency guess; compile-time L wins
        const int strips = (g.n2 + v.tw() - 1) / v.tw();
        double cost = (double)strips * v.tw() * (v.LT ? 1.0 : 1.6);
        if (v.lds(g.L) > kMaxLds / 2) cost *= 1.3; // one workgroup per CU only
        if (v.family == Family::Roll) {
            // barrier-free rolling kernel: ≈2× the ring kernels per column (measured, cfg3); thin
            // remainder columns cost next to nothing
            const int r = g.n2 % v.tw();
            const int cols = (g.n2 > v.tw() && r > 0 && r <= kThinMax) ? g.n2 - r : strips * v.tw();
            cost = 0.5 * cols;
        }
        if (!best || cost < best_cost) { best = &v; best_cost = cost; }
    }
    if (!best) { *why = "no kernel specialisation fits this target_width/window (LDS)"; return PDOG_E_ARG; }
    p.shape = best;
    p.nstrips = (g.n2 + best->tw() - 1) / best->tw();
    p.forced = forced >= 0;
    // Exact mode's refinement (dog_exact.hpp) works on blocks of `cbw` window columns whose row-pass result (two doubles
    // per element in the Float64 stage) fits ≈24 KB of LDS; the block's pixels go through an LDS tile — all n1 + l − 1 rows
    // resident when that fits 100 KB in total (l ≲ 150: a candidate's exact chain then reads LDS), otherwise ≈24 KB slices.
    const int NA = g.n1 + g.L - 1;
    p.ref_cbw = std::max(1, std::min({8, g.n2, (int)(24576 / ((size_t)NA * 16))}));
    p.ref_rows = refine_lds_bytes(g.n1, g.L, p.ref_cbw, NA) <= 100 * 1024 ? NA : refine_slice_rows(NA, g.L, p.ref_cbw, 24576);
    // (the finishing kernel's limit is raised for the refinement's block whether exact mode is on or not)
    p.lds.finish = refine_lds_bytes(g.n1, g.L, p.ref_cbw, p.ref_rows);
    if (p.fused.ok) p.lds.fused = p.fused.lds;
    plan_tiled(p, sw);
    if (best->family == Family::Fused) {
        p.nstrips = 1;
        *out = p;
        return PDOG_OK;
    }
    {
        // The two-pass kernels spread one window over dozens of workgroups, so they win whenever the batch
        // cannot fill the GPU with one wave per strip (single-frame tracking: 36 µs vs 144 µs for one
        // 257×257 window).  Set them up whenever their LDS tiles fit.
        p.tp_ph1 = sw.tp_ph1 ? sw.tp_ph1 : pick_h1_outputs(g.n2);
        p.tp_php = sw.tp_php ? sw.tp_php : pick_hpass_outputs(g.n1);
        const size_t hl = (size_t)HP_ROWS * twopass_pitch(g.n1, g.L) * 8;
        const size_t h1l = (size_t)HP_ROWS * twopass_pitch_q(g.n2, g.L, 16 * p.tp_ph1) * sizeof(float);
        const size_t hl8 = (size_t)8 * twopass_pitch_q(g.n1, g.L, 32 * p.tp_php) * 8;
        if (hl <= kMaxLds - 1024 && h1l <= kMaxLds - 1024 && hl8 <= kMaxLds - 1024) {
            p.lds.tp_col16 = hl;
            p.lds.tp_col8 = hl8;
            p.lds.tp_row = h1l;
            p.small_twopass = true;
        }
    }
    if (best->family == Family::TwoPass) {
        p.nstrips = (g.n2 + HP_ROWS - 1) / HP_ROWS; // partial slots = 16-column blocks
        if (!p.small_twopass) { *why = "two-pass kernels: the window's rows do not fit LDS"; return PDOG_E_ARG; }
        *out = p;
        return PDOG_OK;
    }
    if (best->full_set && g.n2 > best->tw()) {
        // width = 64·k + r: r ≤ kThinMax columns are cheaper one by one than as an extra strip
        const int r = g.n2 % best->tw();
        const size_t thin_lds = thin_lds_bytes(g.n1, g.L);
        if (r > 0 && r <= kThinMax && thin_lds <= kMaxLds - 1024) {
            p.lds.thin = thin_lds;
            p.nthin = r;
            p.thin_x0 = g.n2 - r;
            p.nstrips = p.thin_x0 / best->tw();
        }
    }
    p.lds.batch = best->lds(g.L);
    *out = p;
    return PDOG_OK;
}

// exact mode needs the refinement's smallest block in the finishing kernel's LDS (n1 + l up to ≈9000 rows)
inline bool exact_fits(const Geometry &g) { return refine_lds_bytes(g.n1, g.L, 1, 8) <= kMaxLds - 8192; }

// Which kernel family a batch of n windows runs on (kPathFused, kPathTiled, kPathTwoPass, otherwise the tracker's
// batch kernel).  A batch of fewer than ≈1000 strip-waves cannot fill 256 CUs × 8 waves with one wave per strip:
// windows that fit in LDS then go to the fused kernel (one workgroup per window, one launch), larger ones to the
// two-pass kernels (dozens of workgroups per window).  pdog_set_variant pins the tracker's kernel.
inline int path_for_batch(const Plan &p, const Switches &sw, int n)
{
    const VariantShape &v = *p.shape;
    const bool twopass = v.family == Family::TwoPass;
    if (v.family == Family::Fused) return kPathFused;
    if (p.forced) return twopass ? kPathTwoPass : v.id;
    // (round 3, with the compile-time-l fused instances: 45×45 windows 1024 / 1536 / 2048 per batch: fused 53.8 / 77.3 / 101.9 µs, roll 79.2 / 75.7 / 103.6;
    // 63×63: 80.9 / 117.5 / 155.8 against 91.6 / 88.7 / 117.2)
    // (… and since a workgroup of the fused kernel walks several windows — dispatch, prologue and first tap loads once per workgroup — 45×45 windows:
    // 1024 / 2048 / 4096 per batch 44.5 / 83 / 155 µs against the roll kernel's 79 / 103 / 163: windows below 3000 pixels stay on it at any batch size)
    const bool few = twopass ? n <= 256 : ((long long)n * (p.nstrips + (p.nthin ? 1 : 0)) < 1200 || (long long)p.geo.n1 * p.geo.n2 < 3000);
    if (sw.tiled_force && p.tiled.ok && n <= sw.tiled_batch) return kPathTiled; // experiment switch
    if (few && p.fused.ok) return kPathFused;
    if (p.tiled.ok && n <= sw.tiled_batch) return kPathTiled; // one or two windows too large for the fused kernel: one launch (dog_tiled.hpp)
    if (twopass || (few && p.small_twopass)) return kPathTwoPass;
    return v.id;
}

// What launch_tiled takes: n windows, or n clips of chain_len > 1 frames with every sub-window's workgroup resident at once
// (`resident`: the workgroups of the tiled kernel the device keeps resident, apply_plan's question; 0 without cooperative launches).
inline bool tiled_serves(const Plan &p, int resident, int n, int chain_len)
{
    return p.tiled.ok && n >= 1 && (chain_len <= 1 || (long long)n * p.tiled.ns1 * p.tiled.ns2 <= resident);
}

inline int chain_strips(const Geometry &g) { return (g.n2 + ROLL_TW - 1) / ROLL_TW; }

// What a chain runs on: a kernel that walks its clips itself, or the stepped walk, a batch per step.
enum class ChainPath { Fused, Persistent, Tiled, Stepped };

// n_clips clips of n_steps steps, contiguous or over a table; progress: one clip whose kernel publishes k + 1 after frame k.
inline ChainPath chain_path(const Plan &p, const Switches &, int tiled_resident, int n_clips, int n_steps, bool table, bool progress)
{
    const VariantShape &v = *p.shape;
    // a table of one step is no chain for the kernels that walk a clip themselves (their chain_len = 1 means independent windows)
    if (table && n_steps == 1) return ChainPath::Stepped;
    // Enough clips to fill the GPU with one wave per strip → ONE persistent launch (a workgroup per clip walks
    // its frames).  Fewer clips are latency-bound by that single wave per strip; then each frame is a small
    // batch that the two-pass kernels spread over many workgroups (21 µs vs 48 µs per frame, one 45×45 window).
    // (round 3: the fused kernel's compile-time-l instances walk 256 … 4096 clips of 45×45 windows at 27–30 M frames/s, the persistent
    // roll chain 19–28 M; at 63×63 the chain wins from ≈1400 clips: 23.5 against 18.0 M frames/s at 2048)
    const long long strip_waves = (long long)n_clips * chain_strips(p.geo);
    const bool fused_wins = p.fused.ok && !p.forced && ((long long)p.geo.n1 * p.geo.n2 < 3000 || strip_waves < 1400);
    const bool persistent = !progress && v.full_set && chain_strips(p.geo) <= 8 && !fused_wins && // (the chain kernel publishes no progress)
                            (p.forced || !p.small_twopass || strip_waves >= 1000);
    if (v.family == Family::Fused || (!persistent && !p.forced && p.fused.ok)) return ChainPath::Fused; // one launch: a workgroup per clip loops over its frames
    if (persistent) return ChainPath::Persistent;
    // the tiled kernel: one cooperative launch, every sub-window's workgroup of every clip resident (as many clips as that
    // allows); with progress its combining workgroup publishes k + 1 after every frame
    if (!p.forced && tiled_serves(p, tiled_resident, n_clips, n_steps)) return ChainPath::Tiled;
    return ChainPath::Stepped;
}

// ---- exact mode's FP32 error bounds: exact_factors (pdog_math.cpp) per kernel family, and here ----
enum KernelFamily : int { kFamRoll, kFamRing, kFamFused, kFamTwoPass8, kFamTwoPass16 };
// the family of the tracker's batch kernel (small batches may run another family with a tighter bound)
inline KernelFamily batch_family(const VariantShape &v)
{
    return v.family == Family::Roll ? kFamRoll : v.family == Family::TwoPass ? kFamTwoPass8 : v.family == Family::Fused ? kFamFused : kFamRing;
}
// the two-pass kernels' factor for the plan's task sizes (hr8: the 8-row column-pass kernels, else the 16-row form <13, 16>);
// F_sym_sep: exact_factors' factor of the plain instances; gp, gm: the two Float64 Gaussians
inline double twopass_factor(const Plan &p, const Switches &sw, bool hr8, double F_sym_sep, const std::vector<double> &gp, const std::vector<double> &gm)
{
    if (!hr8 || p.geo.L < TWOPASS_FLUSH_L) return F_sym_sep; // the plain instances: symmetric row pass, separate column chains
    const int l = p.geo.L, H = l / 2;
    const int U1 = sw.h1_u, m_r = twopass_ring(p.tp_ph1, U1), U2 = hr8 ? sw.hp_u : 16, m_c = hr8 ? twopass_ring(p.tp_php, U2) : twopass_ring(13, 16);
    auto blocked = [](const std::vector<double> &terms, int m, int n_full) { // chains of m terms (n_full of them), then ONE chain with the rest
        double F = 0, total = 0;
        const int n = (int)terms.size();
        for (int c = 0, a = 0; c <= n_full; ++c) {
            const int b = c < n_full ? std::min(a + m, n) : n; // (the column pass's last full trip may end in the table's zero padding: l = 113, 117, 137, …)
            double w = 0;
            for (int i = a; i < b; ++i) { w += terms[i]; F += w; } // the chain's own running sums, from zero
            total += w;
            F += total;                                             // the addition that takes the chain's sum into the running total
            a = b;
        }
        return F;
    };
    auto row = [&](const std::vector<double> &g) {
        std::vector<double> terms(H + 1);
        for (int k = 0; k <= H; ++k) terms[k] = (k < H ? 2.0 : 1.0) * g[k];
        return blocked(terms, m_r, (H / U1) / (m_r / U1)) + 1.0;
    };
    auto col = [&](const std::vector<double> &g) { return blocked(g, m_c, ((l + U2 - 1) / U2) / (m_c / U2)); };
    return row(gp) + row(gm) + col(gp) + col(gm) + 4.0;
}
// the factor of a kernel family's bound: exact_factors' three (pdog_math.cpp), or the two-pass kernels' own for the plan's task sizes
inline double family_factor(KernelFamily fam, double F_sym_int, double F_sym_sep, double F_ring, const Plan &p, const Switches &sw,
                            const std::vector<double> &gp, const std::vector<double> &gm)
{
    return fam == kFamRoll ? F_sym_int : fam == kFamRing ? F_ring : fam == kFamFused ? F_sym_sep : twopass_factor(p, sw, fam == kFamTwoPass8, F_sym_sep, gp, gm);
}
// The thresholds a kernel family flags with: T = 2δ between a window's two best FP32 responses, T_rescan for the finishing
// kernel's rescan; F: the family's factor, F_rescan: exact_factors' rescan factor.  exact_all: infinite, every window is refined.
struct ExactThresholds {
    float T, T_rescan;
};
inline ExactThresholds exact_thresholds(double F, double F_rescan, bool exact_all)
{
    const double u = std::ldexp(1.0, -24);
    ExactThresholds x;
    x.T = exact_all ? __builtin_huge_valf() : std::nextafter((float)(2.0 * u * F * 1.02 + 2e-9), 1.0f);
    x.T_rescan = exact_all ? __builtin_huge_valf() : std::nextafter((float)(u * (F + F_rescan) * 1.02 + 2e-9), 1.0f);
    return x;
}

} // namespace pdog
