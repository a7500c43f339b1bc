// pdog_policy.hpp — the two adaptive policies of the roll family's batch path (launch_strips, pawsome_dog.hip) as host-only
// value types: no HIP, no tracker, so the host compiler can test them (tests/policy_main.cpp).  Both read cumulative counts
// that kernels publish through the mailbox (pdog_mailbox.hpp); launch_strips loads the words and hands the values in.
// Nothing here waits for the GPU.
#pragma once
#include <stdint.h>

namespace pdog {

// ---- response-map policy (exact mode on the roll / ring kernels) ----
// A batch whose predecessors flagged more than 1 in kMapOnOneIn (8 %) of their windows writes its responses (the kernels'
// RESP instances: +15 % on the strips) and the finishing kernel reads the candidates off that map instead of recomputing them
// per window; back to the plain instances after kMapCalmRuns observations in a row below 1 in kMapOffOneIn (2 %).  The
// finishing kernels publish the flagged count TOGETHER with the number of windows it came from, so the rate is right however
// many batches are in flight (round 2 compared the count's increase with ONE batch's size: with three batches in flight
// 0.9 % looked like 2.7 % and one step in four paid for a map it did not need).
constexpr int kMapOnOneIn = 12, kMapOffOneIn = 50;
constexpr int kMapCalmRuns = 8;
struct MapPolicy {
    uint32_t flag_last = 0, win_last = 0; // KernelWords::flagged / finished as last seen
    int calm = 0;
    // the published counts as just loaded (the low 32 bits of cumulative counts: differences wrap correctly)
    void observe(uint32_t flagged, uint32_t finished)
    {
        const long long delta = (long long)(uint32_t)(flagged - flag_last), dwin = (long long)(uint32_t)(finished - win_last);
        if (dwin <= 0) return; // no finishing kernel has published since the last look
        flag_last = flagged;
        win_last = finished;
        if (delta * kMapOnOneIn > dwin) { on_ = true; calm = 0; }
        else if (delta * kMapOffOneIn < dwin) { if (++calm >= kMapCalmRuns) on_ = false; }
        else calm = 0;
    }
    bool on() const { return on_; }

private:
    bool on_ = false;
};

// ---- pruning policy (dog_prune.hpp) ----
// The pre-pass pays where it lets the strips skip more than it costs.  Measured on the flagship batch, kernel trace of
// bench.py (profiles/prune_profile_this.txt, profiles/prune_profile_parent.txt): dog_prune_kernel takes 0.474 ms beside the
// dense roll kernel's 1.314 ms, 36 % of it (kPrunePrePct), so a batch that keeps more than 64 % of its (slot, sub-chunk) pairs
// (kPruneBreakEvenPct) is better off dense.  Noise-only windows and heavy texture are such batches (nothing can be excluded).
// (Since the pre-pass forms its energies from raw-pixel moments it takes 0.331 ms, 25 % of the dense roll kernel:
// profiles/prepass_profile_this.txt.  The constant has not followed yet: bench data at ±40 levels keeps 76 % of its pairs,
// right at the share that ratio would give, and whether pruning pays there is unmeasured — profiles/prepass_ab.txt.
// With clamped loads and the next cell's loads in flight: 0.302 ms, 23 % — profiles/prepass_latency_ab.txt.
// With the job list, which the pre-pass also files: 0.306 ms, still 23 % — profiles/compact_ab.txt.
// With the relaxed publish: 0.148 ms, 11 %.  And the ±40-level question is now measured — profiles/publish_ab.txt: with the
// constant at 11 those batches, 76 % kept, run pruned and take 1.510 ms where the dense path takes 1.364.  What decides at such a
// share is the PRUNE instance on three quarters of the sub-chunks against the dense instance on all of them, not the pre-pass:
// the constant stays, and stands for that.)
// The pre-pass publishes its cumulative kept / total counts in one word (Mailbox::prune_pub); when the pairs counted since the
// last look kept more than the break-even share, the next kPruneProbeEvery batches run dense, then one batch probes again.
constexpr int kPrunePrePct = 36;
constexpr int kPruneBreakEvenPct = 100 - kPrunePrePct;
constexpr int kPruneProbeEvery = 64;
struct PrunePolicy {
    uint32_t kept_last = 0, total_last = 0; // the published counts last seen
    int sleep = 0;                          // batches left to run dense before the next probe
    // One eligible batch: `published` is Mailbox::prune_pub as just loaded.  true: run the pre-pass.
    bool decide(uint64_t published)
    {
        const uint32_t kept = (uint32_t)published, total = (uint32_t)(published >> 32); // (low halves of cumulative counts: differences wrap correctly)
        const long long dk = (long long)(uint32_t)(kept - kept_last), dt = (long long)(uint32_t)(total - total_last);
        if (dt > 0) {
            kept_last = kept;
            total_last = total;
            sleep = dk * 100 > dt * kPruneBreakEvenPct ? kPruneProbeEvery : 0;
        }
        if (sleep > 0) { --sleep; return false; }
        return true;
    }
};

} // namespace pdog
