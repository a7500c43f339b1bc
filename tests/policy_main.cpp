// Stand-alone host check of csrc/pdog_policy.hpp and csrc/pdog_mailbox.hpp (tests/test_policy_cpu.py builds and runs it, plain
// and under AddressSanitizer + UBSan).  The two rules are stated a second time here, over 64-bit cumulative counts and with
// their figures written out (1 in 12, 1 in 50, eight calm looks; 64 %, 64 dense batches), and compared call by call with
// MapPolicy / PrunePolicy, which only ever see the low 32 bits as a Mailbox carries them: over fixed sequences (each also
// checked against the answer written beside it) and over seeded random ones.  Exit status 1 on any difference.
#include <cstdint>
#include <cstdio>

#include "pdog_mailbox.hpp"
#include "pdog_policy.hpp"

using namespace pdog;

static long failures = 0, checks = 0;
static void expect(bool ok, const char *what, long step = -1)
{
    ++checks;
    if (ok) return;
    if (++failures <= 20) std::printf("MISMATCH %s (step %ld)\n", what, step);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// ---- the response-map rule, restated ----
// Since the last look that saw new windows: more than one window in 12 flagged → on; fewer than one in 50, eight such looks in
// a row → off; anything between starts the row again.  A look that sees no new window changes nothing.
struct MapModel {
    uint64_t flagged_seen = 0, windows_seen = 0;
    int calm_looks = 0;
    bool on = false;
    void look(uint64_t flagged, uint64_t windows)
    {
        if (windows == windows_seen) return;
        const uint64_t f = flagged - flagged_seen, w = windows - windows_seen;
        flagged_seen = flagged;
        windows_seen = windows;
        if (12 * f > w) {
            on = true;
            calm_looks = 0;
        } else if (50 * f < w) {
            calm_looks += 1;
            if (calm_looks >= 8) on = false;
        } else
            calm_looks = 0;
    }
};

// The finishing kernels' side and the host's, with the mailbox between them.
struct MapRig {
    uint64_t flagged, windows; // cumulative, 64-bit
    Mailbox box{};
    MapPolicy policy;
    MapModel model;
    explicit MapRig(uint64_t start = 0) : flagged(start), windows(start)
    {
        box.kernel.flagged = policy.flag_last = (uint32_t)start; // a tracker that has come this far
        box.kernel.finished = policy.win_last = (uint32_t)start;
        model.flagged_seen = model.windows_seen = start;
    }
    void batch(uint64_t n_flagged, uint64_t n_windows) // one finishing kernel publishes
    {
        flagged += n_flagged;
        windows += n_windows;
        box.kernel.flagged = (uint32_t)flagged;
        box.kernel.finished = (uint32_t)windows;
    }
    bool look(long step = -1) // launch_strips
    {
        policy.observe(box.kernel.flagged, box.kernel.finished);
        model.look(flagged, windows);
        expect(policy.on() == model.on, "MapPolicy::on against the restated rule", step);
        expect(policy.calm == model.calm_looks, "MapPolicy::calm against the restated rule", step);
        expect(policy.flag_last == (uint32_t)model.flagged_seen && policy.win_last == (uint32_t)model.windows_seen, "MapPolicy's last-seen counts", step);
        return policy.on();
    }
};

static void map_fixed()
{
    { // 1. nothing finished: any number of looks changes nothing, on or off, whatever `flagged` shows
        MapRig r;
        for (int i = 0; i < 100; ++i) { r.box.kernel.flagged = rnd(); r.look(); }
        expect(!r.policy.on() && r.policy.calm == 0 && r.policy.flag_last == 0 && r.policy.win_last == 0, "map 1: idle looks, off");
        r.box.kernel.flagged = 0;
        r.batch(50, 100);
        expect(r.look(), "map 1: 50 of 100 turns it on");
        r.batch(1, 100);
        r.look();
        const MapPolicy before = r.policy;
        for (int i = 0; i < 100; ++i) r.look();
        expect(r.policy.on() && r.policy.calm == before.calm && r.policy.flag_last == before.flag_last && r.policy.win_last == before.win_last, "map 1: idle looks, on");
    }
    { // 2. 8 of 100 leaves it off, 9 of 100 turns it on
        MapRig a, b;
        a.batch(8, 100);
        expect(!a.look(), "map 2: 8 of 100 stays off");
        b.batch(9, 100);
        expect(b.look(), "map 2: 9 of 100 turns on");
    }
    { // 3. on: seven looks at 1 of 100 leave it on, the eighth turns it off
        MapRig r;
        r.batch(100, 100);
        expect(r.look(), "map 3: on");
        for (int i = 1; i <= 8; ++i) {
            r.batch(1, 100);
            expect(r.look() == (i < 8), "map 3: off at the eighth calm look exactly", i);
        }
    }
    { // 4. a look at 2 of 100 among them starts the count again
        MapRig r;
        r.batch(100, 100);
        r.look();
        for (int i = 1; i <= 7; ++i) { r.batch(1, 100); expect(r.look(), "map 4: still on", i); }
        r.batch(2, 100);
        expect(r.look() && r.policy.calm == 0, "map 4: 2 of 100 restarts");
        for (int i = 1; i <= 8; ++i) {
            r.batch(1, 100);
            expect(r.look() == (i < 8), "map 4: eight more calm looks", i);
        }
    }
    { // 5. both counts cross 2^32 between two looks (last seen 0xFFFFFFF0, now 0x10)
        MapRig r(0xFFFFFFF0ull);
        r.batch(0x20, 0x20);
        expect(r.box.kernel.flagged == 0x10u && r.box.kernel.finished == 0x10u, "map 5: the words wrapped");
        expect(r.look(), "map 5: 32 of 32 across the wrap turns on");
        MapRig q(0xFFFFFFF0ull);
        q.batch(2, 0x20); // (flagged stays below 2^32, finished crosses it)
        expect(!q.look() && q.policy.calm == 0, "map 5: 2 of 32 across the wrap is neither");
        MapRig c(0xFFFFFFF0ull);
        c.batch(0, 0x20);
        expect(!c.look() && c.policy.calm == 1, "map 5: 0 of 32 across the wrap is calm");
    }
    { // 6. one look covers three batches: the rate is taken over all their windows
        MapRig r;
        for (int k = 0; k < 3; ++k) r.batch(1, 100); // 0.9 % flagged with three batches in flight: against ONE batch's size it looked like 2.7 %
        expect(!r.look() && r.policy.calm == 1, "map 6: 3 of 300 is calm");
        for (int k = 0; k < 3; ++k) r.batch(3, 100); // 9 of 300: 9 of ONE batch's 100 would turn it on
        expect(!r.look() && r.policy.calm == 0, "map 6: 9 of 300 stays off");
        for (int k = 0; k < 3; ++k) r.batch(9, 100);
        expect(r.look(), "map 6: 27 of 300 turns on");
    }
}

static void map_random(uint32_t seed, uint64_t start)
{
    rng_state = seed * 0x2545F4914F6CDD1Dull + 1;
    MapRig r(start);
    for (long step = 0; step < 20000; ++step) {
        const int batches = rnd() % 4; // 0: a look with nothing new
        const uint32_t regime = (rnd() >> 8) % 5;
        for (int k = 0; k < batches; ++k) {
            const uint64_t n = 1 + rnd() % ((rnd() & 15) == 0 ? 3000000u : 5000u);
            int64_t f = 0;
            switch (regime) {
            case 0: f = 0; break;
            case 1: f = (int64_t)(n / 50) + (int64_t)(rnd() % 3) - 1; break; // around the lower threshold
            case 2: f = (int64_t)(n / 12) + (int64_t)(rnd() % 3) - 1; break; // around the upper threshold
            case 3: f = (int64_t)n; break;
            default: f = (int64_t)(rnd() % (n + 1)); break;
            }
            if (f < 0) f = 0;
            if (f > (int64_t)n) f = (int64_t)n;
            r.batch((uint64_t)f, n);
        }
        r.look(step);
    }
}

// ---- the pruning rule, restated ----
// Each eligible batch: if the pre-pass has published since the last look and the pairs counted since then kept more than 64 in
// 100, the next 64 batches (this one included) run dense; a publication with a lower share ends that at once.
struct PruneModel {
    uint64_t kept_seen = 0, total_seen = 0;
    int dense_left = 0;
    bool batch(uint64_t kept, uint64_t total)
    {
        if (total != total_seen) {
            const uint64_t k = kept - kept_seen, t = total - total_seen;
            kept_seen = kept;
            total_seen = total;
            dense_left = 100 * k > 64 * t ? 64 : 0;
        }
        if (dense_left == 0) return true;
        dense_left -= 1;
        return false;
    }
};

struct PruneRig {
    uint64_t kept, total;
    Mailbox box{};
    PrunePolicy policy;
    PruneModel model;
    explicit PruneRig(uint64_t kept0 = 0, uint64_t total0 = 0) : kept(kept0), total(total0)
    {
        policy.kept_last = (uint32_t)kept0;
        policy.total_last = (uint32_t)total0;
        model.kept_seen = kept0;
        model.total_seen = total0;
        box.prune_pub = (kept0 & 0xffffffffull) | (total0 << 32);
    }
    void publish(uint64_t k, uint64_t t) // one pre-pass finishes: one 64-bit store
    {
        kept += k;
        total += t;
        box.prune_pub = (kept & 0xffffffffull) | (total << 32);
    }
    bool batch(long step = -1)
    {
        const bool got = policy.decide(box.prune_pub), want = model.batch(kept, total);
        expect(got == want, "PrunePolicy::decide against the restated rule", step);
        expect(policy.sleep == model.dense_left, "PrunePolicy::sleep against the restated rule", step);
        return got;
    }
};

static void prune_fixed()
{
    static_assert(kPruneProbeEvery == 64 && kPruneBreakEvenPct == 64 && kPrunePrePct == 36, "the figures this file writes out");
    { // 1. no publication: every batch prunes
        PruneRig r;
        for (int i = 0; i < 200; ++i) expect(r.batch(), "prune 1: no publication", i);
    }
    { // 2. 64 of 100 keeps pruning; 65 of 100 answers dense for exactly kPruneProbeEvery batches, that one included, then probes
        PruneRig a;
        a.publish(64, 100);
        expect(a.batch(), "prune 2: 64 of 100 prunes");
        PruneRig b;
        b.publish(65, 100);
        for (int i = 1; i <= kPruneProbeEvery; ++i) expect(!b.batch(), "prune 2: dense while asleep", i);
        expect(b.batch(), "prune 2: the probe after kPruneProbeEvery dense batches");
        expect(b.batch(), "prune 2: and on, until the probe publishes");
    }
    { // 3. a publication with a low share that arrives while asleep wakes it at once
        PruneRig r;
        r.publish(90, 100);
        for (int i = 0; i < 10; ++i) expect(!r.batch(), "prune 3: asleep", i);
        r.publish(10, 100); // (a pre-pass that was in flight)
        expect(r.batch() && r.policy.sleep == 0, "prune 3: awake at once");
    }
    { // 4. both 32-bit halves wrap
        PruneRig r(0xFFFFFFF0ull, 0xFFFFFFF8ull);
        r.publish(0x20, 0x40); // kept 0x10, total 0x38 in the word: 32 of 64
        expect((uint32_t)r.box.prune_pub == 0x10u && (uint32_t)(r.box.prune_pub >> 32) == 0x38u, "prune 4: the halves wrapped");
        expect(r.batch(), "prune 4: 32 of 64 across the wrap prunes");
        PruneRig q(0xFFFFFFF0ull, 0xFFFFFFF8ull);
        q.publish(0x30, 0x40);
        expect(!q.batch() && q.policy.sleep == kPruneProbeEvery - 1, "prune 4: 48 of 64 across the wrap sleeps");
    }
}

static void prune_random(uint32_t seed, uint64_t kept0, uint64_t total0)
{
    rng_state = seed * 0x2545F4914F6CDD1Dull + 7;
    PruneRig r(kept0, total0);
    for (long step = 0; step < 20000; ++step) {
        if (rnd() % 3 == 0) { // a pre-pass finished since the last batch (sometimes two)
            for (int k = 1 + (rnd() % 5 == 0); k > 0; --k) {
                const uint64_t t = 1 + rnd() % ((rnd() & 15) == 0 ? 40000000u : 70000u);
                const uint32_t regime = rnd() % 4;
                uint64_t kk = regime == 0 ? t : regime == 1 ? t * 64 / 100 + (rnd() % 3) : regime == 2 ? t / 3 : rnd() % (t + 1);
                if (kk > t) kk = t;
                r.publish(kk, t);
            }
        }
        r.batch(step);
    }
}

int main()
{
    map_fixed();
    prune_fixed();
    for (uint32_t seed = 1; seed <= 8; ++seed) {
        map_random(seed, seed & 1 ? 0 : 0xFFFFFFFFull - 1000 * seed); // (every other run starts just below 2^32)
        prune_random(seed, seed & 1 ? 0 : 0xFFFFFFFFull - 700 * seed, seed & 1 ? 0 : 0xFFFFFFFFull - 300 * seed);
    }
    std::printf("%ld checks, %ld mismatches\n", checks, failures);
    return failures ? 1 : 0;
}
