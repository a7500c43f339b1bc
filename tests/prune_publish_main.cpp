// Stand-alone host check of csrc/dog_prune_publish.hpp (tests/test_prune_publish_cpu.py builds and runs it, plain and under
// AddressSanitizer + UBSan): the packed word through which the workgroups of one pre-pass launch meet.  The fetch-adds of a
// batch are run one after the other in a random arrival order — on the device they have a single total order too — and
// what every arriver derives from the returned word is held against the direct sums.  Exit status 1 on any difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <utility>
#include <vector>

#include "dog_prune_publish.hpp"

using namespace pdog;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static long failures = 0, checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { if (++failures <= 20) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// The device's cumulative counters and the host word, as the last arriver of every batch leaves them.
struct Stat {
    uint64_t kept = 0, total = 0, word = 0, host = 0;
    int header = -1;
};

// One batch of n workgroups; kind 0: random counts, 1: every count at its largest, 2: nothing kept anywhere.
static void run_batch(Stat &st, uint32_t n, int nstrips, int nslots, int nsub, int kind)
{
    CHECK(pp_fits(n, nstrips, nslots, nsub), "n=%u nstrips=%d nslots=%d nsub=%d", n, nstrips, nslots, nsub);
    std::vector<uint32_t> njobs(n), kept(n), order(n);
    for (uint32_t b = 0; b < n; ++b) {
        njobs[b] = kind == 1 ? (uint32_t)nstrips : kind == 2 ? 0u : rnd() % (uint32_t)(nstrips + 1);
        kept[b] = kind == 1 ? (uint32_t)(nslots * nsub) : kind == 2 ? 0u : rnd() % (uint32_t)(nslots * nsub + 1);
    }
    std::iota(order.begin(), order.end(), 0u);
    for (uint32_t i = n; i > 1; --i) std::swap(order[i - 1], order[rnd() % i]);
    const uint64_t sum_jobs = std::accumulate(njobs.begin(), njobs.end(), (uint64_t)0), sum_kept = std::accumulate(kept.begin(), kept.end(), (uint64_t)0);

    CHECK(st.word == 0, "the word is zero when a batch starts: %llx", (unsigned long long)st.word);
    uint64_t next_base = 0;
    uint32_t lasts = 0;
    const uint64_t kept_before = st.kept, total_before = st.total;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t b = order[i];
        const uint64_t returned = st.word; // the fetch-add
        st.word += pp_increment(njobs[b], kept[b]);
        const PpArrival a = pp_arrive(returned, njobs[b], kept[b], n);
        // the bases partition [0, Σ njobs) in arrival order
        CHECK(a.base == next_base, "arrival %u: base %u, want %llu", i, a.base, (unsigned long long)next_base);
        next_base += njobs[b];
        CHECK(a.last == (i == n - 1), "arrival %u of %u: last %d", i, n, (int)a.last);
        CHECK(pp_arrivals(st.word) == i + 1 && pp_jobs(st.word) == next_base, "arrival %u: the word's fields %u %u", i, pp_arrivals(st.word), pp_jobs(st.word));
        if (a.last) {
            ++lasts;
            CHECK(a.jobs == sum_jobs && a.kept == sum_kept, "the last arriver's sums %u %u, direct %llu %llu", a.jobs, a.kept, (unsigned long long)sum_jobs,
                  (unsigned long long)sum_kept);
            // what it publishes (dog_prune.hpp, the publish block)
            st.word = 0;
            const uint64_t total = (uint64_t)n * (uint64_t)(nslots * nsub);
            const uint64_t k = st.kept + a.kept, t = st.total + total; // the two returning adds
            st.kept = k;
            st.total = t;
            st.host = pp_host_word(k, t);
            st.header = (int)a.jobs;
        }
    }
    CHECK(lasts == 1, "%u arrivers saw n - 1 arrivals", lasts);
    CHECK(next_base == sum_jobs, "the bases end at %llu of %llu", (unsigned long long)next_base, (unsigned long long)sum_jobs);
    CHECK(st.word == 0, "the word is zero again");
    CHECK(st.kept == kept_before + sum_kept && st.total == total_before + (uint64_t)n * nslots * nsub, "cumulative counts");
    CHECK((uint32_t)st.host == (uint32_t)st.kept && (st.host >> 32) == (st.total & 0xffffffffull), "host word %llx", (unsigned long long)st.host);
    CHECK(st.header == (int)sum_jobs, "list header %d of %llu", st.header, (unsigned long long)sum_jobs);
}

int main()
{
    // ---- the fields ----
    const uint64_t amax = (1ull << PP_ARRIVAL_BITS) - 1, jmax = (1ull << PP_JOB_BITS) - 1, kmax = (1ull << PP_KEPT_BITS) - 1;
    {
        const uint64_t w = pp_pack(amax, jmax, kmax);
        CHECK(w == ~0ull, "%llx", (unsigned long long)w);
        CHECK(pp_arrivals(w) == amax && pp_jobs(w) == jmax && pp_kept(w) == kmax, "largest fields");
        for (int f = 0; f < 3; ++f) { // each field alone at its largest: the neighbours read zero
            const uint64_t v = pp_pack(f == 0 ? amax : 0, f == 1 ? jmax : 0, f == 2 ? kmax : 0);
            CHECK(pp_arrivals(v) == (f == 0 ? amax : 0) && pp_jobs(v) == (f == 1 ? jmax : 0) && pp_kept(v) == (f == 2 ? kmax : 0), "field %d alone", f);
        }
        CHECK(pp_increment(3, 700) == (1ull | (3ull << 20) | (700ull << 40)), "the increment's layout");
    }
    // ---- the fit test: the largest fitting value of each bound, and one past it ----
    CHECK(pp_fits(4096, 4, 5, 41), "cfg3");
    CHECK(pp_fits((1 << 20) - 1, 1, 1, 1) && !pp_fits(1 << 20, 1, 1, 1), "arrivals");
    CHECK(pp_fits(349525, 3, 3, 1) && !pp_fits(262144, 4, 4, 1) && !pp_fits(349526, 3, 3, 1), "jobs");        // 3 · 349525 = 2^20 − 1
    CHECK(pp_fits(4095, 16, 17, 241) && !pp_fits(4096, 4, 4, 1024) && !pp_fits(4095, 16, 17, 242), "kept pairs"); // 4095 · 17 · 241 = 2^24 − 1
    CHECK(!pp_fits(0, 1, 1, 1) && !pp_fits(1ll << 40, 1ll << 30, 1ll << 30, 8), "no windows; products beyond 32 bits");

    // ---- arrivals in random order ----
    Stat st;
    for (int trial = 0; trial < 400; ++trial) {
        const int nstrips = 1 + (int)(rnd() % 8), nslots = nstrips + (int)(rnd() % 4), nsub = 1 + (int)(rnd() % 60);
        const uint32_t n = trial < 8 ? (uint32_t)trial + 1 : 1 + rnd() % 3000;
        run_batch(st, n, nstrips, nslots, nsub, trial % 7 == 3 ? 1 : trial % 11 == 5 ? 2 : 0);
    }
    run_batch(st, 4096, 4, 5, 41, 0); // cfg3
    run_batch(st, 4096, 4, 5, 41, 1);
    // every field at its largest fitting sum, every workgroup at its largest count: nothing carries
    run_batch(st, (1u << 20) - 1, 1, 1, 16, 1);  // arrivals and jobs 2^20 − 1, pairs 2^24 − 16
    run_batch(st, 349525, 3, 3, 16, 1);          // jobs 2^20 − 1, pairs 2^24 − 16
    run_batch(st, 4095, 16, 17, 241, 1);         // pairs 2^24 − 1
    // the cumulative kept count past 32 bits: the host word keeps its low half, the total's low half above it
    {
        Stat big;
        big.kept = 0xfffffff0ull;
        big.total = 0x1fffffff0ull;
        run_batch(big, 100, 2, 3, 41, 1);
        CHECK(big.kept > 0xffffffffull && (uint32_t)big.host == (uint32_t)big.kept, "kept past 32 bits");
    }

    std::printf("%ld checks, %ld mismatches\n", checks, failures);
    return failures ? 1 : 0;
}
