// Stand-alone host check of csrc/pdog_plan.hpp (tests/test_plan_cpu.py builds and runs it, plain and under AddressSanitizer +
// UBSan; linked with csrc/pdog_math.cpp for the reference's Float64 arithmetic).  Two modes:
//
//   plan_main replay FH FW TARGET_WIDTH WIN_H WIN_W BATCHES CALL…
//       What pdog_create and then each call — v:ID (pdog_set_variant) or t:KEY:VALUE (pdog_set_tuning) — leave of the plan,
//       through make_plan / path_for_batch / exact_thresholds as pawsome_dog.hip goes through them: after creation and after
//       each call one line, the snapshot tests/test_gpu_dispatch.py takes of a tracker on the GPU,
//       [status, variant, n_strips, strip_w, exact on, threshold, [path per batch size]] (BATCHES: the sizes, comma-separated).
//       The device has one say in this: a dynamic-LDS request beyond the CU's LDS is refused (hipFuncSetAttribute,
//       PDOG_E_HIP).  Here that is "a request of the plan exceeds kMaxLds": a creation that meets it prints [2] and nothing
//       more, a later call answers 2 and leaves the plan as it was.
//   plan_main check FH FW TARGET_WIDTH WIN_H WIN_W
//       chain_path against its rule stated a second time below, over a grid of clip counts, step counts, table / progress and
//       resident counts, for the case's plan as created and pinned; tiled_serves on either side of n · ns1 · ns2 = resident;
//       what Plan::part_slots has to hold; and two facts plan_tiled's comment states.  "N checks, 0 mismatches", exit status
//       1 on any difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pdog_host.hpp" // sigma_of, kernel_len_of_sigma, gaussian_1d, exact_factors (pdog_math.cpp)
#include "pdog_plan.hpp"

using namespace pdog;

namespace {

// the part of a tracker the plan and its observers read
struct Model {
    Geometry geo;
    Switches sw;
    Plan plan;
    bool exact = false;
    std::vector<double> gp, gm;
    ExactFactors ef{};
};

bool device_refuses(const Plan &p)
{
    for (size_t bytes : {p.lds.fused, p.lds.tiled, p.lds.tp_col16, p.lds.tp_col8, p.lds.tp_row, p.lds.thin, p.lds.batch, p.lds.finish})
        if (bytes > kMaxLds) return true;
    return false;
}

// make_plan, then what apply_plan can answer without a device
int replan(Model &m, const Switches &sw, int forced)
{
    Plan p;
    std::string why;
    if (int rc = make_plan(m.geo, sw, forced, &p, &why)) return rc;
    if (device_refuses(p)) return PDOG_E_HIP;
    m.sw = sw;
    m.plan = p;
    return PDOG_OK;
}

Geometry geometry(char **a, double *target_width)
{
    Geometry g;
    g.fh = std::atoi(a[0]);
    g.fw = std::atoi(a[1]);
    *target_width = std::atof(a[2]);
    g.n1 = 2 * (std::atoi(a[3]) / 2) + 1;
    g.n2 = 2 * (std::atoi(a[4]) / 2) + 1;
    g.L = kernel_len_of_sigma(sigma_of(*target_width));
    return g;
}

int create(Model &m, char **a)
{
    double tw = 0;
    m.geo = geometry(a, &tw);
    if (int rc = replan(m, Switches(), -1)) return rc;
    const double sigma = sigma_of(tw);
    m.gp.resize(m.geo.L);
    m.gm.resize(m.geo.L);
    gaussian_1d(sigma, m.geo.L, m.gp.data());
    gaussian_1d(sigma * std::sqrt(2.0), m.geo.L, m.gm.data());
    m.ef = exact_factors(m.gp, m.gm);
    m.exact = exact_fits(m.geo);
    return PDOG_OK;
}

void snapshot(const Model &m, int status, const std::vector<int> &batches)
{
    const double F = family_factor(batch_family(*m.plan.shape), m.ef.sym_int, m.ef.sym_sep, m.ef.ring, m.plan, m.sw, m.gp, m.gm);
    std::printf("[%d,%d,%d,%d,%s,%.17g,[", status, m.plan.shape->id, m.plan.nstrips, m.plan.shape->tw(), m.exact ? "true" : "false",
                (double)exact_thresholds(F, m.ef.rescan, false).T);
    for (size_t i = 0; i < batches.size(); ++i) std::printf("%s%d", i ? "," : "", path_for_batch(m.plan, m.sw, batches[i]));
    std::printf("]]\n");
}

int replay(int argc, char **argv)
{
    if (argc < 6) return 2;
    std::vector<int> batches;
    for (const char *s = argv[5]; *s;) {
        batches.push_back((int)std::strtol(s, const_cast<char **>(&s), 10));
        if (*s == ',') ++s;
    }
    Model m;
    if (int rc = create(m, argv)) {
        std::printf("[%d]\n", rc);
        return 0;
    }
    snapshot(m, 0, batches);
    for (int i = 6; i < argc; ++i) {
        const std::string call(argv[i]);
        int status = PDOG_E_ARG;
        if (call.rfind("v:", 0) == 0) {
            const int id = std::atoi(call.c_str() + 2);
            if (id < 0 || find_variant(id)) status = replan(m, m.sw, id); // (else: pdog_set_variant's "unknown variant id")
        } else if (call.rfind("t:", 0) == 0) {
            const size_t colon = call.find(':', 2);
            if (colon == std::string::npos) return 2;
            const std::string key = call.substr(2, colon - 2);
            const bool on = std::atoi(call.c_str() + colon + 1) != 0;
            Switches sw = m.sw;
            if (key == "no_tiled") sw.no_tiled = on;
            else if (key == "no_fused_c") sw.no_fused_c = on;
            else return 2; // (the other keys are no input of the plan)
            status = replan(m, sw, m.plan.forced ? m.plan.shape->id : -1);
        } else
            return 2;
        snapshot(m, status, batches);
    }
    return 0;
}

// ---- the checks ----
long failures = 0, checks = 0;
void expect(bool ok, const char *what, long a = -1, long b = -1, long c = -1)
{
    ++checks;
    if (ok) return;
    if (++failures <= 20) std::printf("MISMATCH %s (%ld, %ld, %ld)\n", what, a, b, c);
}

// chain_path's rule, a second time.  A pinned tracker runs its own kernel and nothing else: the chain kernel where it has one
// (a roll row with its full instance set, up to 8 strips, no progress to publish), the stepped walk otherwise.  Unpinned, the
// window decides: where the fused kernel fits it takes the chains unless the chain kernel is both available and better —
// better meaning at least 3000 pixels per window and 1400 strip-waves, and, where the two-pass kernels are set up, 1000
// strip-waves.  Windows too large for the fused kernel go to the chain kernel on the same terms, then to the tiled kernel if
// all clips' sub-windows are resident at once, then to the stepped walk.
ChainPath chain_path_restated(const Plan &p, int resident, int n_clips, int n_steps, bool table, bool progress)
{
    if (table && n_steps == 1) return ChainPath::Stepped;
    if (p.shape->family == Family::Fused) return ChainPath::Fused;
    const long strips = (p.geo.n2 + 63) / 64, waves = (long)n_clips * strips;
    const bool chain_kernel = !progress && p.shape->full_set && strips <= 8;
    if (p.forced) return chain_kernel ? ChainPath::Persistent : ChainPath::Stepped;
    const bool enough_waves = !p.small_twopass || waves >= 1000;
    if (p.fused.ok) {
        const bool fused_better = (long)p.geo.n1 * p.geo.n2 < 3000 || waves < 1400;
        return chain_kernel && !fused_better && enough_waves ? ChainPath::Persistent : ChainPath::Fused;
    }
    if (chain_kernel && enough_waves) return ChainPath::Persistent;
    const bool all_resident = n_steps <= 1 || (long)n_clips * p.tiled.ns1 * p.tiled.ns2 <= resident;
    return p.tiled.ok && n_clips >= 1 && all_resident ? ChainPath::Tiled : ChainPath::Stepped;
}

void check_plan(const Plan &p, const Switches &sw)
{
    for (int resident : {0, 81, 256})
        for (int n_clips : {1, 2, 125, 126, 349, 350, 1024, 4096})
            for (int n_steps : {1, 2, 64})
                for (int flags = 0; flags < 4; ++flags) {
                    const bool table = flags & 1, progress = flags & 2;
                    expect(chain_path(p, sw, resident, n_clips, n_steps, table, progress) == chain_path_restated(p, resident, n_clips, n_steps, table, progress),
                           "chain_path against the restated rule (clips, steps, resident)", n_clips, n_steps, resident);
                }
    // part_slots: every variant a later pdog_set_variant may pin, with its thin columns, and the tiled kernel's two sets
    for (const VariantShape &v : kVariantShapes)
        if (v.family != Family::Fused) expect(p.part_slots >= (p.geo.n2 + v.tw() - 1) / v.tw() + kThinMax, "part_slots holds the variant's slots", v.id);
    if (p.tiled.ok) {
        const int nsub = p.tiled.ns1 * p.tiled.ns2;
        expect(p.part_slots >= 2 * nsub, "part_slots holds the tiled kernel's two sets", nsub);
        for (int n : {1, 2, 3, 7}) {
            expect(tiled_serves(p, n * nsub, n, 2), "tiled_serves: n * ns1 * ns2 = resident", n, nsub);
            expect(!tiled_serves(p, n * nsub - 1, n, 2), "tiled_serves: one workgroup short", n, nsub);
            expect(tiled_serves(p, n * nsub, n, 64) && !tiled_serves(p, n * nsub, n + 1, 64), "tiled_serves: one clip too many", n, nsub);
            expect(tiled_serves(p, 0, n, 1), "tiled_serves: independent windows need no resident workgroup", n);
        }
        expect(!tiled_serves(p, 1 << 20, 0, 1) && !tiled_serves(p, 1 << 20, 0, 2), "tiled_serves: no window");
    } else
        expect(!tiled_serves(p, 1 << 20, 1, 1) && !tiled_serves(p, 1 << 20, 1, 2), "tiled_serves without a tiled plan");
}

int check(int argc, char **argv)
{
    if (argc < 5) return 2;
    double tw = 0;
    const Geometry g = geometry(argv, &tw);
    int plans = 0;
    for (int forced : {-1, -2, 0, kPathTwoPass, kPathFused}) { // -2: pinned to the variant the plan chose itself
        Plan p;
        std::string why;
        if (forced == -2) {
            if (make_plan(g, Switches(), -1, &p, &why)) continue;
            forced = p.shape->id;
        }
        for (bool no_tiled : {false, true}) {
            Switches sw;
            sw.no_tiled = no_tiled;
            if (make_plan(g, sw, forced, &p, &why)) continue;
            expect(p.forced == (forced >= 0) && p.shape && (forced < 0 || p.shape->id == forced), "the plan names the pinned variant", forced);
            check_plan(p, sw);
            ++plans;
        }
    }
    expect(plans >= 1, "no plan for this case");
    // plan_tiled's comment: a 257×257 window at l = 65 is cut into 81 sub-windows, a 129×129 window into 36
    for (int n : {257, 129}) {
        Plan p;
        std::string why;
        expect(make_plan(Geometry{1080, 1920, n, n, 65}, Switches(), -1, &p, &why) == PDOG_OK && p.tiled.ok && p.tiled.ns1 * p.tiled.ns2 == (n == 257 ? 81 : 36),
               "sub-windows of a square window at l = 65", n, p.tiled.ns1, p.tiled.ns2);
    }
    std::printf("%ld checks, %ld mismatches\n", checks, failures);
    return failures ? 1 : 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "replay")) return replay(argc - 2, argv + 2);
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return check(argc - 2, argv + 2);
    std::fprintf(stderr, "usage: plan_main replay|check FH FW TARGET_WIDTH WIN_H WIN_W [BATCHES CALL...]\n");
    return 2;
}
