// The weights of the pre-pass's second stage (csrc/pdog_math.cpp, dog_refine_weights; csrc/dog_prune.hpp, "the cell bound") and the
// cells' roots (csrc/dog_prune_words.hpp, pw_root16) under the host compiler.  For l = 17, 65 and 149:
//   * every box sum RefineBoxes::norm2(dy, i, dx, j) against the direct Σ K² over the box's rows and columns of the dense
//     kernel K = g₊⊗g₊ − g₋⊗g₋, in long double, within 1e-12·‖K‖₂²;
//   * for every offset (i, j) the NS² boxes tile the kernel: their sums add up to ‖K‖₂² within 1e-12 relative;
//   * every weight, in its unit ‖K‖₂ / 2¹², is at least the brute-force maximum over the 64 offsets and both tap roundings, and
//     at most one unit and a thousandth above it;
//   * the table is symmetric and NS × NS.
// pw_root16(e) is the smallest r with r² ≥ 256·e for every e up to 2¹⁶, around every square and at the top of its range.
// Build: g++ -std=c++17 -I csrc tests/refine_weights_main.cpp csrc/pdog_math.cpp
#include "pdog_host.hpp"
#include "dog_prune_words.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

using namespace pdog;

static long checks = 0, bad = 0;
#define CHECK(c, ...) do { ++checks; if (!(c)) { if (++bad <= 20) { std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void one_length(int l)
{
    double tw = 0;
    for (double t = 1.0; t < 200.0; t += 0.5)
        if (kernel_len_of_sigma(sigma_of(t)) == l) { tw = t; break; }
    CHECK(tw > 0, "no target width gives l = %d", l);
    if (tw <= 0) return;
    const double sg = sigma_of(tw);
    std::vector<double> gp(l), gm(l);
    gaussian_1d(sg, l, gp.data());
    gaussian_1d(sg * std::sqrt(2.0), l, gm.data());
    const double norm = dog_kernel_norm_up(gp, gm);
    const std::vector<uint32_t> wq = dog_refine_weights(gp, gm, norm);
    const int ns = refine_span(l);
    CHECK((int)wq.size() == ns * ns, "l = %d: %zu weights, NS = %d", l, wq.size(), ns);
    std::vector<long double> wmax((size_t)ns * ns, 0.0L);
    for (int f32 = 0; f32 < 2; ++f32) {
        const RefineBoxes box(gp, gm, f32 != 0);
        CHECK(box.ns == ns, "span");
        std::vector<long double> K2((size_t)l * l);
        long double total = 0;
        for (int a = 0; a < l; ++a)
            for (int b = 0; b < l; ++b) {
                const long double pa = f32 ? (long double)(float)gp[a] : (long double)gp[a], pb = f32 ? (long double)(float)gp[b] : (long double)gp[b];
                const long double ma = f32 ? (long double)(float)gm[a] : (long double)gm[a], mb = f32 ? (long double)(float)gm[b] : (long double)gm[b];
                const long double k = pa * pb - ma * mb;
                K2[(size_t)a * l + b] = k * k;
                total += k * k;
            }
        CHECK(std::sqrt((double)total) <= norm && std::sqrt((double)total) >= norm * (1 - 1e-6), "l = %d: the norm %.17g against %.17g", l, norm, std::sqrt((double)total));
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j) {
                long double sum = 0;
                for (int dy = 0; dy < ns; ++dy)
                    for (int dx = 0; dx < ns; ++dx) {
                        long double direct = 0;
                        for (int a = std::max(8 * dy - i, 0); a < std::min(8 * dy - i + 8, l); ++a)
                            for (int b = std::max(8 * dx - j, 0); b < std::min(8 * dx - j + 8, l); ++b) direct += K2[(size_t)a * l + b];
                        const double got = box.norm2(dy, i, dx, j);
                        CHECK(std::fabs((double)((long double)got - direct)) <= 1e-12 * (double)total, "l = %d f32 = %d box (%d, %d) offset (%d, %d): %.17g against %.17g", l, f32, dy, dx, i, j, got, (double)direct);
                        sum += (long double)got;
                        wmax[(size_t)dy * ns + dx] = std::max(wmax[(size_t)dy * ns + dx], direct);
                    }
                CHECK(std::fabs((double)(sum - total)) <= 1e-12 * (double)total, "l = %d f32 = %d offset (%d, %d): the boxes sum to %.17g, the kernel to %.17g", l, f32, i, j, (double)sum, (double)total);
            }
    }
    for (int dy = 0; dy < ns; ++dy)
        for (int dx = 0; dx < ns; ++dx) {
            const long double exact = 4096.0L * std::sqrt(wmax[(size_t)dy * ns + dx]) / (long double)norm; // in the weights' unit
            const uint32_t w = wq[(size_t)dy * ns + dx];
            CHECK((long double)w >= exact, "l = %d weight (%d, %d): %u below the exact %.6Lf", l, dy, dx, w, exact);
            CHECK((long double)w <= exact + 1.001L, "l = %d weight (%d, %d): %u far above the exact %.6Lf", l, dy, dx, w, exact);
            CHECK(w == wq[(size_t)dx * ns + dy] && w <= 4097u, "l = %d weight (%d, %d): symmetry and range", l, dy, dx);
        }
    std::printf("l = %d (target width %.1f): NS = %d, corner weight %u, centre weight %u\n", l, tw, ns, wq[0], wq[(size_t)(ns / 2) * ns + ns / 2]);
}

static void roots()
{
    auto want = [](uint32_t e) {
        uint64_t r = (uint64_t)std::floor(16.0 * std::sqrt((double)e));
        while (r > 0 && (r - 1) * (r - 1) >= 256ull * e) --r;
        while (r * r < 256ull * e) ++r;
        return (uint32_t)r;
    };
    const uint32_t top = 64u * 255u * 255u;
    for (uint32_t e = 0; e <= 65536u; ++e) CHECK(pw_root16(e) == want(e), "root of %u: %u against %u", e, pw_root16(e), want(e));
    for (uint32_t s = 1; s <= 2040u; ++s)
        for (int d = -2; d <= 2; ++d) {
            const uint32_t e = std::min(top, s * s + (uint32_t)d);
            CHECK(pw_root16(e) == want(e), "root of %u: %u against %u", e, pw_root16(e), want(e));
        }
    for (uint32_t e = top - 4096u; e <= top; ++e) CHECK(pw_root16(e) == want(e), "root of %u: %u against %u", e, pw_root16(e), want(e));
    CHECK(pw_root16(top) == 32640u, "the largest root");
}

int main()
{
    for (int l : {17, 65, 149}) one_length(l);
    roots();
    std::printf("%ld checks, %ld mismatches\n", checks, bad);
    return bad ? 1 : 0;
}
