// exclusive_main.cpp — pdog_assign_exclusive_host (csrc/pdog_math.cpp) as a stand-alone program for the host compiler and its
// sanitizers (tests/test_exclusive_cpu.py builds it plain and with AddressSanitizer + UBSan): seeded random groups of the kind
// the Python test draws — T and k in 1 ... 32, positions on a small grid so that blocking and ties are common, unsorted
// lists, -inf and NaN entries, counts below k, extreme positions — through the library's host function, each checked against
// the rule's consequences (include/pawsome_exclusive.h): every state is -1 or a pick 1 ... k that is admissible, an assigned
// position is that pick's, a held one prev, no two assigned targets lie closer than d, no held target had an admissible
// entry free of every assigned position, T = 1 takes pick 1.  Prints "<n> groups, <m> mismatches"; exits non-zero on any.
#include "pdog_math.cpp"

#include <cstdio>
#include <limits>
#include <random>

int main()
{
    using namespace pdog::exclusive;
    std::mt19937_64 rng(20251019);
    auto below = [&](int n) { return (int)(rng() % (uint64_t)n); };
    long long groups = 0, bad = 0;
    for (int trial = 0; trial < 3000; ++trial) {
        const int G = 1 + below(3), T = trial < 64 ? 1 + trial % 32 : 1 + below(32), k = trial < 64 ? 32 - trial % 32 : 1 + below(32);
        const int d = 1 + below(6), grid = 2 + below(12);
        const double rho = (trial % 5 == 0) ? (trial % 10 == 0 ? 0.0 : 1.0) : (rng() % 1001) / 1000.0;
        const bool wild = trial % 97 == 0; // positions at the ends of int32: the distance test must not overflow
        const size_t n = (size_t)G * T;
        std::vector<int32_t> prev(2 * n), ij(2 * n * k), count(n), out(2 * n, 12345), state(n, 12345);
        std::vector<float> peak(n * k);
        for (auto &v : prev) v = below(grid);
        for (auto &v : ij) v = wild ? (below(2) ? std::numeric_limits<int32_t>::max() - below(3) : std::numeric_limits<int32_t>::min() + below(3)) : below(grid);
        for (auto &v : count) v = below(k + 2); // 0 and k + 1 included: the rule reads what it is given
        for (auto &v : peak) {
            const int kind = below(16);
            v = kind == 0 ? -std::numeric_limits<float>::infinity() : kind == 1 ? std::numeric_limits<float>::quiet_NaN()
                : kind == 2 ? -0.0f : kind == 3 ? 0.0f : (float)(below(9) - 2) * 0.25f;
        }
        if (pdog_assign_exclusive_host(G, T, k, d, rho, prev.data(), ij.data(), peak.data(), count.data(), out.data(), state.data()) != PDOG_OK) {
            ++bad;
            continue;
        }
        const float rho_f = (float)rho;
        for (int g = 0; g < G; ++g, ++groups) {
            const size_t w0 = (size_t)g * T;
            for (int t = 0; t < T; ++t) {
                const size_t w = w0 + t;
                const int s = state[w];
                if (s == -1) {
                    bad += out[2 * w] != prev[2 * w] || out[2 * w + 1] != prev[2 * w + 1];
                    for (int q = 0; q < k; ++q) { // a held target had no head when the step ended
                        if (!admissible(q, count[w], peak[w * k + q], peak[w * k], rho_f)) continue;
                        bool blocked = false;
                        for (int u = 0; u < T; ++u)
                            blocked |= state[w0 + u] >= 1 && blocks(ij[2 * (w * k + q)], ij[2 * (w * k + q) + 1], out[2 * (w0 + u)], out[2 * (w0 + u) + 1], d);
                        bad += !blocked;
                    }
                    continue;
                }
                if (s < 1 || s > k) { ++bad; continue; }
                const int q = s - 1;
                bad += !admissible(q, count[w], peak[w * k + q], peak[w * k], rho_f);
                bad += out[2 * w] != ij[2 * (w * k + q)] || out[2 * w + 1] != ij[2 * (w * k + q) + 1];
                for (int u = 0; u < t; ++u)
                    bad += state[w0 + u] >= 1 && blocks(out[2 * w], out[2 * w + 1], out[2 * (w0 + u)], out[2 * (w0 + u) + 1], d);
            }
            if (T == 1) bad += state[w0] != 1;
        }
    }
    // what the function refuses, outputs untouched
    int32_t p[2] = {1, 1}, o[2] = {7, 7}, c = 1, s = 7;
    float v = 1.f;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bad += pdog_assign_exclusive_host(1, 0, 1, 1, 0.5, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 33, 1, 1, 0.5, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 1, 0, 1, 0.5, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 1, 33, 1, 0.5, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 1, 1, 0, 0.5, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 1, 1, 1, 1.5, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 1, 1, 1, -0.1, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 1, 1, 1, nan, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(0, 1, 1, 1, 0.5, p, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += pdog_assign_exclusive_host(1, 1, 1, 1, 0.5, nullptr, p, &v, &c, o, &s) != PDOG_E_ARG;
    bad += o[0] != 7 || s != 7;
    bad += pdog_assign_exclusive_host(1, 1, 1, 1, 0.5, p, p, &v, &c, o, &s) != PDOG_OK || s != 1 || o[0] != 1;
    std::printf("%lld groups, %lld mismatches\n", groups, bad);
    return bad ? 1 : 0;
}
