// motion_main.cpp — pdog_assign_motion_host (csrc/pdog_math.cpp) as a stand-alone program for the host compiler and its
// sanitizers (tests/test_motion_cpu.py builds it plain and with AddressSanitizer + UBSan): seeded random groups of the kind
// the Python test draws — T and k in 1 ... 32, positions on a small grid so that blocking and ties are common, unsorted
// lists, -inf and NaN entries, counts below k, random velocities and hold counts, extreme positions — through the library's
// host function, each held to a second, naive statement of the rule (include/pawsome_motion.h) written without the rule
// header's helpers: per round every free entry of every unassigned target is listed, a target's head is the first of its
// entries in (D, q) order, and the heads are compared as floats, not as keys.  Prints "<n> groups, <m> mismatches"; exits
// non-zero on any.
#include "pdog_math.cpp"

#include <cstdio>
#include <limits>
#include <random>

namespace {

struct Entry { double D; int q; };

long long clampll(long long x, long long n) { return x < 1 ? 1 : x > n ? n : x; }

// D in doubles: exact for |difference| < 65536 (squares below 2^32, their sum below 2^33)
double naive_D(long long i, long long j, long long ci, long long cj)
{
    const long long di = i > ci ? i - ci : ci - i, dj = j > cj ? j - cj : cj - j;
    if (di > 65535 || dj > 65535) return 4294967295.0;
    return std::min(4294967295.0, (double)di * (double)di + (double)dj * (double)dj);
}

bool within(long long i, long long j, long long oi, long long oj, long long d)
{
    const __int128 di = (__int128)i - oi, dj = (__int128)j - oj;
    return di * di + dj * dj < (__int128)d * d;
}

// the value as the round ranks it
float rank_of(float v) { return v != v ? -std::numeric_limits<float>::infinity() : v; }

void naive_group(int T, int k, int d, float rho, float m, int coast, int h, int w, const int32_t *prev, const int32_t *ms_in,
                 const int32_t *ij, const float *peak, const int32_t *count, int32_t *out, int32_t *state, int32_t *next, int32_t *ms_out)
{
    std::vector<long long> ci(T), cj(T);
    std::vector<bool> done(T, false);
    for (int t = 0; t < T; ++t) {
        ci[t] = clampll((long long)prev[2 * t] + ms_in[4 * t], h);
        cj[t] = clampll((long long)prev[2 * t + 1] + ms_in[4 * t + 1], w);
        state[t] = -1;
    }
    for (;;) {
        int wt = -1, wq = 0;
        double wD = 0;
        for (int t = 0; t < T; ++t) {
            if (done[t]) continue;
            std::vector<Entry> free_entries;
            for (int q = 0; q < k; ++q) {
                const float v = peak[t * k + q], lim = rho * peak[t * k];
                if (q != 0 && q >= count[t]) continue;
                if (!(v > m) || !(v >= lim)) continue;
                bool blocked = false;
                for (int u = 0; u < T; ++u)
                    if (done[u] && within(ij[2 * (t * k + q)], ij[2 * (t * k + q) + 1], out[2 * u], out[2 * u + 1], d)) blocked = true;
                if (!blocked) free_entries.push_back({naive_D(ij[2 * (t * k + q)], ij[2 * (t * k + q) + 1], ci[t], cj[t]), q});
            }
            if (free_entries.empty()) continue;
            std::stable_sort(free_entries.begin(), free_entries.end(), [](const Entry &a, const Entry &b) { return a.D < b.D; });
            const Entry e = free_entries[0];
            const bool better = wt < 0 || e.D < wD || (e.D == wD && rank_of(peak[t * k + e.q]) > rank_of(peak[wt * k + wq]));
            if (better) { wt = t; wq = e.q; wD = e.D; }
        }
        if (wt < 0) break;
        done[wt] = true;
        out[2 * wt] = ij[2 * (wt * k + wq)];
        out[2 * wt + 1] = ij[2 * (wt * k + wq) + 1];
        state[wt] = wq + 1;
    }
    for (int t = 0; t < T; ++t) {
        long long vi = ms_in[4 * t], vj = ms_in[4 * t + 1], nh = ms_in[4 * t + 2];
        if (!done[t]) {
            out[2 * t] = (int32_t)ci[t];
            out[2 * t + 1] = (int32_t)cj[t];
            nh = std::min(nh + 1, 2147483647LL);
            if (nh >= coast) vi = vj = 0;
        } else {
            bool contested = false;
            for (int u = 0; u < T; ++u) contested = contested || (u != t && within(out[2 * t], out[2 * t + 1], ci[u], cj[u], d));
            if (!contested) {
                vi = (int32_t)(uint32_t)((long long)out[2 * t] - prev[2 * t]);         // modulo 2^32
                vj = (int32_t)(uint32_t)((long long)out[2 * t + 1] - prev[2 * t + 1]);
            }
            nh = 0;
        }
        ms_out[4 * t] = (int32_t)vi; ms_out[4 * t + 1] = (int32_t)vj; ms_out[4 * t + 2] = (int32_t)nh; ms_out[4 * t + 3] = 0;
        next[2 * t] = (int32_t)clampll(out[2 * t] + vi, h);
        next[2 * t + 1] = (int32_t)clampll(out[2 * t + 1] + vj, w);
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261019);
    auto below = [&](int n) { return (int)(rng() % (uint64_t)n); };
    long long groups = 0, bad = 0, held = 0, later = 0;
    for (int trial = 0; trial < 3000; ++trial) {
        const int G = 1 + below(3), T = trial < 64 ? 1 + trial % 32 : 1 + below(32), k = trial < 64 ? 32 - trial % 32 : 1 + below(32);
        const int d = 1 + below(6), grid = 2 + below(12), coast = below(5), h = 1 + below(2 * grid), w = 1 + below(2 * grid);
        const double rho = (trial % 5 == 0) ? (trial % 10 == 0 ? 0.0 : 1.0) : (rng() % 1001) / 1000.0;
        const double m = trial % 3 == 0 ? 0.0 : below(9) * 0.125;
        const bool wild = trial % 97 == 0; // positions and velocities at the ends of int32: nothing may overflow
        const size_t n = (size_t)G * T;
        std::vector<int32_t> prev(2 * n), ms(4 * n), ij(2 * n * k), count(n), out(2 * n, 12345), state(n, 12345), next(2 * n, 12345);
        std::vector<float> peak(n * k);
        auto extreme = [&] { return below(2) ? std::numeric_limits<int32_t>::max() - below(3) : std::numeric_limits<int32_t>::min() + below(3); };
        for (auto &v : prev) v = wild && below(2) ? extreme() : below(grid);
        for (auto &v : ij) v = wild ? (below(4) ? extreme() : below(grid) + below(2) * 65536) : below(grid);
        for (size_t p = 0; p < n; ++p) {
            ms[4 * p] = wild && below(2) ? extreme() : below(7) - 3;
            ms[4 * p + 1] = wild && below(2) ? extreme() : below(7) - 3;
            ms[4 * p + 2] = wild && below(4) == 0 ? std::numeric_limits<int32_t>::max() - below(2) : below(6);
            ms[4 * p + 3] = below(100);
        }
        for (auto &v : count) v = below(k + 2); // 0 and k + 1 included: the rule reads what it is given
        for (auto &v : peak) {
            const int kind = below(16);
            v = kind == 0 ? -std::numeric_limits<float>::infinity() : kind == 1 ? std::numeric_limits<float>::quiet_NaN()
                : kind == 2 ? -0.0f : kind == 3 ? 0.0f : (float)(below(9) - 2) * 0.25f;
        }
        const std::vector<int32_t> ms_in = ms;
        if (pdog_assign_motion_host(G, T, k, d, rho, m, coast, h, w, prev.data(), ms.data(), ij.data(), peak.data(), count.data(), out.data(),
                                    state.data(), next.data()) != PDOG_OK) {
            ++bad;
            continue;
        }
        for (int g = 0; g < G; ++g, ++groups) {
            const size_t w0 = (size_t)g * T;
            std::vector<int32_t> wo(2 * T), ws(T), wn(2 * T), wm(4 * T);
            naive_group(T, k, d, (float)rho, (float)m, coast, h, w, &prev[2 * w0], &ms_in[4 * w0], &ij[2 * w0 * k], &peak[w0 * k], &count[w0],
                        wo.data(), ws.data(), wn.data(), wm.data());
            for (int t = 0; t < T; ++t) {
                bad += ws[t] != state[w0 + t];
                held += ws[t] == -1;
                later += ws[t] > 1;
                for (int c = 0; c < 2; ++c) bad += (wo[2 * t + c] != out[2 * (w0 + t) + c]) + (wn[2 * t + c] != next[2 * (w0 + t) + c]);
                for (int c = 0; c < 4; ++c) bad += wm[4 * t + c] != ms[4 * (w0 + t) + c];
                for (int u = 0; u < t; ++u) // two assigned targets are never closer than d
                    bad += ws[t] >= 1 && ws[u] >= 1 && within(out[2 * (w0 + t)], out[2 * (w0 + t) + 1], out[2 * (w0 + u)], out[2 * (w0 + u) + 1], d);
            }
        }
    }
    bad += held < 1000 || later < 1000; // the draw exercises what it is for
    // what the function refuses, outputs and mstate untouched
    int32_t p[2] = {1, 1}, s4[4] = {7, 7, 7, 7}, o[2] = {7, 7}, nx[2] = {7, 7}, c = 1, s = 7;
    float v = 1.f;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto call = [&](int G, int T, int k, int d, double rho, double m, int coast, int h, int w, const int32_t *pp = nullptr) {
        return pdog_assign_motion_host(G, T, k, d, rho, m, coast, h, w, pp ? pp : p, s4, p, &v, &c, o, &s, nx);
    };
    bad += call(1, 0, 1, 1, 0.5, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 33, 1, 1, 0.5, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 0, 1, 0.5, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 33, 1, 0.5, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 0, 0.5, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, 1.5, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, nan, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, 0.5, -0.5, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, 0.5, nan, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, 0.5, inf, 1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, 0.5, 0, -1, 9, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, 0.5, 0, 1, 0, 9) != PDOG_E_ARG;
    bad += call(1, 1, 1, 1, 0.5, 0, 1, 9, 0) != PDOG_E_ARG;
    bad += call(0, 1, 1, 1, 0.5, 0, 1, 9, 9) != PDOG_E_ARG;
    bad += pdog_assign_motion_host(1, 1, 1, 1, 0.5, 0, 1, 9, 9, nullptr, s4, p, &v, &c, o, &s, nx) != PDOG_E_ARG;
    bad += o[0] != 7 || s != 7 || nx[0] != 7 || s4[0] != 7 || s4[3] != 7;
    s4[0] = s4[1] = s4[2] = 0;
    bad += call(1, 1, 1, 1, 0.5, 0, 1, 9, 9) != PDOG_OK || s != 1 || o[0] != 1 || nx[0] != 1 || s4[3] != 0;
    std::printf("%lld groups, %lld mismatches (%lld held, %lld later picks)\n", groups, bad, held, later);
    return bad ? 1 : 0;
}
