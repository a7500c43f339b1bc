// frame_blobs_main.cpp — the host-only pieces of the frame-blob kernels (csrc/pdog_frame_blobs.hpp) held to direct
// computations, by the host compiler alone (tests/test_frame_blobs_cpu.py builds this plain and with ASan + UBSan):
//   1. the row-word operations (run_start, run_starts, links_up / _left / _right, next_bound, run_sums) against their per-bit
//      definitions on random and on patterned words;
//   2. THE KERNELS' STEPS REPLAYED IN ORDER with the header's own functions and its own union-find loops on plain memory —
//      tiles of 64 x 64 labelled by runs and links, the border merge's three item sets, the flatten, the compaction through
//      block counts and block_offsets, the sums by stretches of 64 lanes — against a pixel flood fill and direct sums, on
//      patterns and noise, at frame sizes around the tile size and at both connectivities;
//   3. derive against long double arithmetic on drawn ellipses;
//   4. the admitted frame sizes (size_refusal) at their edges, where a product formed in 64 bits would wrap (UBSan watches).
// With the argument `sizes` it only prints size_refusal's verdict on the sizes it reads.  Otherwise prints "<n> checks, <m> mismatches"; exit status 1 on any mismatch.
#include "pdog_frame_blobs.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

using namespace pdog::fblobs;

static long n_checks = 0, n_bad = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        ++n_checks;                                      \
        if (!(cond)) {                                   \
            if (++n_bad <= 20) { std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                \
    } while (0)

static bool bit(uint64_t m, int c) { return c >= 0 && c < 64 && ((m >> c) & 1); }

static void check_words(uint64_t m, uint64_t up)
{
    uint64_t starts = 0, lu = 0, ll = 0, lr = 0;
    for (int c = 0; c < 64; ++c) {
        if (bit(m, c) && !bit(m, c - 1)) starts |= 1ull << c;
        if (bit(m, c) && bit(up, c) && !(bit(m, c - 1) && bit(up, c - 1))) lu |= 1ull << c;
        if (bit(m, c) && bit(up, c - 1) && !bit(up, c) && !bit(m, c - 1)) ll |= 1ull << c;
        if (bit(m, c) && bit(up, c + 1) && !bit(up, c) && !bit(m, c + 1)) lr |= 1ull << c;
        if (bit(m, c)) {
            int s = c;
            while (bit(m, s - 1)) --s;
            CHECK(run_start(m, c) == s, "run_start(%llx, %d) = %d, expected %d", (unsigned long long)m, c, run_start(m, c), s);
        }
        int e = c + 1;
        while (e < 64 && !bit(m, e)) ++e;
        CHECK(next_bound(m, c) == e, "next_bound(%llx, %d) = %d, expected %d", (unsigned long long)m, c, next_bound(m, c), e);
    }
    CHECK(run_starts(m) == starts, "run_starts(%llx)", (unsigned long long)m);
    CHECK(links_up(m, up) == lu, "links_up(%llx, %llx)", (unsigned long long)m, (unsigned long long)up);
    CHECK(links_left(m, up) == ll, "links_left(%llx, %llx)", (unsigned long long)m, (unsigned long long)up);
    CHECK(links_right(m, up) == lr, "links_right(%llx, %llx)", (unsigned long long)m, (unsigned long long)up);
}

struct Frame {
    int h, w;
    std::vector<uint8_t> mask; // 0 / 1
    std::vector<int> s;        // contrasts
    bool at(int r, int c) const { return r >= 0 && r < h && c >= 0 && c < w && mask[(size_t)r * w + c]; }
};

// the label of every pixel by a plain flood fill in raster order: the index of the blob's first pixel, -1 outside the mask
static std::vector<int> flood(const Frame &f, bool conn8)
{
    std::vector<int> lab((size_t)f.h * f.w, -1), stack;
    for (int p = 0; p < f.h * f.w; ++p) {
        if (!f.mask[p] || lab[p] >= 0) continue;
        lab[p] = p;
        stack.push_back(p);
        while (!stack.empty()) {
            const int q = stack.back(), r = q / f.w, c = q % f.w;
            stack.pop_back();
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) {
                    if ((!dr && !dc) || (!conn8 && dr && dc)) continue;
                    if (f.at(r + dr, c + dc) && lab[(r + dr) * f.w + c + dc] < 0) {
                        lab[(r + dr) * f.w + c + dc] = p;
                        stack.push_back((r + dr) * f.w + c + dc);
                    }
                }
        }
    }
    return lab;
}

// the kernels' steps (a) - (c), in order, on plain memory
static std::vector<int> replay_labels(const Frame &f, bool conn8)
{
    const int h = f.h, w = f.w;
    std::vector<int> L((size_t)h * w, -1);
    const auto plain = [](std::vector<int> &par) {
        return std::make_pair([&par](int i) { return par[i]; }, [&par](int i, int v) { const int old = par[i]; par[i] = std::min(old, v); return old; });
    };
    // (a) every tile by runs and links
    for (int ty = 0; ty * kTile < h; ++ty)
        for (int tx = 0; tx * kTile < w; ++tx) {
            uint64_t m[kTile] = {};
            for (int r = 0; r < kTile; ++r)
                for (int c = 0; c < kTile; ++c)
                    if (f.at(ty * kTile + r, tx * kTile + c)) m[r] |= 1ull << c;
            std::vector<int> par(kTile * kTile);
            for (int i = 0; i < kTile * kTile; ++i) par[i] = i;
            auto [load, lower] = plain(par);
            for (int r = kTile - 1; r >= 1; --r) { // (the kernel's lanes run in no particular order: bottom-up here)
                const uint64_t up = m[r - 1];
                for (uint64_t l = links_up(m[r], up); l; l &= l - 1) {
                    const int c = __builtin_ctzll(l);
                    uf_union(load, lower, r * kTile + run_start(m[r], c), (r - 1) * kTile + run_start(up, c));
                }
                if (!conn8) continue;
                for (uint64_t l = links_left(m[r], up); l; l &= l - 1) {
                    const int c = __builtin_ctzll(l);
                    uf_union(load, lower, r * kTile + run_start(m[r], c), (r - 1) * kTile + run_start(up, c - 1));
                }
                for (uint64_t l = links_right(m[r], up); l; l &= l - 1) {
                    const int c = __builtin_ctzll(l);
                    uf_union(load, lower, r * kTile + run_start(m[r], c), (r - 1) * kTile + run_start(up, c + 1));
                }
            }
            for (int r = 0; r < kTile; ++r)
                for (int c = 0; c < kTile; ++c)
                    if ((m[r] >> c) & 1) {
                        const int root = uf_find(load, lower, r * kTile + run_start(m[r], c));
                        L[(size_t)(ty * kTile + r) * w + tx * kTile + c] = (ty * kTile + (root >> 6)) * w + tx * kTile + (root & 63);
                    }
        }
    // (b) the border merge's items, as fb_merge_kernel numbers them (here from the last to the first)
    auto [load, lower] = plain(L);
    const auto at = [&](int r, int c) { return r >= 0 && r < h && c >= 0 && c < w ? L[(size_t)r * w + c] : -1; };
    const int n_hb = (h - 1) / kTile, n_vb = (w - 1) / kTile;
    for (int item = n_hb * w + 2 * n_vb * h - 1; item >= 0; --item) {
        int idx = item;
        if (idx < n_hb * w) {
            const int r = (idx / w + 1) * kTile, c = idx % w;
            if (at(r, c) < 0) continue;
            if (at(r - 1, c) >= 0) {
                uf_union(load, lower, r * w + c, (r - 1) * w + c);
            } else if (conn8) {
                if (at(r - 1, c - 1) >= 0) uf_union(load, lower, r * w + c, (r - 1) * w + c - 1);
                if (at(r - 1, c + 1) >= 0) uf_union(load, lower, r * w + c, (r - 1) * w + c + 1);
            }
            continue;
        }
        idx -= n_hb * w;
        if (idx < n_vb * h) {
            const int c = (idx / h + 1) * kTile, r = idx % h;
            if (at(r, c) < 0) continue;
            if (at(r, c - 1) >= 0) uf_union(load, lower, r * w + c, r * w + c - 1);
            else if (conn8 && at(r - 1, c - 1) >= 0) uf_union(load, lower, r * w + c, (r - 1) * w + c - 1);
            continue;
        }
        idx -= n_vb * h;
        if (conn8) {
            const int c = (idx / h + 1) * kTile - 1, r = idx % h;
            if (at(r, c) >= 0 && at(r - 1, c) < 0 && at(r - 1, c + 1) >= 0) uf_union(load, lower, r * w + c, (r - 1) * w + c + 1);
        }
    }
    // (c) the flatten
    for (int p = 0; p < h * w; ++p)
        if (L[p] >= 0) L[p] = uf_find(load, lower, L[p]);
    return L;
}

// steps (d) and (e) on flat labels against direct sums over the flood fill's blobs
static void check_words_of(const Frame &f, const std::vector<int> &lab, int64_t min_area, int64_t max_area, int cap)
{
    const int h = f.h, w = f.w, n_pix = h * w, block = 256, n_blocks = (n_pix + block - 1) / block;
    // direct: the blobs in ascending first
    std::vector<std::vector<int64_t>> direct;
    std::vector<int> rank_of(n_pix, -1);
    std::vector<int64_t> area(n_pix, 0);
    for (int p = 0; p < n_pix; ++p)
        if (lab[p] >= 0) ++area[lab[p]];
    int64_t kept_total = 0;
    for (int p = 0; p < n_pix; ++p)
        if (lab[p] == p && area[p] >= min_area && area[p] <= max_area) {
            if (kept_total < cap) {
                rank_of[p] = (int)kept_total;
                direct.push_back({0, 0, 0, 0, 0, 0, h, -1, w, -1, p, 0});
            }
            ++kept_total;
        }
    for (int p = 0; p < n_pix; ++p) {
        if (lab[p] < 0 || rank_of[lab[p]] < 0) continue;
        auto &o = direct[rank_of[lab[p]]];
        const int64_t r = p / w, c = p % w;
        o[W_N] += 1; o[W_SY] += r; o[W_SX] += c; o[W_SYY] += r * r; o[W_SYX] += r * c; o[W_SXX] += c * c; o[W_SS] += f.s[p];
        o[W_RMIN] = std::min(o[W_RMIN], r); o[W_RMAX] = std::max(o[W_RMAX], r);
        o[W_CMIN] = std::min(o[W_CMIN], c); o[W_CMAX] = std::max(o[W_CMAX], c);
    }
    // (d) block counts, their offsets, the ranks
    std::vector<int32_t> counts(n_blocks, 0), offsets(n_blocks, 0);
    const auto kept = [&](int p) { return lab[p] == p && area[p] >= min_area && area[p] <= max_area; };
    for (int p = 0; p < n_pix; ++p) counts[p / block] += kept(p);
    CHECK(block_offsets(counts.data(), n_blocks, offsets.data()) == kept_total, "block_offsets total");
    std::vector<int> rank(n_pix, -1);
    std::vector<std::vector<int64_t>> got(std::min<int64_t>(kept_total, cap), std::vector<int64_t>(kWords, 0));
    for (int b = 0; b < n_blocks; ++b) {
        int below = 0;
        for (int p = b * block; p < std::min(n_pix, (b + 1) * block); ++p)
            if (kept(p)) {
                const int k = offsets[b] + below++;
                if (k < cap) {
                    rank[p] = k;
                    got[k][W_RMIN] = h; got[k][W_RMAX] = -1; got[k][W_CMIN] = w; got[k][W_CMAX] = -1; got[k][W_FIRST] = p;
                }
            }
    }
    for (int p = 0; p < n_pix; ++p) CHECK(rank[p] == rank_of[p], "rank of %d: %d, expected %d", p, rank[p], rank_of[p]);
    // (e) a "wave" per 64 pixels of a row
    const int wpr = (w + 63) / 64;
    for (int item = 0; item < h * wpr; ++item) {
        const int row = item / wpr, c0 = (item % wpr) * 64;
        int rk[64], s[64], incl[64];
        uint64_t bounds = 0;
        for (int lane = 0; lane < 64; ++lane) {
            const int col = c0 + lane;
            rk[lane] = -1;
            s[lane] = 0;
            if (col < w && lab[row * w + col] >= 0) rk[lane] = rank[lab[row * w + col]];
            if (rk[lane] >= 0) s[lane] = f.s[row * w + col];
            incl[lane] = s[lane] + (lane ? incl[lane - 1] : 0);
            if (lane == 0 || rk[lane] != rk[lane - 1]) bounds |= 1ull << lane;
        }
        for (int lane = 0; lane < 64; ++lane) {
            if (rk[lane] < 0 || !((bounds >> lane) & 1)) continue;
            const int end = next_bound(bounds, lane);
            int64_t n, sx, sxx;
            const int64_t a = c0 + lane, b = a + (end - lane) - 1, y = row;
            run_sums(a, b, &n, &sx, &sxx);
            auto &o = got[rk[lane]];
            o[W_N] += n; o[W_SY] += n * y; o[W_SX] += sx; o[W_SYY] += n * y * y; o[W_SYX] += y * sx; o[W_SXX] += sxx;
            o[W_SS] += incl[end - 1] - (incl[lane] - s[lane]);
            o[W_RMIN] = std::min(o[W_RMIN], y); o[W_RMAX] = std::max(o[W_RMAX], y);
            o[W_CMIN] = std::min(o[W_CMIN], a); o[W_CMAX] = std::max(o[W_CMAX], b);
        }
    }
    CHECK(got.size() == direct.size(), "rows");
    for (size_t k = 0; k < std::min(got.size(), direct.size()); ++k)
        for (int i = 0; i < kWords; ++i) CHECK(got[k][i] == direct[k][i], "blob %zu word %d: %lld, expected %lld", k, i, (long long)got[k][i], (long long)direct[k][i]);
}

static Frame make_frame(int h, int w, int kind, std::mt19937_64 &rng)
{
    Frame f{h, w, std::vector<uint8_t>((size_t)h * w, 0), std::vector<int>((size_t)h * w, 0)};
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            bool on = false;
            switch (kind) {
            case 0: on = rng() % 100 < 41; break;                                   // noise below the thresholds
            case 1: on = rng() % 100 < 59; break;                                   // and above
            case 2: on = (r + c) % 2 == 0; break;                                   // checkerboard
            case 3: on = c % 2 == 0 || r == h - 1; break;                           // comb
            case 4: on = r == c || r + c == 2 * kTile - 1 || r + 1 == c || r + c == 2 * kTile; break; // staircases through the tile corners
            case 5: on = r % kTile == 32 || c % kTile == 32 || r == 0; break;       // lattice
            case 6: on = c == kTile - 2 || c == kTile || r == kTile - 1 || r == kTile + 1; break;     // neighbours across borders
            case 7: on = true; break;
            case 8: on = (r % kTile >= 62 || r % kTile <= 1) && (c % kTile >= 62 || c % kTile <= 1) && rng() % 100 < 50; break; // noise at the corners
            default: on = (r % 4 == 0 && (c + 1) % kTile != (r / 4) % kTile) || (r % 4 == 2 && c % 8 == 0) || (r % 2 == 1 && (c == 0 || c == w - 1) && (r / 2) % 2 == (c == 0)); break; // a serpentine
            }
            f.mask[(size_t)r * w + c] = on;
            f.s[(size_t)r * w + c] = on ? 8 + (int)(rng() % 61) : 0;
        }
    return f;
}

// `frame_blobs sizes`: reads "h w" pairs from standard input and prints, for each, "h w admitted" or "h w refused: <what does
// not fit>" — size_refusal's verdict, which the pytest compares with the rule in Python integers.
static int sizes_mode()
{
    long long h, w;
    while (std::scanf("%lld %lld", &h, &w) == 2) {
        const char *why = size_refusal(h, w);
        if (why) std::printf("%lld %lld refused: %s\n", h, w, why);
        else std::printf("%lld %lld admitted\n", h, w);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "sizes") return sizes_mode();
    std::mt19937_64 rng(20261021);
    // 1. row words
    const uint64_t patterns[] = {0, ~0ull, 1, 1ull << 63, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull, 0x8000000000000001ull, 0x00ff00ff00ff00ffull, 0x7ffffffffffffffeull};
    for (uint64_t a : patterns)
        for (uint64_t b : patterns) check_words(a, b);
    for (int i = 0; i < 4000; ++i) {
        uint64_t a = rng(), b = rng();
        if (i % 3 == 1) a &= rng(), b &= rng();
        if (i % 3 == 2) a |= rng(), b |= rng();
        check_words(a, b);
    }
    for (int a = 0; a < 70; ++a)
        for (int b = a; b < 200; b += 7) {
            int64_t n, sx, sxx, dn = 0, dsx = 0, dsxx = 0;
            for (int c = a; c <= b; ++c) { dn += 1; dsx += c; dsxx += (int64_t)c * c; }
            run_sums(a, b, &n, &sx, &sxx);
            CHECK(n == dn && sx == dsx && sxx == dsxx, "run_sums(%d, %d)", a, b);
        }
    {   // a wave's 64 lanes at the end of the widest row an entry point accepts: no overflow on the way (UBSan watches)
        int64_t n, sx, sxx, dsx = 0, dsxx = 0;
        const int64_t b = (1ll << 21) - 1, a = b - 63;
        for (int64_t c = a; c <= b; ++c) { dsx += c; dsxx += c * c; }
        run_sums(a, b, &n, &sx, &sxx);
        CHECK(n == 64 && sx == dsx && sxx == dsxx, "run_sums at 2^21");
    }
    // 2. the kernels' steps against the flood fill
    const int hs[] = {1, 2, 31, 33, 64, 65, 70, 130}, ws[] = {1, 63, 64, 65, 127, 129, 200};
    long frames = 0;
    for (int h : hs)
        for (int w : ws)
            for (int kind = 0; kind < 10; ++kind) {
                const Frame f = make_frame(h, w, kind, rng);
                for (int conn8 = 0; conn8 < 2; ++conn8) {
                    const std::vector<int> want = flood(f, conn8), got = replay_labels(f, conn8);
                    long bad = 0;
                    for (int p = 0; p < h * w; ++p) bad += want[p] != got[p];
                    CHECK(bad == 0, "labels of kind %d at %d x %d, connectivity %d: %ld pixels differ", kind, h, w, conn8 ? 8 : 4, bad);
                    check_words_of(f, want, 1, (int64_t)h * w, 64);
                    if (kind < 2) check_words_of(f, want, 3, 40, 5);
                    ++frames;
                }
            }
    // 3. derive on drawn ellipses
    for (int i = 0; i < 200; ++i) {
        const double cy = 40 + (double)(rng() % 1000) / 50, cx = 60 + (double)(rng() % 1000) / 50, a = 4 + (double)(rng() % 300) / 10, b = 2 + (double)(rng() % 100) / 10, th = (double)(rng() % 314) / 100;
        int64_t s[kWords] = {};
        long double n = 0, sy = 0, sx = 0, syy = 0, syx = 0, sxx = 0;
        for (int r = 0; r < 120; ++r)
            for (int c = 0; c < 160; ++c) {
                const double u = (c - cx) * std::cos(th) + (r - cy) * std::sin(th), v = -(c - cx) * std::sin(th) + (r - cy) * std::cos(th);
                if (u * u / (a * a) + v * v / (b * b) > 1) continue;
                s[W_N] += 1; s[W_SY] += r; s[W_SX] += c; s[W_SYY] += r * r; s[W_SYX] += r * c; s[W_SXX] += c * c;
                n += 1; sy += r; sx += c; syy += (long double)r * r; syx += (long double)r * c; sxx += (long double)c * c;
            }
        double out[6];
        derive(s, out);
        if (n == 0) { CHECK(out[0] != out[0], "empty ellipse"); continue; }
        const long double my = sy / n, mx = sx / n, myy = syy / n - my * my + 1.0L / 12, mxx = sxx / n - mx * mx + 1.0L / 12, myx = syx / n - my * mx;
        const long double t = std::hypot(2 * myx, mxx - myy), lo = std::max(0.0L, (mxx + myy - t) / 2);
        const long double want[6] = {1 + my, 1 + mx, 0.5L * std::atan2(2 * myx, mxx - myy), 4 * std::sqrt((mxx + myy + t) / 2), 4 * std::sqrt(lo), 2 * std::sqrt(n / 3.14159265358979323846L)};
        for (int k = 0; k < 6; ++k) {
            if (k == 2 && t < 1e-6L) continue; // a circle has no direction
            CHECK(std::fabs((double)(out[k] - want[k])) <= 1e-9 * std::max(1.0, std::fabs((double)want[k])), "derive value %d: %.17g, expected %.17Lg", k, out[k], want[k]);
        }
    }
    // 4. the admitted sizes: the last admitted and the first refused of three widths, and sides whose 64-bit products would wrap
    CHECK(!size_refusal(3024617, 1) && size_refusal(3024618, 1), "sizes at width 1");
    CHECK(!size_refusal(243353, 1920) && size_refusal(243354, 1920), "sizes at width 1920");
    CHECK(!size_refusal(3, 1 << 21) && size_refusal(4, 1 << 21) && size_refusal(1, (1 << 21) + 1), "sizes at width 2^21");
    CHECK(!size_refusal(32768, 32768) && size_refusal(32769, 32768) && !size_refusal(1, 1), "sizes at the pixel limit");
    CHECK(size_refusal(INT64_MAX, INT64_MAX) && size_refusal(INT64_MAX, 2) && size_refusal(INT64_MIN, 1) && size_refusal(0, 5) && size_refusal(5, -1), "sizes outside every range");
    std::printf("%ld frames replayed\n%ld checks, %ld mismatches\n", frames, n_checks, n_bad);
    return n_bad ? 1 : 0;
}
