// The blob rule's row-word operations (csrc/pdog_blob_fill.hpp) held against pixel arithmetic on the host: run_fill for one and
// for four words against a bit-by-bit run extension, the neighbour candidates for both connectivities against a per-pixel
// test, and the whole region grow — sweeps of sweep_row1 / sweep_row4 over every row from the same old state, until one adds
// no bit — against a pixel flood fill with an explicit stack, on square masks of D = 5, 17, 63, 64, 65, 127, 129 and 255 columns:
// random masks at several densities, vertical and horizontal combs, all-ones rows, single bits at the word edges.  It also holds
// the sweeps to their bound (component pixels + 1) and prints the sweep counts of the masks DESIGN.md quotes.
// Prints "<n> checks, <m> mismatches"; exits non-zero on any.
#include "pdog_blob_fill.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pdog::blobfill;

static long long bad = 0, checks = 0;
static uint64_t rng_state = 0x2026102012345677ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static void expect(bool ok, const char *what, long long a, long long b, long long c)
{
    ++checks;
    if (!ok && bad++ < 20) std::printf("MISMATCH %s (%lld, %lld, %lld)\n", what, a, b, c);
}

static const Row4 kZero = {{0, 0, 0, 0}};
static bool get(const Row4 &r, int x) { return (r.w[x >> 6] >> (x & 63)) & 1u; }
static void set(Row4 &r, int x) { r.w[x >> 6] |= 1ull << (x & 63); }
static bool same(const Row4 &a, const Row4 &b) { return !differ4(a, b); }

static Row4 random_row(int D, unsigned per_mille)
{
    Row4 r = kZero;
    for (int x = 0; x < D; ++x)
        if (rnd() % 1000u < per_mille) set(r, x);
    return r;
}

// bit by bit: every bit of s extended to its run of m
static Row4 naive_run_fill(const Row4 &m, const Row4 &s, int D)
{
    Row4 o = kZero;
    for (int x = 0; x < D; ++x) {
        if (!get(s, x)) continue;
        for (int u = x; u >= 0 && get(m, u); --u) set(o, u);
        for (int u = x; u < D && get(m, u); ++u) set(o, u);
    }
    return o;
}

static Row4 naive_candidates(const Row4 &m, const Row4 &f, const Row4 &up, const Row4 &dn, bool eight, int D)
{
    Row4 o = kZero;
    for (int x = 0; x < D; ++x) {
        if (!get(m, x)) continue;
        bool hit = get(f, x) || get(up, x) || get(dn, x);
        if (eight) {
            if (x > 0) hit = hit || get(up, x - 1) || get(dn, x - 1);
            if (x + 1 < D) hit = hit || get(up, x + 1) || get(dn, x + 1);
        }
        if (hit) set(o, x);
    }
    return o;
}

static void check_row_ops(const Row4 &m, const Row4 &s_any, const Row4 &up, const Row4 &dn, int D, const char *what)
{
    Row4 s;
    for (int k = 0; k < 4; ++k) s.w[k] = s_any.w[k] & m.w[k];
    const Row4 want = naive_run_fill(m, s, D);
    expect(same(run_fill4(m, s), want), what, D, 4, 0);
    if (D <= 64) expect(run_fill1(m.w[0], s.w[0]) == want.w[0], what, D, 1, 0);
    for (int eight = 0; eight < 2; ++eight) {
        const Row4 c = naive_candidates(m, s, up, dn, eight != 0, D);
        expect(same(candidates4(m, s, up, dn, eight != 0), c), what, D, 4, 1 + eight);
        expect(same(sweep_row4(m, s, up, dn, eight != 0), naive_run_fill(m, c, D)), what, D, 4, 3 + eight);
        if (D <= 64) {
            expect(candidates1(m.w[0], s.w[0], up.w[0], dn.w[0], eight != 0) == c.w[0], what, D, 1, 1 + eight);
            expect(sweep_row1(m.w[0], s.w[0], up.w[0], dn.w[0], eight != 0) == naive_run_fill(m, c, D).w[0], what, D, 1, 3 + eight);
        }
    }
}

using Mask = std::vector<Row4>;     // D rows

// a pixel flood fill with an explicit stack
static Mask naive_flood(const Mask &m, int D, int sy, int sx, bool eight)
{
    Mask f(D, kZero);
    if (!get(m[sy], sx)) return f;
    std::vector<int> stack;
    set(f[sy], sx);
    stack.push_back(sy * D + sx);
    while (!stack.empty()) {
        const int y = stack.back() / D, x = stack.back() % D;
        stack.pop_back();
        for (int ey = -1; ey <= 1; ++ey)
            for (int ex = -1; ex <= 1; ++ex) {
                if ((!ey && !ex) || (!eight && ey && ex)) continue;
                const int v = y + ey, u = x + ex;
                if (v < 0 || v >= D || u < 0 || u >= D || !get(m[v], u) || get(f[v], u)) continue;
                set(f[v], u);
                stack.push_back(v * D + u);
            }
    }
    return f;
}

// the region grow as the kernels run it: every row from the same old state, until a sweep adds no bit.  Returns the sweeps.
static long long grow(const Mask &m, int D, int sy, int sx, bool eight, bool one_word, Mask &f)
{
    f.assign(D, kZero);
    if (get(m[sy], sx)) set(f[sy], sx);
    long long sweeps = 0;
    for (;;) {
        Mask nf(D, kZero);
        bool changed = false;
        for (int r = 0; r < D; ++r) {
            const Row4 &up = r > 0 ? f[r - 1] : kZero, &dn = r + 1 < D ? f[r + 1] : kZero;
            if (one_word)
                nf[r].w[0] = sweep_row1(m[r].w[0], f[r].w[0], up.w[0], dn.w[0], eight);
            else
                nf[r] = sweep_row4(m[r], f[r], up, dn, eight);
            changed = changed || differ4(nf[r], f[r]);
        }
        f.swap(nf);
        ++sweeps;
        if (!changed) return sweeps;
    }
}

static long long pixels(const Mask &f)
{
    long long n = 0;
    for (const Row4 &r : f)
        for (int k = 0; k < 4; ++k) n += __builtin_popcountll(r.w[k]);
    return n;
}

static long long check_grow(const Mask &m, int D, int sy, int sx, const char *what)
{
    long long sweeps8 = 0;
    for (int eight = 0; eight < 2; ++eight) {
        const Mask want = naive_flood(m, D, sy, sx, eight != 0);
        Mask f;
        const long long sweeps = grow(m, D, sy, sx, eight != 0, false, f);
        bool ok = true;
        for (int r = 0; r < D; ++r) ok = ok && same(f[r], want[r]);
        expect(ok, what, D, eight, 4);
        expect(sweeps <= pixels(want) + 1, "sweeps within the bound", D, sweeps, pixels(want));
        if (D <= 64) {
            const long long s1 = grow(m, D, sy, sx, eight != 0, true, f);
            ok = s1 == sweeps;
            for (int r = 0; r < D; ++r) ok = ok && same(f[r], want[r]);
            expect(ok, what, D, eight, 1);
        }
        sweeps8 = sweeps;
    }
    return sweeps8;
}

static Mask comb(int D, bool vertical)
{
    // corridors along every second column, joined at alternating ends; transposed for the horizontal one
    std::vector<std::vector<char>> p(D, std::vector<char>(D, 0));
    for (int x = 0, k = 0; x < D; x += 2, ++k) {
        for (int y = 0; y < D; ++y) p[y][x] = 1;
        if (x + 1 < D) p[k % 2 ? 0 : D - 1][x + 1] = 1;
    }
    Mask m(D, kZero);
    for (int y = 0; y < D; ++y)
        for (int x = 0; x < D; ++x)
            if (vertical ? p[y][x] : p[x][y]) set(m[y], x);
    return m;
}

static Mask disc(int R, bool vertical_comb)
{
    const int D = 2 * R + 1;
    Mask m(D, kZero);
    for (int y = -R; y <= R; ++y)
        for (int x = -R; x <= R; ++x)
            if (y * y + x * x <= R * R && (!vertical_comb || x % 2 == 0)) set(m[y + R], x + R);
    if (vertical_comb)                      // every corridor joined to the next at alternating ends of the shorter chord
        for (int x = -R + R % 2, k = 0; x + 2 <= R; x += 2, ++k) {
            const int a = x * x > (x + 2) * (x + 2) ? x : x + 2;          // the shorter of the two chords
            int h = 0;
            while ((h + 1) * (h + 1) + a * a <= R * R) ++h;
            while (h > 0 && h * h + (x + 1) * (x + 1) > R * R) --h;
            set(m[R + (k % 2 ? -h : h)], x + 1 + R);
        }
    return m;
}

int main()
{
    const int sizes[] = {5, 17, 63, 64, 65, 127, 129, 255};
    for (int D : sizes) {
        // the row operations: random rows, all-ones rows, single bits at the word edges
        for (int t = 0; t < 400; ++t) {
            const unsigned pm = (unsigned)(rnd() % 1001u);
            check_row_ops(random_row(D, pm), random_row(D, (unsigned)(rnd() % 300u)), random_row(D, 300), random_row(D, 300), D, "random rows");
        }
        const Row4 ones = random_row(D, 1000);
        const int edges[] = {0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, 253, 254};
        for (int e : edges) {
            if (e >= D) continue;
            Row4 one = kZero;
            set(one, e);
            check_row_ops(ones, one, kZero, kZero, D, "all ones, one seed");
            check_row_ops(ones, kZero, one, kZero, D, "all ones, one bit above");
            check_row_ops(ones, kZero, kZero, one, D, "all ones, one bit below");
            check_row_ops(one, one, kZero, kZero, D, "single bit");
            check_row_ops(random_row(D, 700), one, one, one, D, "dense row, bits at a word edge");
            Row4 gap = ones;                 // all ones but the bit at the edge: the run must stop there
            gap.w[e >> 6] &= ~(1ull << (e & 63));
            check_row_ops(gap, random_row(D, 30), one, one, D, "gap at a word edge");
        }
        check_row_ops(ones, ones, ones, ones, D, "all ones");
        check_row_ops(ones, kZero, kZero, kZero, D, "no seed");
        // the region grow
        const unsigned dens[] = {300, 420, 500, 600, 750, 1000};
        for (unsigned pm : dens)
            for (int t = 0; t < (D > 100 ? 3 : 10); ++t) {
                Mask m(D);
                for (int r = 0; r < D; ++r) m[r] = random_row(D, pm);
                const int sy = (int)(rnd() % (unsigned)D), sx = (int)(rnd() % (unsigned)D);
                set(m[sy], sx);
                check_grow(m, D, sy, sx, "random mask");
            }
        check_grow(comb(D, true), D, D / 2 - (D / 2) % 2, 0, "vertical comb");
        check_grow(comb(D, true), D, 0, D - 1 - (D - 1) % 2, "vertical comb, far end");
        check_grow(comb(D, false), D, 0, D / 2, "horizontal comb");
        Mask single(D, kZero);
        set(single[D - 1], D - 1);
        check_grow(single, D, D - 1, D - 1, "single pixel in the corner");
        Mask empty(D, kZero);
        check_grow(empty, D, D / 2, D / 2, "empty mask");
    }
    // the sweep counts quoted in DESIGN.md, from this emulation of the scheme
    std::printf("sweeps: filled disc R 25: %lld, R 127: %lld; vertical comb over the disc R 127: %lld, over the square D 255: %lld\n",
                check_grow(disc(25, false), 51, 25, 25, "disc 25"), check_grow(disc(127, false), 255, 127, 127, "disc 127"),
                check_grow(disc(127, true), 255, 127, 127, "comb disc 127"), check_grow(comb(255, true), 255, 0, 0, "comb 255"));
    std::printf("%lld checks, %lld mismatches\n", checks, bad);
    return bad ? 1 : 0;
}
