// The Float64 part of the shape rule (csrc/pdog_shape.hpp: steps 7 and 8 of include/pawsome_shape.h) under the host compiler,
// against tabulated cases: masks whose moments are known in closed form (a single pixel, a row of pixels, a column, a
// diagonal, a disc, the empty mask, the largest sums the rule allows) and walks whose headings follow from the rule's text
// (motion forwards and backwards, a stop, a NaN in between, ties, the wrap to (-pi, pi]).
// Prints "<n> checks, <m> mismatches"; exits non-zero on any.
#include "pdog_shape.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace pdog::shape;

static long long bad = 0, checks = 0;
static void expect(bool ok, const char *what, double got, double want)
{
    ++checks;
    if (!ok && bad++ < 20) std::printf("MISMATCH %s: got %.17g, expected %.17g\n", what, got, want);
}
static void close_to(const char *what, double got, double want, double tol = 1e-12)
{
    expect(std::fabs(got - want) <= tol, what, got, want);
}

// the eight sums of a mask given as offsets
static void sums_of(const std::vector<int> &dy, const std::vector<int> &dx, int32_t s[8])
{
    for (int k = 0; k < 8; ++k) s[k] = 0;
    for (size_t k = 0; k < dy.size(); ++k) {
        s[0] += 1;
        s[1] += dy[k];
        s[2] += dx[k];
        s[3] += dy[k] * dy[k];
        s[4] += dy[k] * dx[k];
        s[5] += dx[k] * dx[k];
    }
    s[6] = 128;
    s[7] = 100;
}

int main()
{
    int32_t s[8];
    double o[6];
    // the empty mask: six NaN
    sums_of({}, {}, s);
    derive(s, 5, 7, o);
    for (int k = 0; k < 6; ++k) expect(o[k] != o[k], "empty mask is NaN", o[k], 0.0);
    // one pixel: a unit square, both moments 1/12, axes 4 sqrt(1/12), theta 0
    sums_of({0}, {0}, s);
    derive(s, 5, 7, o);
    close_to("pixel row", o[0], 5.0);
    close_to("pixel col", o[1], 7.0);
    expect(o[2] == 0.0, "pixel theta", o[2], 0.0);
    close_to("pixel major", o[3], 4.0 * std::sqrt(1.0 / 12.0));
    close_to("pixel minor", o[4], 4.0 * std::sqrt(1.0 / 12.0));
    close_to("pixel width", o[5], 2.0 * std::sqrt(1.0 / kPi));
    // a row of m pixels at dx = 3 ... 3 + m - 1, dy = -2: a 1 x m rectangle, theta 0, moments (m*m)/12 and 1/12
    for (int m = 2; m <= 40; ++m) {
        std::vector<int> dy(m, -2), dx(m);
        for (int k = 0; k < m; ++k) dx[k] = 3 + k;
        sums_of(dy, dx, s);
        derive(s, 10, 20, o);
        close_to("row: row", o[0], 8.0);
        close_to("row: col", o[1], 20.0 + 3.0 + (m - 1) / 2.0);
        expect(o[2] == 0.0, "row: theta", o[2], 0.0);
        close_to("row: major", o[3], 4.0 * std::sqrt(m * (double)m / 12.0), 1e-11);
        close_to("row: minor", o[4], 4.0 * std::sqrt(1.0 / 12.0), 1e-9); // (a difference of nearly equal numbers under the root)
        close_to("row: width", o[5], 2.0 * std::sqrt(m / kPi));
        // the same as a column: theta pi/2 (the end of the range that belongs to it)
        sums_of(dx, dy, s);
        derive(s, 10, 20, o);
        close_to("column: theta", o[2], kPi / 2.0);
        close_to("column: major", o[3], 4.0 * std::sqrt(m * (double)m / 12.0), 1e-11);
        // the diagonals: +col towards +row is +pi/4, the other one -pi/4
        std::vector<int> d(m), e(m);
        for (int k = 0; k < m; ++k) { d[k] = k; e[k] = -k; }
        sums_of(d, d, s);
        derive(s, 1, 1, o);
        close_to("diagonal: theta", o[2], kPi / 4.0);
        sums_of(e, d, s);
        derive(s, 1, 1, o);
        close_to("anti-diagonal: theta", o[2], -kPi / 4.0);
    }
    // the disc of radius 5 seen from 3 rows below its centre: the centroid is the disc's centre, the axes are equal
    {
        std::vector<int> dy, dx;
        for (int y = -5; y <= 5; ++y)
            for (int x = -5; x <= 5; ++x)
                if (y * y + x * x <= 25) { dy.push_back(y - 3); dx.push_back(x); }
        sums_of(dy, dx, s);
        expect(s[0] == 81, "disc n", s[0], 81);
        derive(s, 64, 83, o);
        close_to("disc row", o[0], 61.0);
        close_to("disc col", o[1], 83.0);
        close_to("disc major = minor", o[3], o[4]);
        close_to("disc width", o[5], 10.155412503859613, 1e-12);
    }
    // the largest sums: the whole disc of radius 127 (no overflow anywhere: UBSan watches the int64 products)
    {
        std::vector<int> dy, dx;
        for (int y = -127; y <= 127; ++y)
            for (int x = -127; x <= 127; ++x)
                if (y * y + x * x <= 127 * 127) { dy.push_back(y); dx.push_back(x); }
        sums_of(dy, dx, s);
        expect(s[3] > 0 && s[5] > 0 && s[3] == s[5], "disc 127 sums", s[3], s[5]);
        derive(s, 200, 300, o);
        close_to("disc 127 row", o[0], 200.0);
        close_to("disc 127 major", o[3], 254.0, 1.5);
        close_to("disc 127 major = minor", o[3], o[4], 1e-9);
        // and a half disc, the most lopsided mask: the first moments at their largest
        std::vector<int> hy, hx;
        for (size_t k = 0; k < dy.size(); ++k)
            if (dx[k] >= 0) { hy.push_back(dy[k]); hx.push_back(dx[k]); }
        sums_of(hy, hx, s);
        derive(s, 200, 300, o);
        close_to("half disc theta", o[2], kPi / 2.0, 1e-9);
        expect(o[1] > 300.0 + 50.0 && o[1] < 300.0 + 60.0, "half disc col", o[1], 354.0); // 4R / (3 pi) = 53.9
    }
    // ---- headings ----
    const double th = 0.5, nan = std::nan("");
    {
        //                 start   +col     rest     NaN      rest     -col     rest
        const int32_t ij[] = {10, 10, 10, 14, 10, 14, 10, 14, 10, 14, 10, 9, 10, 9};
        const double theta[] = {th, th, th, nan, th, th, th};
        double out[7];
        headings(theta, ij, 7, 1.0, out);
        close_to("first step: theta itself", out[0], th);
        close_to("along +col", out[1], th);
        close_to("kept at rest", out[2], th);
        expect(out[3] != out[3], "NaN theta", out[3], nan);
        close_to("kept across the NaN", out[4], th);
        close_to("turned by pi", out[5], th - kPi);
        close_to("kept turned", out[6], th - kPi);
    }
    {
        // previous heading theta + pi, then at rest: the flipped side is kept whatever theta does within pi/2
        const int32_t ij[] = {10, 10, 10, 5, 10, 5, 10, 5};
        const double theta[] = {0.2, 0.2, -0.9, 1.5};
        double out[4];
        headings(theta, ij, 4, 1.0, out);
        close_to("flip", out[1], 0.2 - kPi);
        close_to("rest 1", out[2], -0.9 + kPi); // within pi/2 of 0.2 - pi: -0.9 + pi - 2 pi = -0.9 - pi is the same direction; in (-pi, pi] it is -0.9 + pi
        close_to("rest 2", out[3], 1.5); // 1.5 lies 0.74 from -0.9 + pi = 2.24: theta itself
        // min_step: a step shorter than it counts as rest
        const int32_t ik[] = {10, 10, 10, 12, 10, 11};
        const double tk[] = {0.0, 0.0, 0.0};
        double ok[3];
        headings(tk, ik, 3, 2.0, ok);
        close_to("min_step: moved", ok[1], 0.0);
        close_to("min_step: a short step back keeps the heading", ok[2], 0.0);
        headings(tk, ik, 3, 1.0, ok);
        close_to("min_step 1: the step back turns it", ok[2], kPi);
        // a displacement perpendicular to the axis: the dot product is (nearly) zero and either side is a valid answer; an
        // axis at exactly pi/2 moving up is -pi/2
        const int32_t iu[] = {10, 10, 5, 10};
        const double tu[] = {kPi / 2.0, kPi / 2.0};
        double ou[2];
        headings(tu, iu, 2, 1.0, ou);
        close_to("upwards", ou[1], -kPi / 2.0);
    }
    std::printf("%lld checks, %lld mismatches\n", checks, bad);
    return bad ? 1 : 0;
}
