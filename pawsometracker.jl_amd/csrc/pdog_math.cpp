// pdog_math.cpp — the part of the C ABI (include/pawsome_dog.h) that needs no GPU: the thread's error text, the
// reference's Float64 kernel arithmetic (src/PawsomeTracker.jl:30, :41-43), mode(_img) (:47) and the window
// tile packer.  Plain C++: no HIP, no kernel header (pdog_host.hpp says why), so tools/asan_host.sh sanitises it alone.
#include "pdog_host.hpp"
#include "pdog_exclusive.hpp"
#include "pdog_motion.hpp"
#include "pdog_shape.hpp"
#include "pdog_frame_blobs.hpp"
#include "../../include/pawsome_exclusive.h"
#include "../../include/pawsome_motion.h"
#include "../../include/pawsome_shape.h"
#include "../../include/pawsome_frame_blobs.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <emmintrin.h>

namespace pdog {

namespace {
thread_local std::string g_err;
}

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

// What the exclusive step's three entry points refuse alike (include/pawsome_exclusive.h); PDOG_E_ARG in `who`'s name.
int check_exclusive(const char *who, int n_groups, int n_targets, int k, double min_ratio)
{
    if (n_groups < 1 || (long long)n_groups * n_targets > 0x7fffffffLL) return fail(PDOG_E_ARG, std::string(who) + ": bad number of groups");
    if (n_targets < 1 || n_targets > exclusive::kMaxTargets) return fail(PDOG_E_ARG, std::string(who) + ": n_targets = " + std::to_string(n_targets) + " lies outside 1 ... 32");
    if (k < 1 || k > PDOG_PEAKS_MAX_K) return fail(PDOG_E_ARG, std::string(who) + ": k = " + std::to_string(k) + " lies outside 1 ... 32");
    if (!(min_ratio >= 0.0 && min_ratio <= 1.0)) return fail(PDOG_E_ARG, std::string(who) + ": min_ratio lies outside [0, 1]");
    return PDOG_OK;
}

// What the motion step's entry points (include/pawsome_motion.h) refuse beyond check_exclusive.
int check_motion(const char *who, double min_response, int coast)
{
    if (!(min_response >= 0.0 && min_response <= 3.4028234663852886e38)) return fail(PDOG_E_ARG, std::string(who) + ": min_response must be finite and not negative");
    if (coast < 0) return fail(PDOG_E_ARG, std::string(who) + ": coast = " + std::to_string(coast) + " is negative");
    return PDOG_OK;
}

double sigma_of(double tw) { return tw / (2.0 * std::sqrt(2.0 * std::log(2.0))); } // :30
int kernel_len_of_sigma(double s) { return 4 * (int)std::ceil(s * std::sqrt(2.0)) + 1; } // Kernel.DoG
void gaussian_1d(double s, int l, double *g)
{ // KernelFactors.gaussian: exp(-x²/2σ²) / sum
#pragma clang fp contract(off)
    const int w = l >> 1;
    for (int x = -w; x <= w; ++x) g[x + w] = std::exp(-((double)x * (double)x) / (2.0 * s * s));
    double sum = 0.0;
    for (int i = 0; i < l; ++i) sum += g[i];
    for (int i = 0; i < l; ++i) g[i] /= sum;
}

// The reference's dense kernel, K = dir·(g₊⊗g₊ − g₋⊗g₋) (src/PawsomeTracker.jl:41-43), column-major, every product and
// the difference rounded separately as Julia evaluates them: a compiler may contract a·b − c·d into an FMA, which
// changes last bits — and last bits are exactly what decides the ties exact mode exists for.
void dense_dog_kernel(const double *gp, const double *gm, int l, bool darker, double *K)
{
#pragma clang fp contract(off)
    const double dir = darker ? -1.0 : 1.0;
    for (int j = 0; j < l; ++j)
        for (int i = 0; i < l; ++i) {
            const double a = gp[i] * gp[j];
            const double b = gm[i] * gm[j];
            K[i + (size_t)l * j] = dir * (a - b);
        }
}

// ---- exact mode's FP32 error bounds, per kernel family (dog_exact.hpp: the guarantee) ----
// An FMA chain ŝ_i = fl(ŝ_{i−1} + a_i·b̂_i) satisfies |ŝ_n − s_n| ≤ u·(1 + u)·Σ_i |ŝ_i| (each step rounds its own result once), and
// |ŝ_i| ≤ V·W_i·(1 + nu) where W_i = Σ_{j ≤ i} |b_j|·max|a_j|/V is the cumulative tap weight IN THE ORDER THE KERNEL ADDS THEM.  The
// Gaussians sum to 1, so Σ_i W_i is far below the chain length n that the order-blind bound n·u·V charges: the kernels add the
// smallest taps (the kernel's edges) first.  The factors below are Σ_i W_i evaluated numerically over the tracker's own Float64
// taps for each family's operation order (+1 per rounded tap table, +2 for a final channel addition); δ = u·(V/255)·F·1.02:
//   row pass, symmetric pairs from the edge inwards, centre last (roll, thin, fused, tiled, two-pass):  W_i = Σ_{j ≤ i} 2g[j]
//   row pass, plain chain over the l taps (ring kernels; the refinement's FP32 rescan):               W_i = Σ_{j ≤ i} g[j]
//   column pass, one f32 per output taking (+, −) terms alternately (roll, thin, folded column, rescan): both cumulative weights per step
//   column pass, the two Gaussians in separate chains, added at the end (ring, fused, tiled, two-pass)
//   two-pass: every chain is one trip of the register ring long, the chains' sums are added up (dog_twopass.hpp) — per chain its own
//   cumulative weights from zero, plus the running total's weight per addition (twopass_factor, pawsome_dog.hip)
// l = 65: 157 (roll) / 94 (fused, tiled) / 138 (ring) against the order-blind 6l + 4 = 394;  l = 293 two-pass: 72 against 1762.
// tests/fp32_restatement.py states the same orders as data and sums the same factors over them; tests/test_gpu_fp32_order.py holds the
// kernels' response maps to those orders bit for bit and the thresholds built from the factors below to the ones derived there.
ExactFactors exact_factors(const std::vector<double> &gp, const std::vector<double> &gm)
{
    const int l = (int)gp.size(), H = l / 2;
    auto row_sym = [&](const std::vector<double> &g) { double W = 0, F = 0; for (int k = 0; k <= H; ++k) { W += (k < H ? 2.0 : 1.0) * g[k]; F += W; } return F + 1.0; };
    auto row_plain = [&](const std::vector<double> &g) { double W = 0, F = 0; for (int k = 0; k < l; ++k) { W += g[k]; F += W; } return F + 1.0; };
    double Gp = 0, Gm = 0, c_sep = 4.0, c_int = 2.0;
    for (int t = 0; t < l; ++t) {
        Gp += gp[t];
        c_int += Gp + Gm; // after the + term of tap t
        Gm += gm[t];
        c_int += Gp + Gm; // after the − term
        c_sep += Gp + Gm;
    }
    ExactFactors f;
    f.sym_int = row_sym(gp) + row_sym(gm) + c_int;
    f.sym_sep = row_sym(gp) + row_sym(gm) + c_sep;
    f.ring = row_plain(gp) + row_plain(gm) + c_sep;
    f.rescan = row_plain(gp) + row_plain(gm) + c_int;
    return f;
}

// ‖K‖₂ (Frobenius) of the dense kernel K = g₊⊗g₊ − g₋⊗g₋, for the pre-pass's Cauchy–Schwarz bound (dog_prune.hpp):
// ‖K‖₂² = (Σg₊²)² + (Σg₋²)² − 2(Σg₊g₋)², in double from the tracker's own f32-rounded taps — and from the Float64 taps the
// error bound δ is stated against; the larger of the two, rounded UP to the next float.
double dog_kernel_norm_up(const std::vector<double> &gp, const std::vector<double> &gm)
{
    auto norm = [&](bool f32) {
        double pp = 0, mm = 0, pm = 0;
        for (size_t k = 0; k < gp.size(); ++k) {
            const double a = f32 ? (double)(float)gp[k] : gp[k], b = f32 ? (double)(float)gm[k] : gm[k];
            pp += a * a; mm += b * b; pm += a * b;
        }
        return std::sqrt(std::max(0.0, pp * pp + mm * mm - 2.0 * pm * pm));
    };
    const double n = std::max(norm(true), norm(false));
    return (double)std::nextafter((float)n, 2.0f); // (the float nearest to n may lie below it; its successor does not)
}

// The weights of the pre-pass's second stage (dog_prune.hpp, "the cell bound").  With the tile cut into 8 × 8 cells, an output
// at offset (i, j) inside its own cell takes from the input cell (dy, dx) cells further on the kernel rows
// [8dy − i, 8dy − i + 8) ∩ [0, l) and the like columns.  K = g₊⊗g₊ − g₋⊗g₋, so the Σ K² of such a box is
// A_r·A_c + B_r·B_c − 2·C_r·C_c with A, B, C the sums of g₊², g₋² and g₊g₋ over the row and the column range: prefix sums.
RefineBoxes::RefineBoxes(const std::vector<double> &gp, const std::vector<double> &gm, bool f32) : ns(refine_span((int)gp.size()))
{
    const int l = (int)gp.size();
    std::vector<double> pp(l + 1, 0.0), mm(l + 1, 0.0), pm(l + 1, 0.0);
    for (int k = 0; k < l; ++k) {
        const double a = f32 ? (double)(float)gp[k] : gp[k], b = f32 ? (double)(float)gm[k] : gm[k];
        pp[k + 1] = pp[k] + a * a;
        mm[k + 1] = mm[k] + b * b;
        pm[k + 1] = pm[k] + a * b;
    }
    A.resize((size_t)ns * 8); B.resize((size_t)ns * 8); C.resize((size_t)ns * 8);
    for (int d = 0; d < ns; ++d)
        for (int i = 0; i < 8; ++i) {
            const int lo = std::min(std::max(8 * d - i, 0), l), hi = std::min(std::max(8 * d - i + 8, 0), l);
            A[d * 8 + i] = pp[hi] - pp[lo];
            B[d * 8 + i] = mm[hi] - mm[lo];
            C[d * 8 + i] = pm[hi] - pm[lo];
        }
}
double RefineBoxes::norm2(int dy, int i, int dx, int j) const
{
    double ab = A[dy * 8 + i] * A[dx * 8 + j];
    const double bb = B[dy * 8 + i] * B[dx * 8 + j], cc = C[dy * 8 + i] * C[dx * 8 + j];
    ab = ab + bb;
    return ab - 2.0 * cc;
}
// Wq[dy][dx] = ⌈2¹²·W/‖K‖₂⌉, W² the largest box sum over the 64 offsets and over the f32-rounded and the Float64 taps (as
// dog_kernel_norm_up takes the larger norm), plus 1e-14·‖K‖₂² — a box sum is a difference of products near 1e-4 and may come
// out 1e-20 low; the slack is 4e-4 of a weight's unit at most.  Every rounding errs upwards.  tests/prune_refine_restatement.py
// restates this function operation for operation (no product here is fused with an addition: the reference arithmetic of
// this file is compiled for a target without FMA).
std::vector<uint32_t> dog_refine_weights(const std::vector<double> &gp, const std::vector<double> &gm, double norm_up)
{
    const RefineBoxes f32(gp, gm, true), f64(gp, gm, false);
    const int ns = f32.ns;
    std::vector<uint32_t> wq((size_t)ns * ns);
    for (int dy = 0; dy < ns; ++dy)
        for (int dx = 0; dx < ns; ++dx) {
            double w2 = 0.0;
            for (const RefineBoxes *t : {&f32, &f64})
                for (int i = 0; i < 8; ++i)
                    for (int j = 0; j < 8; ++j) w2 = std::max(w2, t->norm2(dy, i, dx, j));
            w2 = w2 + 1e-14 * (norm_up * norm_up);
            wq[(size_t)dy * ns + dx] = (uint32_t)std::ceil(4096.0 * (std::sqrt(w2) / norm_up));
        }
    return wq;
}

// One window's padded tile, (n1+l-1) rows of `pitch` bytes: the frame rectangle the functor reads, with the
// PaddedView fill (:48) materialised wherever the rectangle leaves the frame.  Tile row a, column b is the
// padded frame at 1-based (g1 - r1 - l÷2 + a, g2 - r2 - l÷2 + b).
void pack_tile_geo(const uint8_t *frame, int fh, int fw, int64_t row_stride, int fill, int L, int r1, int r2, int g1, int g2,
                   uint8_t *dst, int64_t pitch, bool stream)
{
    const int hw = L >> 1, th = 2 * r1 + 1 + 2 * hw, tw = 2 * r2 + 1 + 2 * hw;
    const int i0 = g1 - r1 - hw - 1, j0 = g2 - r2 - hw - 1;        // 0-based frame coordinates of tile (0, 0)
    const int jl = std::min(tw, std::max(0, -j0));                 // columns left of the frame
    const int jr = std::max(jl, std::min(tw, fw - j0));            // first column right of the frame
    // stream: the tile goes to pinned staging that only the DMA engine reads next — assemble each row in a small
    // buffer and write it with non-temporal stores, so the copy engine finds the data in DRAM instead of having to
    // snoop dirty lines out of this core's cache
    const bool nt = stream && pitch % 16 == 0 && pitch <= 4096 && ((uintptr_t)dst & 15) == 0;
    alignas(16) uint8_t rowbuf[4096];
    for (int a = 0; a < th; ++a) {
        uint8_t *out = dst + (size_t)a * pitch;
        uint8_t *row = nt ? rowbuf : out;
        const int gi = i0 + a;
        if (gi < 0 || gi >= fh) {
            std::memset(row, fill, (size_t)pitch);
        } else {
            if (jl) std::memset(row, fill, (size_t)jl);
            if (jr > jl) std::memcpy(row + jl, frame + (size_t)gi * row_stride + (j0 + jl), (size_t)(jr - jl));
            if (pitch > jr) std::memset(row + jr, fill, (size_t)(pitch - jr));
        }
        if (nt)
            for (int64_t k = 0; k < pitch; k += 16)
                _mm_stream_si128((__m128i *)(out + k), _mm_load_si128((const __m128i *)(rowbuf + k)));
    }
    if (nt) _mm_sfence(); // the non-temporal stores are globally visible before the caller publishes the tile
}

int chain_table_lengths(const char *who, const int32_t *h_table, int n_steps, int n_clips, int n_frames, int32_t *out_len, int *max_len)
{
    *max_len = 0;
    for (int c = 0; c < n_clips; ++c) {
        const int32_t *row = h_table + (size_t)c * n_steps;
        int len = 0;
        while (len < n_steps && row[len] >= 0) ++len;
        for (int k = 0; k < n_steps; ++k)
            if (row[k] >= n_frames || (k > len && row[k] >= 0))
                return fail(PDOG_E_ARG, std::string(who) + ": entry " + std::to_string(k) + " of clip " + std::to_string(c) +
                                            (row[k] >= n_frames ? " names a frame outside the stack" : " follows a negative one"));
        out_len[c] = len;
        *max_len = std::max(*max_len, len);
    }
    return PDOG_OK;
}

int check_table_walk(TableWalk &w, std::vector<int32_t> &len)
{
    const long long n = (long long)w.n_rows * w.windows;
    if (int rc = check_stack(w.who, w.fw, w.n_frames, w.row_stride, w.frame_stride,
                             w.n_steps > 0 && w.n_rows > 0 && w.windows > 0 && n <= 0x7fffffffLL && n * w.n_steps <= 0x7fffffffLL))
        return rc;
    if (n * w.n_strips > 0x7ffffff0LL) return fail(PDOG_E_ARG, std::string(w.who) + ": batch too large"); // (judged before the first launch)
    if (w.first != 0 && w.first != 1) return fail(PDOG_E_ARG, std::string(w.who) + ": first must be 0 or 1");
    if (len.size() < (size_t)w.n_rows) len.resize((size_t)w.n_rows);
    return chain_table_lengths(w.who, w.h_table, w.n_steps, w.n_rows, w.n_frames, len.data(), &w.max_len);
}

void fill_table(const int32_t *h_table, const int32_t *len, const TableShape &s, int32_t *out)
{
    const size_t cells = table_cells(s);
    if (!s.windows) std::copy_n(h_table, cells, out);
    else
        for (int r = 0; r < s.n_rows; ++r) {
            const int32_t *row = h_table + (size_t)r * s.n_steps;
            for (int k = 0; k < s.max_len; ++k)
                std::fill_n(out + ((size_t)k * s.n_rows + r) * s.windows, s.windows, k < len[r] ? row[k] : (len[r] ? row[len[r] - 1] : 0));
        }
    std::copy_n(len, s.n_rows, out + cells);
}

} // namespace pdog

using namespace pdog;

extern "C" {

const char *pdog_last_error(void) { return g_err.c_str(); }

double pdog_sigma(double target_width) { return sigma_of(target_width); }
int pdog_default_window(double target_width) { return 4 * (int)std::ceil(sigma_of(target_width)) + 1; } // :64-68
int pdog_kernel_len(double target_width) { return kernel_len_of_sigma(sigma_of(target_width)); }

int pdog_gaussian_taps(double target_width, int which, double *out, int cap)
{
    if (!out || (which != 0 && which != 1) || !(target_width > 0)) return fail(PDOG_E_ARG, "pdog_gaussian_taps: bad argument");
    const double s = sigma_of(target_width);
    const int l = kernel_len_of_sigma(s);
    if (cap < l) return fail(PDOG_E_ARG, "pdog_gaussian_taps: buffer too small");
    gaussian_1d(which ? s * std::sqrt(2.0) : s, l, out);
    return PDOG_OK;
}

int pdog_dense_kernel(double target_width, int darker_target, double *out, int cap)
{
    if (!out || !(target_width > 0)) return fail(PDOG_E_ARG, "pdog_dense_kernel: bad argument");
    const double s = sigma_of(target_width);
    const int l = kernel_len_of_sigma(s);
    if ((long long)cap < (long long)l * l) return fail(PDOG_E_ARG, "pdog_dense_kernel: buffer too small");
    std::vector<double> gp(l), gm(l);
    gaussian_1d(s, l, gp.data());
    gaussian_1d(s * std::sqrt(2.0), l, gm.data());
    dense_dog_kernel(gp.data(), gm.data(), l, darker_target != 0, out);
    return PDOG_OK;
}

int pdog_mode_u8(const uint8_t *img, int h, int w, int64_t row_stride, int *out_mode)
{
    if (!img || !out_mode || h <= 0 || w <= 0 || row_stride < w) return fail(PDOG_E_ARG, "pdog_mode_u8: bad argument");
    // StatsBase.mode over the h×w view, column-major scan (row index fastest): per-value
    // running counts; the winner is the value whose count FIRST exceeds the running maximum.
    // Equivalent single pass per column block: counts are order dependent only through ties,
    // so keep the literal scan order.
    int64_t cnt[256];
    std::memset(cnt, 0, sizeof cnt);
    int64_t mc = 0;
    int mv = img[0];
    for (int j = 0; j < w; ++j) {
        const uint8_t *p = img + j;
        for (int i = 0; i < h; ++i) {
            const int v = p[(int64_t)i * row_stride];
            const int64_t c = ++cnt[v];
            if (c > mc) { mc = c; mv = v; }
        }
    }
    *out_mode = mv;
    return PDOG_OK;
}

// The tile packer as a host-only entry (no GPU): what the host paths hand to the kernels, checkable on a CPU box.
int pdog_window_tile(const uint8_t *h_frame, int frame_h, int frame_w, int64_t row_stride, int fill, double target_width,
                     int win_h, int win_w, const int32_t guess[2], uint8_t *h_out, int64_t out_pitch)
{
    if (!h_frame || !guess || !h_out) return fail(PDOG_E_ARG, "pdog_window_tile: null pointer");
    if (frame_h <= 0 || frame_w <= 0 || row_stride < frame_w || fill < 0 || fill > 255 || win_h <= 0 || win_w <= 0 || !(target_width > 0))
        return fail(PDOG_E_ARG, "pdog_window_tile: bad argument");
    const int L = kernel_len_of_sigma(sigma_of(target_width)), r1 = win_h / 2, r2 = win_w / 2;
    if (out_pitch < 2 * r2 + L) return fail(PDOG_E_ARG, "pdog_window_tile: out_pitch smaller than the tile width");
    pack_tile_geo(h_frame, frame_h, frame_w, row_stride, fill, L, r1, r2, guess[0], guess[1], h_out, out_pitch);
    return PDOG_OK;
}

// The grouping plan of pdog_clips_track (pawsome_clips.hip), host arithmetic only.  A clip takes part when it has a frame to
// compute (len > first); the participants are sorted by (fill ascending, len descending, clip ascending), so that a group
// is one run of equal fills and the clips of a group that are still active at frame k are a prefix of it.
int pdog_clips_plan(int n_clips, int n_frames, int first, const int32_t *h_fill, const int32_t *h_len, int32_t *out_order,
                    int32_t *out_group_fill, int32_t *out_group_start, int *out_n_groups)
{
    if (!out_order || !out_group_fill || !out_group_start || !out_n_groups) return fail(PDOG_E_ARG, "pdog_clips_plan: null output");
    if (n_clips <= 0 || n_frames <= 0 || (first != 0 && first != 1)) return fail(PDOG_E_ARG, "pdog_clips_plan: bad size or first");
    for (int c = 0; c < n_clips; ++c) { // everything is checked before anything is written
        if (h_fill && (h_fill[c] < 0 || h_fill[c] > 255)) return fail(PDOG_E_ARG, "pdog_clips_plan: fill of clip " + std::to_string(c) + " outside 0 ... 255");
        if (h_len && (h_len[c] < 0 || h_len[c] > n_frames)) return fail(PDOG_E_ARG, "pdog_clips_plan: length of clip " + std::to_string(c) + " outside 0 ... n_frames");
    }
    auto len_of = [&](int c) { return h_len ? (int)h_len[c] : n_frames; };
    auto fill_of = [&](int c) { return h_fill ? (int)h_fill[c] : -1; };
    int n = 0;
    for (int c = 0; c < n_clips; ++c)
        if (len_of(c) > first) out_order[n++] = c;
    std::sort(out_order, out_order + n, [&](int32_t a, int32_t b) {
        if (fill_of(a) != fill_of(b)) return fill_of(a) < fill_of(b);
        if (len_of(a) != len_of(b)) return len_of(a) > len_of(b);
        return a < b;
    });
    int ng = 0;
    for (int p = 0; p < n; ++p)
        if (p == 0 || fill_of(out_order[p]) != fill_of(out_order[p - 1])) {
            out_group_fill[ng] = fill_of(out_order[p]);
            out_group_start[ng++] = p;
        }
    out_group_start[ng] = n;
    *out_n_groups = ng;
    return PDOG_OK;
}

// ---- start, stop, fps as host arithmetic (include/pawsome_video.h) ----
namespace {
// n = round(Int, fps * (stop - start)), src/PawsomeTracker.jl:150-151 (nearbyint: ties to even in the default rounding mode)
int time_axis_len(const char *who, double start, double stop, double fps, int *n)
{
    if (!(stop > start) || !(fps > 0.0)) return fail(PDOG_E_ARG, std::string(who) + ": stop <= start or fps <= 0");
    const double r = std::nearbyint(fps * (stop - start));
    if (!(r >= 1.0) || r > 2147483647.0) return fail(PDOG_E_ARG, std::string(who) + ": round(fps * (stop - start)) outside 1 ... 2^31 - 1");
    *n = (int)r;
    return PDOG_OK;
}
} // namespace

int pdog_time_axis(double start, double stop, double fps, double *out_ts, int cap, int *out_n)
{
#pragma clang fp contract(off)
    if (!out_n) return fail(PDOG_E_ARG, "pdog_time_axis: out_n is null");
    int n = 0;
    if (int rc = time_axis_len("pdog_time_axis", start, stop, fps, &n)) return rc;
    if (out_ts) {
        if (cap < n) return fail(PDOG_E_ARG, "pdog_time_axis: out_ts has room for " + std::to_string(cap) + " of " + std::to_string(n) + " values");
        out_ts[0] = start; // range(start, stop, 1) is [start]
        if (n > 1) {
            const double step = (stop - start) / (double)(n - 1);
            for (int j = 0; j < n; ++j) out_ts[j] = start + (double)j * step;
        }
    }
    *out_n = n;
    return PDOG_OK;
}

int pdog_fps_table(double rate, int n_frames, double start, double stop, double fps, int32_t *out_index, int cap, int *out_n)
{
#pragma clang fp contract(off)
    if (!out_n) return fail(PDOG_E_ARG, "pdog_fps_table: out_n is null");
    if (!(rate > 0.0) || n_frames <= 0 || !(start >= 0.0)) return fail(PDOG_E_ARG, "pdog_fps_table: rate <= 0, no frames or start < 0");
    int n = 0;
    if (int rc = time_axis_len("pdog_fps_table", start, stop, fps, &n)) return rc;
    const double first = std::ceil(start * rate); // the first frame at or after `start`
    if (!(first < (double)n_frames)) return fail(PDOG_E_ARG, "pdog_fps_table: the stack holds no frame at or after start");
    const int i0 = (int)first, last = n_frames - 1 - i0;
    auto o = [&](int i) { return std::floor(((double)i * fps) / rate + 0.5); }; // output slot of input frame i (round = near)
    const double m = std::min((double)n, o(last) + 1.0);
    const int count = (int)m;
    if (out_index) {
        if (cap < count) return fail(PDOG_E_ARG, "pdog_fps_table: out_index has room for " + std::to_string(cap) + " of " + std::to_string(count) + " entries");
        int i = 0; // max{ i : o(i) <= j } is monotone in j (o(0) = 0, so it exists for every j)
        for (int j = 0; j < count; ++j) {
            while (i < last && o(i + 1) <= (double)j) ++i;
            out_index[j] = i0 + i;
        }
    }
    *out_n = count;
    return PDOG_OK;
}

// ---- the exclusive step on the host (include/pawsome_exclusive.h): the rule round by round, as the header states it ----
int pdog_assign_exclusive_host(int n_groups, int n_targets, int k, int min_distance, double min_ratio, const int32_t *prev,
                               const int32_t *ij, const float *peak, const int32_t *count, int32_t *out_ij, int32_t *out_state)
{
    using namespace pdog::exclusive;
    if (!prev || !ij || !peak || !count || !out_ij || !out_state) return fail(PDOG_E_ARG, "pdog_assign_exclusive_host: null pointer");
    if (int rc = check_exclusive("pdog_assign_exclusive_host", n_groups, n_targets, k, min_ratio)) return rc;
    if (min_distance < 1) return fail(PDOG_E_ARG, "pdog_assign_exclusive_host: min_distance must be given (>= 1)");
    const int T = n_targets;
    const long long d = min_distance;
    const float rho = (float)min_ratio;
    for (int g = 0; g < n_groups; ++g) {
        const size_t w0 = (size_t)g * T;
        bool assigned[kMaxTargets] = {};
        int32_t *oij = out_ij + 2 * w0, *ost = out_state + w0;
        for (int t = 0; t < T; ++t) { // held until a round says otherwise
            oij[2 * t] = prev[2 * (w0 + t)];
            oij[2 * t + 1] = prev[2 * (w0 + t) + 1];
            ost[t] = -1;
        }
        for (int round = 0; round < T; ++round) {
            uint64_t best = 0;
            int best_q = 0;
            for (int t = 0; t < T; ++t) {
                if (assigned[t]) continue;
                const int32_t *pij = ij + 2 * (w0 + t) * k;
                const float *pk = peak + (w0 + t) * k;
                for (int q = 0; q < k; ++q) { // the head: the first entry that is admissible and not blocked
                    if (!admissible(q, count[w0 + t], pk[q], pk[0], rho)) continue;
                    bool blocked = false;
                    for (int u = 0; u < T && !blocked; ++u)
                        blocked = assigned[u] && blocks(pij[2 * q], pij[2 * q + 1], oij[2 * u], oij[2 * u + 1], d);
                    if (blocked) continue;
                    const uint64_t key = head_key(pk[q], t);
                    if (key > best) { best = key; best_q = q; }
                    break;
                }
            }
            if (!best) break;
            const int t = key_target(best);
            const int32_t *pij = ij + 2 * (w0 + t) * k;
            assigned[t] = true;
            oij[2 * t] = pij[2 * best_q];
            oij[2 * t + 1] = pij[2 * best_q + 1];
            ost[t] = best_q + 1;
        }
    }
    return PDOG_OK;
}

// ---- the motion step on the host (include/pawsome_motion.h): the rule round by round, as the header states it ----
int pdog_assign_motion_host(int n_groups, int n_targets, int k, int min_distance, double min_ratio, double min_response, int coast,
                            int frame_h, int frame_w, const int32_t *prev, int32_t *mstate, const int32_t *ij, const float *peak,
                            const int32_t *count, int32_t *out_ij, int32_t *out_state, int32_t *next)
{
    using namespace pdog::motion;
    const char *who = "pdog_assign_motion_host";
    if (!prev || !mstate || !ij || !peak || !count || !out_ij || !out_state || !next) return fail(PDOG_E_ARG, std::string(who) + ": null pointer");
    if (int rc = check_exclusive(who, n_groups, n_targets, k, min_ratio)) return rc;
    if (int rc = check_motion(who, min_response, coast)) return rc;
    if (min_distance < 1) return fail(PDOG_E_ARG, std::string(who) + ": min_distance must be given (>= 1)");
    if (frame_h < 1 || frame_w < 1) return fail(PDOG_E_ARG, std::string(who) + ": the frame size must be given (>= 1 x 1)");
    const int T = n_targets;
    const long long d = min_distance;
    const float rho = (float)min_ratio, m = (float)min_response;
    for (int g = 0; g < n_groups; ++g) {
        const size_t w0 = (size_t)g * T;
        int ci[kMaxTargets] = {}, cj[kMaxTargets] = {}, ai[kMaxTargets] = {}, aj[kMaxTargets] = {}, st[kMaxTargets] = {};
        for (int t = 0; t < T; ++t) { // 1: the predictions; held until a round says otherwise
            ci[t] = predict(prev[2 * (w0 + t)], mstate[4 * (w0 + t)], frame_h);
            cj[t] = predict(prev[2 * (w0 + t) + 1], mstate[4 * (w0 + t) + 1], frame_w);
            st[t] = -1;
        }
        for (int round = 0; round < T; ++round) {
            bool any = false;
            uint32_t best_d = 0;
            uint64_t best_key = 0;
            int best_q = 0;
            for (int t = 0; t < T; ++t) {
                if (st[t] != -1) continue;
                const int32_t *pij = ij + 2 * (w0 + t) * k;
                const float *pk = peak + (w0 + t) * k;
                bool has = false; // 4: the head, the free entry nearest to the prediction
                uint32_t hd = 0;
                int hq = 0;
                for (int q = 0; q < k; ++q) {
                    if (!admissible(q, count[w0 + t], pk[q], pk[0], m, rho)) continue;
                    bool blocked = false;
                    for (int u = 0; u < T && !blocked; ++u)
                        blocked = st[u] != -1 && blocks(pij[2 * q], pij[2 * q + 1], ai[u], aj[u], d);
                    if (blocked) continue;
                    const uint32_t D = dist2(pij[2 * q], pij[2 * q + 1], ci[t], cj[t]);
                    if (!has || D < hd) { has = true; hd = D; hq = q; }
                }
                if (!has) continue;
                const uint64_t key = head_key(pk[hq], t); // 5: the smallest D, then the larger value, then the smaller t
                if (!any || hd < best_d || (hd == best_d && key > best_key)) { any = true; best_d = hd; best_key = key; best_q = hq; }
            }
            if (!any) break;
            const int t = key_target(best_key);
            const int32_t *pij = ij + 2 * (w0 + t) * k;
            ai[t] = pij[2 * best_q];
            aj[t] = pij[2 * best_q + 1];
            st[t] = best_q + 1;
        }
        for (int t = 0; t < T; ++t) { // 6 - 8
            const size_t w = w0 + t;
            Carry c = {mstate[4 * w], mstate[4 * w + 1], mstate[4 * w + 2]};
            int oi = ci[t], oj = cj[t];
            if (st[t] == -1) c = carry_held(c, coast);
            else {
                bool contested = false;
                for (int u = 0; u < T; ++u) contested |= u != t && blocks(ai[t], aj[t], ci[u], cj[u], d);
                c = carry_assigned(c, contested, prev[2 * w], prev[2 * w + 1], ai[t], aj[t]);
                oi = ai[t];
                oj = aj[t];
            }
            out_ij[2 * w] = oi;
            out_ij[2 * w + 1] = oj;
            out_state[w] = st[t];
            next[2 * w] = predict(oi, c.vi, frame_h);
            next[2 * w + 1] = predict(oj, c.vj, frame_w);
            mstate[4 * w] = c.vi; mstate[4 * w + 1] = c.vj; mstate[4 * w + 2] = c.n_held; mstate[4 * w + 3] = 0;
        }
    }
    return PDOG_OK;
}

// ---- the shape rule's Float64 part on the host (include/pawsome_shape.h, steps 7 and 8; pdog_shape.hpp holds the arithmetic) ----
int pdog_shape_derive(const int32_t sums[8], const int32_t ij[2], double out[6])
{
    if (!sums || !ij || !out) return fail(PDOG_E_ARG, "pdog_shape_derive: null pointer");
    pdog::shape::derive(sums, ij[0], ij[1], out);
    return PDOG_OK;
}

int pdog_shape_headings(const double *theta, const int32_t *ij, int n_steps, double min_step, double *out)
{
    if (n_steps < 0 || !(min_step >= 0)) return fail(PDOG_E_ARG, "pdog_shape_headings: n_steps < 0, or a min_step that is negative or NaN");
    if (n_steps == 0) return PDOG_OK;
    if (!theta || !ij || !out) return fail(PDOG_E_ARG, "pdog_shape_headings: null pointer");
    pdog::shape::headings(theta, ij, n_steps, min_step, out);
    return PDOG_OK;
}

// ---- the frame-blob rule's Float64 part on the host (include/pawsome_frame_blobs.h, "Derived"; pdog_frame_blobs.hpp holds the arithmetic) ----
int pdog_frame_blobs_derive(const int64_t words[12], double out[6])
{
    if (!words || !out) return fail(PDOG_E_ARG, "pdog_frame_blobs_derive: null pointer");
    pdog::fblobs::derive(words, out);
    return PDOG_OK;
}

} // extern "C"
