// dog_motion.hpp — the motion step (include/pawsome_motion.h states the rule; tests/motion_restatement.py restates it in NumPy
// and this kernel is held to that bit for bit): the targets of one group share out the peaks that pdog_detect_peaks found in
// windows centred on their PREDICTIONS, each taking the free peak nearest to its prediction, and the same kernel carries
// velocity and hold count to the next step and files the walk.
//
// THE KERNEL.  One wave per group, lane t serves target t (T <= 32: the upper half of the wave idles).  No workgroup barrier,
// no scratch; plain vector stores only.
//   Lists    A lane's head is a MINIMUM over its whole list (the entry nearest to the prediction), so a lane keeps a 32-bit
//            mask of the entries still ALIVE — admissible and blocked by no position taken so far — beside its head (entry,
//            position, value, D).  Admissibility does not change during a step and the taken set only grows: bits only go.
//            kLds = false reads an entry from global memory whenever it is looked at; kLds = true stages the lists in LDS in
//            the first pass (entry q of lane t at word q * 32 + t of three arrays, 12 KiB: no bank conflict) — a lane only
//            ever reads what it wrote itself, so the wave needs no barrier.
//   Round    The wave-wide minimum of the heads' D (DPP reduction), then the 64-bit head_key maximum of dog_assign.hpp over the
//            lanes that hold that minimum; no lane with a head = the step is over.  The winner's position is broadcast with
//            v_readlane.  A lane whose alive entries ALL lie farther than d from it along an axis (a bounding box kept since
//            the first pass) loses nothing and does nothing; the others walk their alive bits once, clear what the position
//            blocks and take the minimum of D over what is left.
//   Contest  An assigned lane tests its position against every other lane's prediction, read with v_readlane.
//   Filing   out[g][t][step], state[g][t][step], the new positions, the next guesses (the next predictions) and mstate.  A
//            group whose table row has ended (len[g] <= step) stores nothing.
// Bounds: lane t < T reads entries q < k of window g*T + t, its count, prev and mstate and nothing else; it writes one pair
// and one state at (g*T + t) * out_stride + step, its own position, next guess and mstate.  LDS words q * 32 + t < 1024.
// Positions enter comparisons widened to 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dog_wave.hpp" // wave_max_u64
#include "pdog_motion.hpp"

namespace pdog {
namespace motion {

using exclusive::wave_max_u64;

struct MotionGeo {
    const int32_t *prev;   // [G][T][2] the positions p of the last step (may be `pos`: a lane reads its own first)
    int32_t *mstate;       // [G][T][4] in: (v_row, v_col, n_held, -); out: the same after the step, word 3 = 0
    const int32_t *ij;     // [G][T][k][2] pdog_detect_peaks' picks at the predictions
    const float *peak;     // [G][T][k]
    const int32_t *count;  // [G][T]
    int32_t *out_ij;       // target (g, t)'s pair of this step at 2 * ((g*T + t) * out_stride + step)
    int32_t *out_state;    // … its state at (g*T + t) * out_stride + step
    int32_t *pos;          // [G][T][2] the new positions, or null
    int32_t *next;         // [G][T][2] the next step's guesses
    const int32_t *len;    // [G] steps of each group, or null: every group takes part
    long long out_stride;  // steps per target in out_ij / out_state
    long long d;           // min_distance
    int step, T, k, h, w, coast;
    float rho, m;          // (float)min_ratio, (float)min_response
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_min_u32(unsigned v)
{
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xF, false);
    return o < v ? o : v;
}
// The DPP steps of dog_wave.hpp's wave_max_u64 for an unsigned minimum.
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    v = dpp_min_u32<0xB1, 0xF>(v);
    v = dpp_min_u32<0x4E, 0xF>(v);
    v = dpp_min_u32<0x141, 0xF>(v);
    v = dpp_min_u32<0x140, 0xF>(v);
    v = dpp_min_u32<0x142, 0xA>(v);
    v = dpp_min_u32<0x143, 0xC>(v);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

constexpr int kLdsWords = kMaxTargets * 32; // per array: 32 lanes x PDOG_PEAKS_MAX_K entries

template <bool kLds>
static __global__ __launch_bounds__(64) void dog_motion_kernel(const MotionGeo a)
{
    __shared__ int32_t s_i[kLds ? kLdsWords : 1], s_j[kLds ? kLdsWords : 1];
    __shared__ float s_v[kLds ? kLdsWords : 1];
    const int g = blockIdx.x, lane = threadIdx.x;
    if (a.len && a.len[g] <= a.step) return; // (uniform) the group's row has ended
    const bool mine = lane < a.T;
    const long long w = (long long)g * a.T + (mine ? lane : 0); // the lane's window
    const int32_t *ij = a.ij + w * a.k * 2;
    const float *pk = a.peak + w * a.k;
    const int sl = lane & 31; // (lanes >= T never touch LDS)
    int cnt = 0, pi = 0, pj = 0;
    float v0 = 0.f;
    Carry c = {0, 0, 0};
    if (mine) {
        cnt = a.count[w]; v0 = pk[0]; pi = a.prev[2 * w]; pj = a.prev[2 * w + 1];
        c.vi = a.mstate[4 * w]; c.vj = a.mstate[4 * w + 1]; c.n_held = a.mstate[4 * w + 2];
    }
    const int ci = predict(pi, c.vi, a.h), cj = predict(pj, c.vj, a.w); // the prediction the window was centred on

    // the first pass: which entries are admissible, the head among them, their bounding box
    unsigned alive = 0;
    unsigned hD = kFar;
    int hq = 0, hi = 0, hj = 0;
    float hv = 0.f;
    int lo_i = 0x7fffffff, hi_i = -0x7fffffff - 1, lo_j = 0x7fffffff, hi_j = -0x7fffffff - 1;
    if (mine)
        for (int q = 0; q < a.k; ++q) {
            const float v = pk[q];
            const int i = ij[2 * q], j = ij[2 * q + 1];
            if (kLds) { s_i[q * 32 + sl] = i; s_j[q * 32 + sl] = j; s_v[q * 32 + sl] = v; }
            if (!admissible(q, cnt, v, v0, a.m, a.rho)) continue;
            const unsigned D = dist2(i, j, ci, cj);
            if (!alive || D < hD) { hD = D; hq = q; hi = i; hj = j; hv = v; } // ties: the smaller q stays
            alive |= 1u << q;
            lo_i = min(lo_i, i); hi_i = max(hi_i, i); lo_j = min(lo_j, j); hi_j = max(hi_j, j);
        }

    bool live = mine;               // not assigned yet
    int ai = 0, aj = 0, state = -1; // the assigned position
    for (int round = 0; round < a.T; ++round) {
        const bool head = live && alive != 0;
        if (!__ballot(head)) break; // no unassigned target has a head
        const unsigned dmin = wave_min_u32(head ? hD : kFar);
        const unsigned long long best = wave_max_u64(head && hD == dmin ? head_key(hv, lane) : 0ull);
        const int win = key_target(best);
        const int wi = __builtin_amdgcn_readlane(hi, win), wj = __builtin_amdgcn_readlane(hj, win);
        if (lane == win) { live = false; ai = hi; aj = hj; state = hq + 1; }
        else if (head && (long long)wi > lo_i - a.d && (long long)wi < hi_i + a.d && (long long)wj > lo_j - a.d && (long long)wj < hi_j + a.d) {
            // (wi, wj) may block some of the lane's entries: clear them, and the minimum of D over what is left
            unsigned left = 0;
            hD = kFar;
            for (unsigned m = alive; m; m &= m - 1) {
                const int q = __builtin_ctz(m);
                const int i = kLds ? s_i[q * 32 + sl] : ij[2 * q], j = kLds ? s_j[q * 32 + sl] : ij[2 * q + 1];
                if (blocks(i, j, wi, wj, a.d)) continue;
                const unsigned D = dist2(i, j, ci, cj);
                if (!left || D < hD) { hD = D; hq = q; hi = i; hj = j; }
                left |= 1u << q;
            }
            alive = left;
            if (alive) hv = kLds ? s_v[hq * 32 + sl] : pk[hq];
        }
    }

    // contested: the assigned position lies within d of ANOTHER target's prediction, whatever became of that target
    bool contested = false;
    for (int u = 0; u < a.T; ++u) {
        const int uu = __builtin_amdgcn_readfirstlane(u);
        const int ui = __builtin_amdgcn_readlane(ci, uu), uj = __builtin_amdgcn_readlane(cj, uu);
        contested |= uu != lane && blocks(ai, aj, ui, uj, a.d);
    }
    if (!mine) return;
    int oi, oj;
    if (live) { oi = ci; oj = cj; c = carry_held(c, a.coast); } // held: it coasts along the prediction
    else { oi = ai; oj = aj; c = carry_assigned(c, contested, pi, pj, ai, aj); }
    const long long o = w * a.out_stride + a.step;
    a.out_ij[2 * o] = oi;
    a.out_ij[2 * o + 1] = oj;
    a.out_state[o] = live ? -1 : state;
    if (a.pos) { a.pos[2 * w] = oi; a.pos[2 * w + 1] = oj; }
    a.next[2 * w] = predict(oi, c.vi, a.h);
    a.next[2 * w + 1] = predict(oj, c.vj, a.w);
    a.mstate[4 * w] = c.vi;
    a.mstate[4 * w + 1] = c.vj;
    a.mstate[4 * w + 2] = c.n_held;
    a.mstate[4 * w + 3] = 0;
}

// Before the first step of a walk: the starts become the positions, clamp(start + v) the first guesses — v from the caller's
// mstate, or a walk at rest, which also clears the walk's own mstate —, and with first = 1 a group that has a step files its
// starts as given, with state 0.
static __global__ void dog_motion_init_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ len, int32_t *__restrict__ pos,
                                              int32_t *__restrict__ guess, int32_t *__restrict__ mstate, int at_rest,
                                              int32_t *__restrict__ out_ij, int32_t *__restrict__ out_state, int n, int T, long long n_steps,
                                              int first, int h, int w)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n) return;
    const int i = start[2 * p], j = start[2 * p + 1];
    if (at_rest) mstate[4 * p] = mstate[4 * p + 1] = mstate[4 * p + 2] = mstate[4 * p + 3] = 0;
    pos[2 * p] = i;
    pos[2 * p + 1] = j;
    guess[2 * p] = predict(i, mstate[4 * p], h);
    guess[2 * p + 1] = predict(j, mstate[4 * p + 1], w);
    if (first && len[p / T] >= 1) {
        out_ij[2 * p * n_steps] = i;
        out_ij[2 * p * n_steps + 1] = j;
        out_state[p * n_steps] = 0;
    }
}

} // namespace motion
} // namespace pdog
