// dog_assign.hpp — the exclusive step (include/pawsome_exclusive.h states the rule; tests/exclusive_restatement.py restates it
// in NumPy and this kernel is held to that bit for bit): the targets of one group share out the peaks that pdog_detect_peaks
// found in their windows, and the same kernel does the bookkeeping dog_step.hpp does for plain walks.
//
// THE KERNEL.  One wave per group, lane t serves target t (T <= 32: the upper half of the wave idles).  No LDS, no workgroup
// barrier, no scratch; plain vector stores only.
//   State    A lane keeps its list position q, whether the entry there is VERIFIED (admissible and free of every position
//            taken so far: its head), and — once it has won a round — its assigned position.  The set of lanes that have
//            won is one wave-uniform 32-bit mask; a taken position is read out of its lane with v_readlane.
//   Settle   Lanes whose entry is not verified look at it: inadmissible or blocked by a taken position, they move on to the
//            next entry (past the count the list is exhausted at once).  q only grows — admissibility does not change during a step and the taken set only grows —, so the
//            loop ends after at most k passes per step in all, and a step in which nobody is blocked passes through it once.
//   Round    The maximum over the lanes of pdog::exclusive::head_key (the orderable FP32 value, then the inverted t), a DPP
//            reduction of the 64-bit key; 0 = no lane has a head = the step is over.  The winner's position is broadcast
//            with v_readlane; a verified lane only has to test its head against THAT position, and settles again if it lost it.
//   Filing   out[g][t][step], state[g][t][step], the next guesses.  A group whose table row has ended (len[g] <= step)
//            stores nothing and keeps its guesses.
// Bounds: lane t < T reads entries q < k of window g*T + t and its count, prev and nothing else; it writes one pair and one
// state at (g*T + t) * out_stride + step and its own next guess.  Positions enter comparisons only, widened to 64 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "pdog_exclusive.hpp"
#include "dog_wave.hpp"

namespace pdog {
namespace exclusive {

struct AssignGeo {
    const int32_t *prev;   // [G][T][2] the positions the windows were centred on (may be `next`: a lane reads its own first)
    const int32_t *ij;     // [G][T][k][2] pdog_detect_peaks' picks
    const float *peak;     // [G][T][k]
    const int32_t *count;  // [G][T]
    int32_t *out_ij;       // target (g, t)'s pair of this step at 2 * ((g*T + t) * out_stride + step)
    int32_t *out_state;    // … its state at (g*T + t) * out_stride + step
    int32_t *next;         // [G][T][2] the next step's guesses, or null
    const int32_t *len;    // [G] steps of each group, or null: every group takes part
    long long out_stride;  // steps per target in out_ij / out_state
    long long d;           // min_distance
    int step, T, k;
    float rho;             // (float)min_ratio
};

static __global__ __launch_bounds__(64) void dog_assign_kernel(const AssignGeo a)
{
    const int g = blockIdx.x, lane = threadIdx.x;
    if (a.len && a.len[g] <= a.step) return; // (uniform) the group's row has ended
    const bool mine = lane < a.T;
    const long long w = (long long)g * a.T + (mine ? lane : 0); // the lane's window
    const int32_t *ij = a.ij + w * a.k * 2;
    const float *pk = a.peak + w * a.k;
    int cnt = 0, pi = 0, pj = 0;
    float v0 = 0.f;
    if (mine) { cnt = a.count[w]; v0 = pk[0]; pi = a.prev[2 * w]; pj = a.prev[2 * w + 1]; }

    bool live = mine, verified = false; // live: not assigned yet
    int q = 0, ci = 0, cj = 0;          // the entry looked at, its position …
    float cv = 0.f;                     // … and value
    int ai = 0, aj = 0, state = -1;     // the assigned position
    unsigned taken = 0;                 // (uniform) the lanes that have won a round
    for (int round = 0; round < a.T; ++round) {
        for (;;) { // settle
            if (q > 0 && q >= cnt) q = a.k; // no entry at or beyond the count is admissible: the list is exhausted
            const bool look = live && !verified && q < a.k;
            bool adm = false;
            if (look) {
                cv = pk[q]; ci = ij[2 * q]; cj = ij[2 * q + 1];
                adm = admissible(q, cnt, cv, v0, a.rho);
            }
            bool blocked = false;
            if (__ballot(adm))
                for (unsigned m = taken; m; m &= m - 1) {
                    const int u = __builtin_amdgcn_readfirstlane(__builtin_ctz(m));
                    blocked |= blocks(ci, cj, __builtin_amdgcn_readlane(ai, u), __builtin_amdgcn_readlane(aj, u), a.d);
                }
            if (look) {
                if (adm && !blocked) verified = true;
                else ++q;
            }
            if (!__ballot(live && !verified && q < a.k)) break;
        }
        const bool head = live && verified;
        const unsigned long long best = wave_max_u64(head ? head_key(cv, lane) : 0ull);
        if (!best) break; // no unassigned target has a head
        const int win = key_target(best);
        const int wi = __builtin_amdgcn_readlane(ci, win), wj = __builtin_amdgcn_readlane(cj, win);
        taken |= 1u << win;
        if (lane == win) { live = false; ai = ci; aj = cj; state = q + 1; }
        else if (head && blocks(ci, cj, wi, wj, a.d)) { verified = false; ++q; }
    }
    if (!mine) return;
    const int oi = live ? pi : ai, oj = live ? pj : aj; // held: the position stays
    const long long o = w * a.out_stride + a.step;
    a.out_ij[2 * o] = oi;
    a.out_ij[2 * o + 1] = oj;
    a.out_state[o] = live ? -1 : state;
    if (a.next) { a.next[2 * w] = oi; a.next[2 * w + 1] = oj; }
}

// Before the first step of a walk: the starts become the guesses, and with first = 1 a group that has a step files them as
// given, with state 0.
static __global__ void dog_assign_init_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ len, int32_t *__restrict__ cur,
                                              int32_t *__restrict__ out_ij, int32_t *__restrict__ out_state, int n, int T, long long n_steps, int first)
{
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n) return;
    const int i = start[2 * p], j = start[2 * p + 1];
    cur[2 * p] = i;
    cur[2 * p + 1] = j;
    if (first && len[p / T] >= 1) {
        out_ij[2 * p * n_steps] = i;
        out_ij[2 * p * n_steps + 1] = j;
        out_state[p * n_steps] = 0;
    }
}

} // namespace exclusive
} // namespace pdog
