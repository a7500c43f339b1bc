// pdog_exclusive.hpp — the pieces of the exclusive step's rule (include/pawsome_exclusive.h) that the kernel (dog_assign.hpp)
// and the host function (pdog_assign_exclusive_host, pdog_math.cpp) must agree on to the bit: which list entries are
// admissible, when one position blocks another, and the order in which heads win a round.  Plain C++, no HIP, no tracker: the
// host compiler takes it as it is (tests/exclusive_main.cpp), hipcc as host and device code.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PDOG_HD __host__ __device__
#else
#define PDOG_HD
#endif

namespace pdog {
namespace exclusive {

constexpr int kMaxTargets = 32; // PDOG_EXCLUSIVE_MAX_TARGETS: a group is one wave's lower half, its taken set one 32-bit mask

// Entry q of a list with `count` entries, value v, pick 1's value v0.  rho_f * v0 is ONE FP32 multiplication (nothing to
// contract it with); a NaN on either side fails the comparisons.
PDOG_HD inline bool admissible(int q, int count, float v, float v0, float rho_f)
{
    return q == 0 || (q < count && v > 0.0f && v >= rho_f * v0);
}

// di*di + dj*dj < d*d in integers, for any int32 positions and 1 <= d < 2^31: the squares are formed only where both
// differences are below d in magnitude (each square < 2^62).
PDOG_HD inline bool blocks(int i, int j, int oi, int oj, long long d)
{
    const long long di = (long long)i - oi, dj = (long long)j - oj;
    if (di >= d || di <= -d || dj >= d || dj <= -d) return false;
    return di * di + dj * dj < d * d;
}

// The round's order as one unsigned key: the value (larger wins; -0 ranks as +0, a NaN as -inf), then the target (smaller t
// wins).  No key of a head is 0, which stands for "no head".
PDOG_HD inline uint64_t head_key(float v, int t)
{
    if (!(v == v)) v = -__builtin_huge_valf();
    if (v == 0.0f) v = 0.0f; // -0 -> +0
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u; // FP32 order as unsigned order
    return ((uint64_t)u << 32) | (uint32_t)(63 - t);
}
PDOG_HD inline int key_target(uint64_t key) { return 63 - (int)(key & 63u); }

} // namespace exclusive
} // namespace pdog
