// dog_wave.hpp — the wave-wide maximum of a 64-bit key, which the exclusive step's kernel (dog_assign.hpp) and the motion step's
// (dog_motion.hpp) both end a round with.  Device code only; no kernel lives here, so any unit may include it.
#pragma once
#include <hip/hip_runtime.h>

namespace pdog {
namespace exclusive {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long v)
{
    const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
    const unsigned olo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
    const unsigned ohi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    return o > v ? o : v;
}
// The DPP steps of dog_peaks.hpp's wave_reduce on both halves of a 64-bit key: lane 63 ends up with the wave's maximum,
// handed back uniform.
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
    v = dpp_max_u64<0xB1, 0xF>(v);  // quad: xor 1
    v = dpp_max_u64<0x4E, 0xF>(v);  // quad: xor 2
    v = dpp_max_u64<0x141, 0xF>(v); // mirror within 8
    v = dpp_max_u64<0x140, 0xF>(v); // mirror within 16
    v = dpp_max_u64<0x142, 0xA>(v); // row broadcast 15
    v = dpp_max_u64<0x143, 0xC>(v); // row broadcast 31
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

} // namespace exclusive
} // namespace pdog
