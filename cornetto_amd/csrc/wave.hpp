// wave.hpp — the add primitives over one wave (64 lanes) that every scan and every ordered scatter of the library is built from.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace cnwave {

// inclusive add-scan over the wave: lane i gets v[0] + ... + v[i]
template <typename T>
__device__ __forceinline__ T wave_incl(T v, int lane)
{
    static_assert(std::is_same<T, uint32_t>::value || std::is_same<T, unsigned long long>::value, "32- and 64-bit counters only");
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// the same scan in six DPP additions (row shifts, then the two row broadcasts)
__device__ __forceinline__ uint32_t wave_incl_dpp(uint32_t v)
{
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);      // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);      // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);      // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);      // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    return (uint32_t)x;
}

// sum over the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

}  // namespace cnwave
