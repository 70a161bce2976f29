/*
 * oslam_lane.h -- what the lanes of one wave (64 on gfx950) hand to each other in the registration kernels: sums and
 * the maximum over the wave, the value of a named lane, and a value that every lane holds moved to scalar registers.
 * Device code only.  Included by oslam_vote_body.inc (the vote units), oslam_scene.hip, oslam_posegpu.hip and
 * oslam_sort.hip.
 */
#ifndef OSLAM_LANE_H
#define OSLAM_LANE_H

#include <stdint.h>

#define WAVE 64

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t w = __shfl_xor(v, o, WAVE);
        v = v > w ? v : w;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

__device__ __forceinline__ float readlane_f(float v, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ uint32_t readlane_u(uint32_t v, int l)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
/* a value every lane holds, moved to scalar registers */
__device__ __forceinline__ uint32_t uni_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ unsigned long long uni_u64(unsigned long long v)
{
    return ((unsigned long long)uni_u32((uint32_t)(v >> 32)) << 32) | uni_u32((uint32_t)v);
}

#endif
