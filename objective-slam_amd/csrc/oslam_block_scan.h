/*
 * oslam_block_scan.h -- sums and exclusive scans of one uint32 per thread over a workgroup of WAVES whole waves, for the
 * grid, surface and mesh kernels.  Device code only.  Contract of the block_* functions:
 *   - row is WAVES words of LDS owned by the caller;
 *   - a call holds exactly one __syncthreads(), between its store to the row and its loads from it, so every thread of
 *     the workgroup makes the call;
 *   - the caller must not let any thread store to the same row again before every thread has loaded from it: a fresh
 *     row per call (s_cnt[it] of the extraction kernels) or a barrier of the caller's own (k_surface_scan's second).
 */
#ifndef OSLAM_BLOCK_SCAN_H
#define OSLAM_BLOCK_SCAN_H

#include <stdint.h>

/* inclusive sum over the lanes of the wave */
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= (uint32_t)off) x += y;
    }
    return x;
}

/* sum over the lanes of the wave, valid in lane 0 */
__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}

/* each wave's writer lane gives wave_total: the sum over the lower waves, *all = over all of them */
template <int WAVES>
__device__ __forceinline__ uint32_t block_before(uint32_t wave_total, bool writer, uint32_t *row, uint32_t *all)
{
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t before = 0, tot = 0;
    if (writer) row[wave] = wave_total;
    __syncthreads();
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)WAVES; w++) {
        const uint32_t c = row[w];
        if (w < wave) before += c;
        tot += c;
    }
    *all = tot;
    return before;
}

/* the sum of v over the lower threads of the workgroup, *all = over all of them */
template <int WAVES> __device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *row, uint32_t *all)
{
    const uint32_t incl = wave_incl_scan(v);
    return block_before<WAVES>(incl, (threadIdx.x & 63u) == 63u, row, all) + incl - v;
}

/* the sum of v over the workgroup, valid in thread 0 */
template <int WAVES> __device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *row)
{
    uint32_t s = 0;
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0u) row[threadIdx.x >> 6] = v;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES; w++) s += row[w];
    return s;
}

#endif /* OSLAM_BLOCK_SCAN_H */
