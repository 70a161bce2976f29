/*
 * oslam_verify.hip -- the verification stage's kernels (semantics: include/oslam.h at oslam_verify; host side:
 * oslam_verify.c).
 *
 *   k_view_z   one thread per pixel: raw depth (uint16 or float) -> float z, exactly depth_at of oslam_depth.hip, with
 *              0 where the pixel is not valid (every valid z is >= z_min > 0).  The z image of a 640x480 frame is
 *              1.2 MB: it stays in L2 / the Infinity Cache for k_verify.
 *   k_verify   one thread per model point, every member of the call in one grid (y = member, x = block of 256 model
 *              points): transform, class, then per class a wave ballot + popcount, the four waves summed in LDS and
 *              one integer atomicAdd per class and workgroup into the member's counters.  Integer sums do not depend
 *              on their order: the counts are deterministic.  The tap variant writes each point's class instead.
 *              The class itself is oslam_verify_class (oslam_verify_class.h), shared with the arbitration stage.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"
#include "oslam_verify_class.h"

__global__ __launch_bounds__(256) void k_view_z(const void *raw, int is_u16, int w, int h, float scale, float z_min,
                                                float z_max, float *z_out)
{
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), v = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (u >= w || v >= h) return;
    const size_t i = (size_t)v * w + u;
    const float z = is_u16 ? (float)reinterpret_cast<const uint16_t *>(raw)[i] * scale
                           : reinterpret_cast<const float *>(raw)[i] * scale;
    z_out[i] = (z >= z_min && z <= z_max) ? z : 0.0f;
}

template <bool TAP>
__global__ __launch_bounds__(OSLAMK_VERIFY_THREADS) void k_verify(const oslamk_view v, const oslamk_verify_member *mem,
                                                                  int window, uint32_t *counts, uint8_t *class_out)
{
    __shared__ uint32_t sh[OSLAMK_VERIFY_THREADS / 64][OSLAMK_VERIFY_CLASSES];
    const uint32_t j = blockIdx.y;
    const oslamk_verify_member *d = &mem[j];
    if (blockIdx.x >= d->n_blocks) return;     /* the whole workgroup leaves together */
    const int i = (int)(blockIdx.x * OSLAMK_VERIFY_THREADS + threadIdx.x);

    const int cls = i < d->m.n ? oslam_verify_class<false>(v, d, i, window, NULL, NULL, NULL) : -1;
    if (TAP) {
        if (cls >= 0) class_out[i] = (uint8_t)cls;
        return;
    }

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < OSLAMK_VERIFY_CLASSES; c++) {
        const unsigned long long b = __ballot(cls == c);
        if (lane == 0) sh[w][c] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (threadIdx.x < OSLAMK_VERIFY_CLASSES) {
        uint32_t s = 0;
#pragma unroll
        for (int ww = 0; ww < OSLAMK_VERIFY_THREADS / 64; ww++) s += sh[ww][threadIdx.x];
        if (s) atomicAdd(&counts[(size_t)j * OSLAMK_VERIFY_CLASSES + threadIdx.x], s);
    }
}

extern "C" int oslamk_view_z(const void *d_raw, int is_u16, int w, int h, float scale, float z_min, float z_max, float *d_z,
                             void *stream)
{
    if (w <= 0 || h <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_view_z, dim3((w + 31) / 32, (h + 7) / 8), dim3(256), 0, (hipStream_t)stream, d_raw, is_u16, w, h,
                       scale, z_min, z_max, d_z);
    return (int)hipGetLastError();
}

extern "C" int oslamk_verify(const oslamk_view *v, const oslamk_verify_member *d_mem, uint32_t n_mem, uint32_t max_blocks,
                             int window, uint32_t *counts, uint8_t *class_out, void *stream)
{
    if (n_mem == 0 || max_blocks == 0) return 0;
    if (n_mem > 65535u || window < 0 || window > 3) return (int)hipErrorInvalidValue;
    const dim3 grid(max_blocks, n_mem);
    if (class_out)
        hipLaunchKernelGGL(k_verify<true>, grid, dim3(OSLAMK_VERIFY_THREADS), 0, (hipStream_t)stream, *v, d_mem, window,
                           counts, class_out);
    else
        hipLaunchKernelGGL(k_verify<false>, grid, dim3(OSLAMK_VERIFY_THREADS), 0, (hipStream_t)stream, *v, d_mem, window,
                           counts, class_out);
    return (int)hipGetLastError();
}
