/*
 * oslam_pyramid.hip -- the image pyramid's kernel (semantics: include/oslam.h at oslam_pyramid_create; host side:
 * oslam_pyramid.c).
 *
 *   k_pyr_down   one launch per level: the z image of level k (w x h) -> the z image of level k + 1
 *                ((w + 1) / 2 x (h + 1) / 2).  One thread per output pixel in 32 x 8 tiles (k_tsdf_raycast's tiling).
 *                The thread loads the centre z[2v][2u]; an invalid centre writes 0.  Otherwise it walks the 5 x 5
 *                window row by row and adds the pixels within depth_band of the centre in float in that order, counts
 *                them, divides and clamps to [z_min, z_max].  The 25 values are loaded straight from the image: the
 *                whole 640 x 480 frame is 1.2 MB, every value is read by at most 9 threads that sit in neighbouring
 *                lanes or rows of one workgroup, and the call is bound by its launch, not by its loads.  No LDS, no
 *                scratch, no atomics.  The translation unit is built with -ffp-contract=off: the sum has no fused
 *                multiply-add, and the division is the correctly rounded one.
 * Bounds: the output pixel is checked against (w', h') before anything is read; the centre (2u, 2v) then lies inside
 * the source (2 * (w' - 1) <= w - 1); every other source index is range-checked before its load.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"

__global__ __launch_bounds__(256) void k_pyr_down(const oslamk_view sv, int wo, int ho, float depth_band, float *z_out)
{
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), v = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (u >= wo || v >= ho) return;
    const int su = 2 * u, sy = 2 * v;
    const float c = sv.z[(size_t)sy * sv.w + su];
    float out = 0.0f;
    if (c != 0.0f) {
        float sum = 0.0f;
        int cnt = 0;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int y = sy + dy;
            if (y < 0 || y >= sv.h) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int x = su + dx;
                if (x < 0 || x >= sv.w) continue;
                const float z = sv.z[(size_t)y * sv.w + x];
                if (z > 0.0f && fabsf(z - c) <= depth_band) {
                    sum += z;
                    cnt++;
                }
            }
        }
        out = fminf(fmaxf(sum / (float)cnt, sv.z_min), sv.z_max);
    }
    z_out[(size_t)v * wo + u] = out;
}

extern "C" int oslamk_pyr_down(const oslamk_view *src, float depth_band, float *z_out, void *stream)
{
    if (!src || !src->z || !z_out || src->w <= 0 || src->h <= 0 || !(depth_band > 0.0f)) return (int)hipErrorInvalidValue;
    const int wo = (src->w + 1) / 2, ho = (src->h + 1) / 2;
    hipLaunchKernelGGL(k_pyr_down, dim3((wo + 31) / 32, (ho + 7) / 8), dim3(256), 0, (hipStream_t)stream, *src, wo, ho,
                       depth_band, z_out);
    return (int)hipGetLastError();
}
