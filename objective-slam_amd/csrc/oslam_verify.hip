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
 * Bounds: a point reads at most (2 window + 1)^2 <= 49 floats of the z image, all inside it (the window is clipped);
 * the pixel is range-checked in float before it becomes an int.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"

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

    int cls = -1;
    if (i < d->m.n) {
        float T[12];
#pragma unroll
        for (int k = 0; k < 12; k++) T[k] = d->T[k];
        const float px = d->m.px[i], py = d->m.py[i], pz = d->m.pz[i];
        const float nx = d->m.nx[i], ny = d->m.ny[i], nz = d->m.nz[i];
        const float qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
        const float qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
        const float qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
        const float mx = (T[0] * nx + T[1] * ny) + T[2] * nz;
        const float my = (T[4] * nx + T[5] * ny) + T[6] * nz;
        const float mz = (T[8] * nx + T[9] * ny) + T[10] * nz;
        if ((mx * qx + my * qy) + mz * qz >= 0.0f) {
            cls = 0;                                               /* BACK */
        } else {
            bool in = qz >= v.z_min && qz <= v.z_max;
            float fu = 0.0f, fv = 0.0f;
            if (in) {
                fu = floorf(((qx * v.fx) / qz + v.cx) + 0.5f);
                fv = floorf(((qy * v.fy) / qz + v.cy) + 0.5f);
                in = fu >= 0.0f && fu < (float)v.w && fv >= 0.0f && fv < (float)v.h;
            }
            if (!in) {
                cls = 1;                                           /* OUT */
            } else {
                const int u = (int)fu, vv = (int)fv;
                const int u0 = max(u - window, 0), u1 = min(u + window, v.w - 1);
                const int v0 = max(vv - window, 0), v1 = min(vv + window, v.h - 1);
                const float tol = d->tol, lim = qz - tol;
                bool sup = false, near = false, any = false;
                for (int y = v0; y <= v1; y++) {
                    const float *row = v.z + (size_t)y * v.w;
                    for (int x = u0; x <= u1; x++) {
                        const float zo = row[x];
                        if (zo > 0.0f) {
                            any = true;
                            if (fabsf(zo - qz) <= tol) sup = true;
                            if (zo < lim) near = true;
                        }
                    }
                }
                cls = sup ? 2 : near ? 3 : any ? 4 : 5;            /* SUPPORTED, OCCLUDED, CONFLICT, UNKNOWN */
            }
        }
    }
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
