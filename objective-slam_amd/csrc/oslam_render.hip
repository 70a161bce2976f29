/*
 * oslam_render.hip -- the render stage's kernels (semantics: include/oslam.h at oslam_render_create and
 * oslam_view_mask; host side: oslam_render.c).
 *
 *   k_render_splat    one thread per model point, every hypothesis of the call in one grid (y = hypothesis, x = block
 *                     of 256 model points, k_verify's grid over k_verify's descriptors): transform, BACK, OUT (both
 *                     oslam_icp_core.h's, unchanged), the half-width k, then one 64-bit unsigned atomicMin of the key
 *                     (bits of p'z) << 32 | h into every pixel of the clipped window.  An unsigned minimum does not
 *                     depend on the order of its operands: the image is the same for every order of points, waves and
 *                     workgroups.  The atomics return nothing and compile to global_atomic_umin_x2, at most 17 x 17 a
 *                     point.  drawn: a wave ballot + popcount, the four waves summed in LDS (16 bytes, the only LDS)
 *                     and one integer atomicAdd per workgroup.  No scratch.
 *   k_render_resolve  one thread per pixel, a 32 x 8 tile per workgroup as in k_view_z: key -> z and label; pixels[label]
 *                     by one integer atomicAdd per wave and label (the lanes of a wave that hold the same label are
 *                     counted by a ballot).  The first workgroup also copies the hypotheses' tolerances out of their
 *                     descriptors for the mask.
 *   k_view_mask       one thread per pixel, the same tile: the (2 dilate + 1)^2 window of labels and rendered z around
 *                     an observed pixel, clipped to the image; three integer counters by ballot + popcount, the four
 *                     waves summed in LDS, one atomicAdd per counter and workgroup.
 *
 * Bounds.  k_render_splat reads point i < m.n of its hypothesis only; the centre pixel is range-checked in float before
 * it becomes an int (oslam_icp_project), 0 <= k <= 8, and every atomic goes to (x, y) with max(u - k, 0) <= x <=
 * min(u + k, w - 1) and the same in y: inside the w x h key buffer.  The label of a key is blockIdx.y < n_mem, so
 * k_render_resolve's pixels[label] and k_view_mask's tol[label] stay inside their n_mem entries.  k_render_resolve and
 * k_view_mask touch pixel (u, v) only when u < w and v < h, and the mask's window is clipped the same way.  Pixel
 * indices are size_t: w * h may reach 2^28.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_icp_core.h"
#include "oslam_kernels.h"

#define RENDER_EMPTY 0xffffffffffffffffull

__global__ __launch_bounds__(OSLAMK_VERIFY_THREADS) void k_render_splat(const oslamk_view v, const oslamk_verify_member *mem,
                                                                        const float *rho, int max_splat, int keep_back,
                                                                        unsigned long long *keys, uint32_t *drawn)
{
    __shared__ uint32_t sh[OSLAMK_VERIFY_THREADS / 64];
    const uint32_t j = blockIdx.y;
    const oslamk_verify_member *d = &mem[j];
    if (blockIdx.x >= d->n_blocks) return;     /* the whole workgroup leaves together */
    const int i = (int)(blockIdx.x * OSLAMK_VERIFY_THREADS + threadIdx.x);
    bool draw = false;

    if (i < d->m.n) {
        float q[3], m[3];
        int u, vv;
        oslam_icp_transform(d->T, d->m.px[i], d->m.py[i], d->m.pz[i], d->m.nx[i], d->m.ny[i], d->m.nz[i], q, m);
        const bool back = (m[0] * q[0] + m[1] * q[1]) + m[2] * q[2] >= 0.0f;
        if ((keep_back || !back) && oslam_icp_project(v, q, &u, &vv)) {
            const float kf = floorf((rho[j] * v.fx) / q[2] + 0.5f);
            const int k = kf < (float)max_splat ? (int)kf : max_splat;
            const int u0 = max(u - k, 0), u1 = min(u + k, v.w - 1);
            const int v0 = max(vv - k, 0), v1 = min(vv + k, v.h - 1);
            const unsigned long long key = ((unsigned long long)__float_as_uint(q[2]) << 32) | j;
            for (int y = v0; y <= v1; y++) {
                unsigned long long *row = keys + (size_t)y * v.w;
                for (int x = u0; x <= u1; x++) atomicMin(&row[x], key);
            }
            draw = true;
        }
    }

    const unsigned long long b = __ballot(draw);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int ww = 0; ww < OSLAMK_VERIFY_THREADS / 64; ww++) s += sh[ww];
        if (s) atomicAdd(&drawn[j], s);
    }
}

__global__ __launch_bounds__(256) void k_render_resolve(const unsigned long long *keys, int w, int h,
                                                        const oslamk_verify_member *mem, uint32_t n_mem, float *z_out,
                                                        int32_t *labels, float *tol_out, uint32_t *pixels)
{
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), v = blockIdx.y * 8 + (threadIdx.x >> 5);
    const int lane = threadIdx.x & 63;
    int lab = -1;
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (uint32_t k = threadIdx.x; k < n_mem; k += 256) tol_out[k] = mem[k].tol;
    if (u < w && v < h) {
        const size_t i = (size_t)v * w + u;
        const unsigned long long key = keys[i];
        if (key != RENDER_EMPTY) lab = (int)(uint32_t)key;
        z_out[i] = key != RENDER_EMPTY ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        labels[i] = lab;
    }
    /* every lane of the wave takes part in the ballots, the ones outside the image with nothing to count */
    bool pending = lab >= 0;
    for (;;) {
        const unsigned long long todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int l0 = __shfl(lab, leader);
        const unsigned long long same = __ballot(pending && lab == l0);
        if (lane == leader) atomicAdd(&pixels[l0], (uint32_t)__popcll(same));
        if (lab == l0) pending = false;
    }
}

__global__ __launch_bounds__(256) void k_view_mask(const oslamk_view v, const float *z_r, const int32_t *labels,
                                                   const float *tol, int mode, int dilate, int32_t only, float *z_out,
                                                   uint32_t *counts)
{
    __shared__ uint32_t sh[4][3];
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), vv = blockIdx.y * 8 + (threadIdx.x >> 5);
    bool valid = false, object = false, kept = false;
    if (u < v.w && vv < v.h) {
        const size_t i = (size_t)vv * v.w + u;
        const float zo = v.z[i];
        valid = zo > 0.0f;
        if (valid) {
            const int u0 = max(u - dilate, 0), u1 = min(u + dilate, v.w - 1);
            const int v0 = max(vv - dilate, 0), v1 = min(vv + dilate, v.h - 1);
            for (int y = v0; y <= v1 && !object; y++) {
                const size_t row = (size_t)y * v.w;
                for (int x = u0; x <= u1; x++) {
                    const int32_t l = labels[row + x];
                    if (l < 0 || (only >= 0 && l != only)) continue;
                    if (fabsf(zo - z_r[row + x]) <= tol[l]) {
                        object = true;
                        break;
                    }
                }
            }
        }
        kept = valid && (mode == 1 ? object : !object);
        z_out[i] = kept ? zo : 0.0f;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b0 = __ballot(valid), b1 = __ballot(object), b2 = __ballot(kept);
    if (lane == 0) {
        sh[wv][0] = (uint32_t)__popcll(b0);
        sh[wv][1] = (uint32_t)__popcll(b1);
        sh[wv][2] = (uint32_t)__popcll(b2);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t s = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
        if (s) atomicAdd(&counts[threadIdx.x], s);
    }
}

extern "C" int oslamk_render_splat(const oslamk_view *v, const oslamk_verify_member *d_mem, const float *d_rho,
                                   uint32_t n_mem, uint32_t max_blocks, int max_splat, int keep_back,
                                   unsigned long long *keys, uint32_t *drawn, void *stream)
{
    if (n_mem == 0 || max_blocks == 0) return 0;
    if (n_mem > 65535u || max_splat < 0 || max_splat > OSLAMK_RENDER_MAX_SPLAT || v->w <= 0 || v->h <= 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_render_splat, dim3(max_blocks, n_mem), dim3(OSLAMK_VERIFY_THREADS), 0, (hipStream_t)stream, *v,
                       d_mem, d_rho, max_splat, keep_back != 0, keys, drawn);
    return (int)hipGetLastError();
}

extern "C" int oslamk_render_resolve(const unsigned long long *keys, int w, int h, const oslamk_verify_member *d_mem,
                                     uint32_t n_mem, float *z_out, int32_t *labels, float *tol_out, uint32_t *pixels,
                                     void *stream)
{
    if (w <= 0 || h <= 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_render_resolve, dim3((w + 31) / 32, (h + 7) / 8), dim3(256), 0, (hipStream_t)stream, keys, w, h,
                       d_mem, n_mem, z_out, labels, tol_out, pixels);
    return (int)hipGetLastError();
}

extern "C" int oslamk_view_mask(const oslamk_view *v, const float *z_r, const int32_t *labels, const float *tol, int mode,
                                int dilate, int32_t only, float *z_out, uint32_t *counts, void *stream)
{
    if (v->w <= 0 || v->h <= 0 || dilate < 0 || dilate > OSLAMK_MASK_MAX_DILATE || (mode != 0 && mode != 1))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_view_mask, dim3((v->w + 31) / 32, (v->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *v, z_r,
                       labels, tol, mode, dilate, only, z_out, counts);
    return (int)hipGetLastError();
}
