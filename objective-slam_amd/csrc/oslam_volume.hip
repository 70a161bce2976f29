/*
 * oslam_volume.hip -- the fusion stage's kernels (semantics: include/oslam.h at oslam_volume_integrate and
 * oslam_volume_raycast; host side: oslam_volume.c).
 *
 *   k_tsdf_integrate   a streaming pass over the volume's words.  A workgroup of 256 threads is a tile of 64 voxels in x
 *                      by 4 in y and walks OSLAMK_VOL_ZRUN consecutive z; a wave touches 64 consecutive words per z.  The
 *                      k-independent part of p' = ((T0*gx + T1*gy) + T2*gz) + T3 is hoisted out of the z loop (the
 *                      pinned grouping allows it without changing a bit).  A voxel the rule skips is neither loaded nor
 *                      stored; a voxel belongs to one thread, so there is no atomic on the volume.  The updated voxels
 *                      are counted per lane, summed over the wave (wave_sum, oslam_block_scan.h) and added as integers
 *                      (one integer atomic per wave: a count does not depend on the order).  No LDS, no scratch.
 *   k_tsdf_raycast     one thread per pixel in 32 x 8 tiles (k_view_normals' tiling), so neighbouring rays read
 *                      neighbouring voxels.  The march, the crossing, the two trilinear reads, the six of the gradient
 *                      and the records of the view (z image and 32-byte map records) in one kernel.  Ray lengths
 *                      diverge within a wave; hits and normals are counted by ballots.  No LDS, no scratch.
 * Bounds.  Integration: a thread's (i, j) is checked against (nx, ny) before anything, k < nz by construction (nz is a
 * multiple of OSLAMK_VOL_ZRUN, checked by the launcher); the pixel is range-checked in float before it becomes an int,
 * so the gather reads inside the w * h floats of the z image.  Ray cast: the slab interval is shrunk by one voxel, and
 * on top of that every voxel coordinate is range-checked in float before it becomes an index (a read that would fall
 * outside counts as a voxel with w = 0), so no load leaves the nx * ny * nz words; a thread's pixel is checked against
 * (w, h) before its stores.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_block_scan.h"
#include "oslam_kernels.h"
#include "oslam_tsdf_read.h"
#include "ppf_math.h"

__global__ __launch_bounds__(256) void k_tsdf_integrate(const oslamk_volume vol, const oslamk_view v, const oslamk_pose P,
                                                        uint32_t *count)
{
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k0 = blockIdx.z * OSLAMK_VOL_ZRUN;
    uint32_t mine = 0;
    if (i < vol.nx && j < vol.ny) {
        const float *T = P.T;
        const float gx = vol.origin[0] + ((float)i + 0.5f) * vol.voxel;
        const float gy = vol.origin[1] + ((float)j + 0.5f) * vol.voxel;
        const float ax = T[0] * gx + T[1] * gy, ay = T[4] * gx + T[5] * gy, az = T[8] * gx + T[9] * gy;
        uint32_t *col = vol.words + ((size_t)k0 * vol.ny + (size_t)j) * vol.nx + (size_t)i;
        const size_t slice = (size_t)vol.ny * vol.nx;
#pragma unroll 4
        for (int kk = 0; kk < OSLAMK_VOL_ZRUN; kk++) {
            const float gz = vol.origin[2] + ((float)(k0 + kk) + 0.5f) * vol.voxel;
            const float pz = (az + T[10] * gz) + T[11];
            if (!(pz > 0.0f)) continue;
            const float px = (ax + T[2] * gz) + T[3], py = (ay + T[6] * gz) + T[7];
            const float fu = floorf(((px * v.fx) / pz + v.cx) + 0.5f);
            const float fv = floorf(((py * v.fy) / pz + v.cy) + 0.5f);
            if (!(fu >= 0.0f && fu < (float)v.w && fv >= 0.0f && fv < (float)v.h)) continue;
            const float zo = v.z[(size_t)(int)fv * v.w + (size_t)(int)fu];
            if (!(zo > 0.0f)) continue;
            const float sdf = zo - pz;
            if (!(sdf >= -vol.mu)) continue;
            const float f = fminf(1.0f, sdf / vol.mu);
            uint32_t *p = col + (size_t)kk * slice;
            const uint32_t word = *p, w = word >> 16;
            const float Fn = ((tsdf_of(word) * (float)w) + f) / (float)(w + 1u);
            const int q = (int)rintf(Fn * 32767.0f);
            const uint32_t wn = w + 1u < vol.max_weight ? w + 1u : vol.max_weight;
            *p = ((uint32_t)q & 0xffffu) | (wn << 16);
            mine++;
        }
    }
    /* every lane of the wave arrives here: the wave's count, one integer add */
    const uint32_t s = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(count, s);
}

/* the word of the voxel that holds the voxel coordinate (gx, gy, gz), 0 (w = 0) outside the volume */
__device__ __forceinline__ uint32_t tsdf_nearest(const oslamk_volume &vol, float gx, float gy, float gz)
{
    const float fi = floorf(gx), fj = floorf(gy), fk = floorf(gz);
    if (!(fi >= 0.0f && fi < (float)vol.nx && fj >= 0.0f && fj < (float)vol.ny && fk >= 0.0f && fk < (float)vol.nz)) return 0u;
    return vol.words[((size_t)(int)fk * vol.ny + (size_t)(int)fj) * vol.nx + (size_t)(int)fi];
}

/* one axis of the slab test: false when the ray misses the slab [lo, hi] */
__device__ __forceinline__ bool tsdf_slab(float o, float d, float lo, float hi, float *tn, float *tf)
{
    if (d == 0.0f) return o >= lo && o <= hi;
    const float ta = (lo - o) / d, tb = (hi - o) / d;
    *tn = fmaxf(*tn, fminf(ta, tb));
    *tf = fminf(*tf, fmaxf(ta, tb));
    return true;
}

/* the crossing of pixel's ray: t* (> 0), or 0 without a hit */
__device__ __forceinline__ float tsdf_march(const oslamk_volume &vol, const float o[3], const float d[3], float z_min,
                                            float z_max)
{
    float tn = z_min, tf = z_max;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int n = a == 0 ? vol.nx : a == 1 ? vol.ny : vol.nz;
        const float lo = vol.origin[a] + vol.voxel, hi = vol.origin[a] + (float)(n - 1) * vol.voxel;
        if (!tsdf_slab(o[a], d[a], lo, hi, &tn, &tf)) return 0.0f;
    }
    if (!(tn <= tf)) return 0.0f;
    const float step = 0.5f * vol.mu;
    bool have = false;
    float Fp = 0.0f, tp = 0.0f;
    for (int k = 0; k < OSLAMK_VOL_MAX_STEPS; k++) {
        const float t = tn + (float)k * step;
        if (!(t <= tf)) break;
        const float x = o[0] + d[0] * t, y = o[1] + d[1] * t, z = o[2] + d[2] * t;
        const uint32_t word = tsdf_nearest(vol, (x - vol.origin[0]) * vol.inv_voxel, (y - vol.origin[1]) * vol.inv_voxel,
                                           (z - vol.origin[2]) * vol.inv_voxel);
        if ((word >> 16) == 0u) {
            have = false;
            continue;
        }
        const float F = tsdf_of(word);
        if (have && Fp > 0.0f && F < 0.0f) {
            float Ft, Ftdt;
            if (!tsdf_trilinear(vol, o[0] + d[0] * tp, o[1] + d[1] * tp, o[2] + d[2] * tp, &Ft) ||
                !tsdf_trilinear(vol, x, y, z, &Ftdt))
                return 0.0f;
            const float den = Ftdt - Ft;
            if (!(den < 0.0f)) return 0.0f;
            const float ts = tp - (step * Ft) / den;
            if (!(ts >= tp && ts <= t && ts >= z_min && ts <= z_max)) return 0.0f;
            return ts;
        }
        if (have && Fp < 0.0f && F > 0.0f) return 0.0f;
        have = true;
        Fp = F;
        tp = t;
    }
    return 0.0f;
}

__global__ __launch_bounds__(256) void k_tsdf_raycast(const oslamk_volume vol, const oslamk_view v, const oslamk_pose P,
                                                      float *z_out, float *maps, uint32_t *count)
{
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), vv = blockIdx.y * 8 + (threadIdx.x >> 5);
    const bool inside = u < v.w && vv < v.h;
    bool hit = false, has = false;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    float ts = 0.0f;
    if (inside) {
        const float *M = P.T;
        const float dx = ((float)u - v.cx) / v.fx, dy = ((float)vv - v.cy) / v.fy;
        const float o[3] = {M[3], M[7], M[11]};
        const float d[3] = {(M[0] * dx + M[1] * dy) + M[2], (M[4] * dx + M[5] * dy) + M[6], (M[8] * dx + M[9] * dy) + M[10]};
        ts = tsdf_march(vol, o, d, v.z_min, v.z_max);
        hit = ts > 0.0f;
        if (hit) {
            const float px = o[0] + d[0] * ts, py = o[1] + d[1] * ts, pz = o[2] + d[2] * ts;
            const float h = vol.voxel;
            float x0, x1, y0, y1, z0, z1;
            if (tsdf_trilinear(vol, px + h, py, pz, &x1) && tsdf_trilinear(vol, px - h, py, pz, &x0) &&
                tsdf_trilinear(vol, px, py + h, pz, &y1) && tsdf_trilinear(vol, px, py - h, pz, &y0) &&
                tsdf_trilinear(vol, px, py, pz + h, &z1) && tsdf_trilinear(vol, px, py, pz - h, &z0)) {
                const float gx = x1 - x0, gy = y1 - y0, gz = z1 - z0;
                const float len = pm_sqrtf(gx * gx + gy * gy + gz * gz);
                if (len > 0.0f && len <= 3.0e38f) {
                    const float nx = gx / len, ny = gy / len, nz = gz / len;
                    const float cx_ = (M[0] * nx + M[4] * ny) + M[8] * nz;
                    const float cy_ = (M[1] * nx + M[5] * ny) + M[9] * nz;
                    const float cz_ = (M[2] * nx + M[6] * ny) + M[10] * nz;
                    const float vx = dx * ts, vy = dy * ts;
                    if ((cx_ * vx + cy_ * vy) + cz_ * ts < 0.0f) {
                        has = true;
                        a = make_float4(vx, vy, ts, 1.0f);
                        b = make_float4(cx_, cy_, cz_, 0.0f);
                    }
                }
            }
        }
        const size_t i = (size_t)vv * v.w + u;
        z_out[i] = ts;
        float4 *dst = reinterpret_cast<float4 *>(maps) + 2 * i;
        dst[0] = a;
        dst[1] = b;
    }
    const uint32_t n_hit = (uint32_t)__popcll(__ballot(hit)), n_has = (uint32_t)__popcll(__ballot(has));
    if ((threadIdx.x & 63) == 0) {
        if (n_hit) atomicAdd(count, n_hit);
        if (n_has) atomicAdd(count + 1, n_has);
    }
}

static bool volume_ok(const oslamk_volume *vol)
{
    return vol->words && oslamk_sides_ok(vol->nx, vol->ny, vol->nz, 2) && vol->nz % OSLAMK_VOL_ZRUN == 0 && vol->voxel > 0.0f &&
           vol->mu > 0.0f;
}

extern "C" int oslamk_tsdf_integrate(const oslamk_volume *vol, const oslamk_view *v, const float *T12, uint32_t *count,
                                     void *stream)
{
    oslamk_pose P;
    if (!volume_ok(vol) || !v->z || v->w <= 0 || v->h <= 0 || !count) return (int)hipErrorInvalidValue;
    for (int k = 0; k < 12; k++) P.T[k] = T12[k];
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((vol->nx + 63) / 64, (vol->ny + 3) / 4, vol->nz / OSLAMK_VOL_ZRUN), dim3(256), 0,
                       (hipStream_t)stream, *vol, *v, P, count);
    return (int)hipGetLastError();
}

extern "C" int oslamk_tsdf_raycast(const oslamk_volume *vol, const oslamk_view *v, const float *T12, float *z_out, float *maps,
                                   uint32_t *count, void *stream)
{
    oslamk_pose P;
    if (!volume_ok(vol) || v->w <= 0 || v->h <= 0 || !z_out || !maps || !count) return (int)hipErrorInvalidValue;
    for (int k = 0; k < 12; k++) P.T[k] = T12[k];
    hipLaunchKernelGGL(k_tsdf_raycast, dim3((v->w + 31) / 32, (v->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *vol, *v, P,
                       z_out, maps, count);
    return (int)hipGetLastError();
}
