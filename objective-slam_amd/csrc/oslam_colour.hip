/*
 * oslam_colour.hip -- the colour volume's kernels (semantics: include/oslam.h at oslam_volume_integrate_colour,
 * oslam_volume_colours and oslam_volume_paint_view; host side: oslam_colour.c).  A colour word is r | g << 8 | b << 16 |
 * wc << 24 in the volume (wc = 0: never coloured) and r | g << 8 | b << 16 | a << 24 in an image (a = 255 or 0).
 *
 *   k_tsdf_colour     the colour pass of an integration: k_tsdf_integrate's layout (a workgroup of 256 threads is a tile
 *                     of 64 voxels in x by 4 in y and walks OSLAMK_VOL_ZRUN consecutive z, a wave touches 64 consecutive
 *                     words per z) and its arithmetic up to sdf, with the same grouping and the same hoisting out of the z
 *                     run.  A voxel outside the band, or whose pixel has no colour, is neither loaded nor stored; a voxel
 *                     belongs to one thread, so there is no atomic on the volume.  The running mean is integer arithmetic
 *                     per channel.  The updated voxels are counted per lane, summed over the wave (wave_sum) and added
 *                     with one integer atomic per wave.  No LDS, no scratch.
 *   k_colour_points   one thread per point: the colour at a volume-frame point, trilinear over the eight corners when all
 *                     of them are coloured, otherwise the colour of the voxel that holds the point.  Points with a colour
 *                     are counted by a ballot.
 *   k_colour_view     one thread per pixel in 32 x 8 tiles (k_tsdf_raycast's tiling): the pixel's vertex from its z, into
 *                     the volume frame, the same read, the word into the view's colour image.
 * Bounds.  k_tsdf_colour: a thread's (i, j) is checked against (nx, ny) before anything, k < nz by construction (nz is a
 * multiple of OSLAMK_VOL_ZRUN, checked by the launcher); the pixel is range-checked in float before it becomes an int,
 * and the one index serves the z image and the colour image, both w * h elements.  The reads of a colour at a point: the
 * base corner is range-checked in float against 0 .. n_a - 2 before it becomes an index, so the eight corners lie inside
 * the nx * ny * nz words; the nearest voxel is range-checked in float against 0 .. n_a - 1 likewise; a NaN or an infinite
 * coordinate fails both checks and reads nothing.  k_colour_points checks its index against n before anything,
 * k_colour_view its pixel against (w, h).
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_block_scan.h"
#include "oslam_colour_lerp.h"
#include "oslam_kernels.h"

__global__ __launch_bounds__(256) void k_tsdf_colour(const oslamk_volume vol, const oslamk_colour col, const oslamk_view v,
                                                     const uint32_t *__restrict__ rgba, const oslamk_pose P, uint32_t *count)
{
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k0 = blockIdx.z * OSLAMK_VOL_ZRUN;
    uint32_t mine = 0;
    if (i < vol.nx && j < vol.ny) {
        const float *T = P.T;
        const float gx = vol.origin[0] + ((float)i + 0.5f) * vol.voxel;
        const float gy = vol.origin[1] + ((float)j + 0.5f) * vol.voxel;
        const float ax = T[0] * gx + T[1] * gy, ay = T[4] * gx + T[5] * gy, az = T[8] * gx + T[9] * gy;
        uint32_t *column = col.words + ((size_t)k0 * vol.ny + (size_t)j) * vol.nx + (size_t)i;
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
            const size_t pixel = (size_t)(int)fv * v.w + (size_t)(int)fu;
            const float zo = v.z[pixel];
            if (!(zo > 0.0f)) continue;
            const float sdf = zo - pz;
            if (!(sdf >= -col.band && sdf <= col.band)) continue;
            const uint32_t pix = rgba[pixel];
            if ((pix >> 24) == 0u) continue;
            uint32_t *p = column + (size_t)kk * slice;
            const uint32_t word = *p, wc = word >> 24, den = wc + 1u, half = den >> 1;
            const uint32_t r = ((word & 0xffu) * wc + (pix & 0xffu) + half) / den;
            const uint32_t g = (((word >> 8) & 0xffu) * wc + ((pix >> 8) & 0xffu) + half) / den;
            const uint32_t b = (((word >> 16) & 0xffu) * wc + ((pix >> 16) & 0xffu) + half) / den;
            const uint32_t wn = den < col.max_weight ? den : col.max_weight;
            *p = r | (g << 8) | (b << 16) | (wn << 24);
            mine++;
        }
    }
    /* every lane of the wave arrives here: the wave's count, one integer add */
    const uint32_t s = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(count, s);
}

/* the colour at the volume-frame point (x, y, z) as an image word: a = 255 with a colour, the word 0 without */
__device__ __forceinline__ uint32_t colour_at(const oslamk_volume &vol, const uint32_t *__restrict__ words, float x, float y, float z)
{
    const float ux = (x - vol.origin[0]) * vol.inv_voxel, uy = (y - vol.origin[1]) * vol.inv_voxel;
    const float uz = (z - vol.origin[2]) * vol.inv_voxel;
    const float gx = ux - 0.5f, gy = uy - 0.5f, gz = uz - 0.5f;
    const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
    if (bx >= 0.0f && bx <= (float)(vol.nx - 2) && by >= 0.0f && by <= (float)(vol.ny - 2) && bz >= 0.0f &&
        bz <= (float)(vol.nz - 2)) {
        const size_t sy = (size_t)vol.nx, sz = (size_t)vol.nx * vol.ny;
        const uint32_t *p = words + ((size_t)(int)bz * vol.ny + (size_t)(int)by) * vol.nx + (size_t)(int)bx;
        const uint32_t c[8] = {p[0], p[1], p[sy], p[sy + 1], p[sz], p[sz + 1], p[sz + sy], p[sz + sy + 1]};
        if ((c[0] >> 24) && (c[1] >> 24) && (c[2] >> 24) && (c[3] >> 24) && (c[4] >> 24) && (c[5] >> 24) && (c[6] >> 24) &&
            (c[7] >> 24)) {
            const float fx = gx - bx, fy = gy - by, fz = gz - bz;
            return colour_channel(c, 0, fx, fy, fz) | (colour_channel(c, 8, fx, fy, fz) << 8) |
                   (colour_channel(c, 16, fx, fy, fz) << 16) | 0xff000000u;
        }
    }
    const float fi = floorf(ux), fj = floorf(uy), fk = floorf(uz);
    if (!(fi >= 0.0f && fi < (float)vol.nx && fj >= 0.0f && fj < (float)vol.ny && fk >= 0.0f && fk < (float)vol.nz)) return 0u;
    const uint32_t word = words[((size_t)(int)fk * vol.ny + (size_t)(int)fj) * vol.nx + (size_t)(int)fi];
    return (word >> 24) ? (word | 0xff000000u) : 0u;
}

__global__ __launch_bounds__(256) void k_colour_points(const oslamk_volume vol, const uint32_t *__restrict__ words,
                                                       const float *__restrict__ xyz, uint32_t n, uint32_t *__restrict__ out,
                                                       uint32_t *count)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t word = 0u;
    if (t < n) {
        word = colour_at(vol, words, xyz[3 * (size_t)t], xyz[3 * (size_t)t + 1], xyz[3 * (size_t)t + 2]);
        out[t] = word;
    }
    const uint32_t n_has = (uint32_t)__popcll(__ballot(word != 0u));
    if ((threadIdx.x & 63) == 0 && n_has) atomicAdd(count, n_has);
}

__global__ __launch_bounds__(256) void k_colour_view(const oslamk_volume vol, const uint32_t *__restrict__ words, const oslamk_view v,
                                                     const oslamk_pose P, uint32_t *__restrict__ out, uint32_t *count)
{
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), vv = blockIdx.y * 8 + (threadIdx.x >> 5);
    uint32_t word = 0u;
    if (u < v.w && vv < v.h) {
        const size_t i = (size_t)vv * v.w + u;
        const float z = v.z[i];
        if (z > 0.0f) {
            const float *M = P.T;
            const float dx = ((float)u - v.cx) / v.fx, dy = ((float)vv - v.cy) / v.fy;
            const float vx = dx * z, vy = dy * z;
            word = colour_at(vol, words, ((M[0] * vx + M[1] * vy) + M[2] * z) + M[3], ((M[4] * vx + M[5] * vy) + M[6] * z) + M[7],
                             ((M[8] * vx + M[9] * vy) + M[10] * z) + M[11]);
        }
        out[i] = word;
    }
    const uint32_t n_has = (uint32_t)__popcll(__ballot(word != 0u));
    if ((threadIdx.x & 63) == 0 && n_has) atomicAdd(count, n_has);
}

static bool colour_volume_ok(const oslamk_volume *vol, const uint32_t *words)
{
    return vol && words && oslamk_sides_ok(vol->nx, vol->ny, vol->nz, 2) && vol->nz % OSLAMK_VOL_ZRUN == 0 && vol->voxel > 0.0f;
}

extern "C" int oslamk_tsdf_colour(const oslamk_volume *vol, const oslamk_colour *col, const oslamk_view *v, const uint32_t *rgba,
                                  const float *T12, uint32_t *count, void *stream)
{
    oslamk_pose P;
    if (!col || !colour_volume_ok(vol, col->words) || !(col->band > 0.0f) || col->max_weight < 1u || col->max_weight > 255u || !v ||
        !v->z || !rgba || v->w <= 0 || v->h <= 0 || !T12 || !count)
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < 12; k++) P.T[k] = T12[k];
    hipLaunchKernelGGL(k_tsdf_colour, dim3((vol->nx + 63) / 64, (vol->ny + 3) / 4, vol->nz / OSLAMK_VOL_ZRUN), dim3(256), 0,
                       (hipStream_t)stream, *vol, *col, *v, rgba, P, count);
    return (int)hipGetLastError();
}

extern "C" int oslamk_colour_points(const oslamk_volume *vol, const uint32_t *words, const float *xyz, uint32_t n, uint32_t *out,
                                    uint32_t *count, void *stream)
{
    if (!colour_volume_ok(vol, words) || !xyz || !out || !count || n == 0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_colour_points, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, *vol, words, xyz, n, out, count);
    return (int)hipGetLastError();
}

extern "C" int oslamk_colour_view(const oslamk_volume *vol, const uint32_t *words, const oslamk_view *v, const float *T12,
                                  uint32_t *out, uint32_t *count, void *stream)
{
    oslamk_pose P;
    if (!colour_volume_ok(vol, words) || !v || !v->z || v->w <= 0 || v->h <= 0 || !T12 || !out || !count)
        return (int)hipErrorInvalidValue;
    for (int k = 0; k < 12; k++) P.T[k] = T12[k];
    hipLaunchKernelGGL(k_colour_view, dim3((v->w + 31) / 32, (v->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *vol, words, *v, P,
                       out, count);
    return (int)hipGetLastError();
}
