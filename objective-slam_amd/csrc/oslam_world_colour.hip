/*
 * oslam_world_colour.hip -- the colour at points of the whole map, voxel store plus window (semantics: include/oslam.h at
 * oslam_world_colours; host side: oslam_world_colour.c).  The map is the table of oslam_world_surface.hip with the brick
 * array holding colour words r | g << 8 | b << 16 | wc << 24: the store's colour bricks sent up, the window's colour
 * buffer written over its box by k_brick_window, which copies words whatever they mean.
 *
 *   k_brick_colours   one thread per point: colour_at of oslam_colour.hip against the map, float sequence unchanged.  The
 *                     base corner A + b of the trilinear stencil is found by one binary search of the table; where the
 *                     stencil stays inside that brick (all three local coordinates <= 6) the eight words come from it,
 *                     otherwise each corner is looked up through map_word.  With all eight coloured the channels are
 *                     blended (oslam_colour_lerp.h); otherwise the voxel that holds the point, A + floorf(u), is looked up
 *                     on its own: in float arithmetic it is not shown to be one of the eight corners.  Points with a
 *                     colour are counted by a ballot and one integer atomic per wave.  No LDS, no scratch, no float atomic.
 *   k_brick_colour_view   one thread per pixel in 32 x 8 tiles (k_colour_view's tiling and arithmetic): the pixel's vertex
 *                     from its z, into the volume frame, the same read, the word into the view's colour image
 *                     (oslam_world_paint_view).
 * Bounds.  A thread's index is checked against n before anything, a pixel against (w, h).  b and floorf(u) are range-checked in float (finite and
 * below 2^22 in size) before they become ints, so with |A_a| <= 2^20 every global coordinate read is below 2^23 in size and
 * its brick coordinate fits the key's 21 bits.  brick_find gives a slot below m.n or none, so every load from the brick
 * array lies inside its n * 512 words; a local index is below 512 by construction, and the in-brick stencil adds at most
 * 73 to a local index of at most 6 + 8 * 6 + 64 * 6 = 438.  A NaN or infinite coordinate fails both range checks and reads
 * nothing.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_brick.h"
#include "oslam_colour_lerp.h"
#include "oslam_kernels.h"

__device__ __forceinline__ bool wcol_in_range(float a, float b, float c)
{
    return fabsf(a) < BRK_COORD_MAX && fabsf(b) < BRK_COORD_MAX && fabsf(c) < BRK_COORD_MAX;      /* false for a NaN */
}

/* the colour at the volume-frame point (x, y, z) as an image word: a = 255 with a colour, the word 0 without */
__device__ __forceinline__ uint32_t wcol_at(const oslamk_brick_map &m, float x, float y, float z)
{
    const float ux = (x - m.origin[0]) * m.inv_voxel, uy = (y - m.origin[1]) * m.inv_voxel;
    const float uz = (z - m.origin[2]) * m.inv_voxel;
    const float gx = ux - 0.5f, gy = uy - 0.5f, gz = uz - 0.5f;
    const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
    if (wcol_in_range(bx, by, bz)) {
        const int cx = m.anchor[0] + (int)bx, cy = m.anchor[1] + (int)by, cz = m.anchor[2] + (int)bz;   /* below 2^23 in size */
        uint32_t c[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};           /* without a brick no corner has a colour */
        if ((cx & 7) <= 6 && (cy & 7) <= 6 && (cz & 7) <= 6) {
            const uint32_t slot = brick_find(m, OSLAMK_BRICK_KEY(cx >> 3, cy >> 3, cz >> 3));
            if (slot != BRK_NONE) {
                const uint32_t *p = m.words + (size_t)slot * OSLAMK_BRICK_WORDS + brick_local(cx, cy, cz);
                c[0] = p[0], c[1] = p[1], c[2] = p[8], c[3] = p[9], c[4] = p[64], c[5] = p[65], c[6] = p[72], c[7] = p[73];
            }
        } else {
            c[0] = map_word(m, cx, cy, cz);
            /* the other seven only while a colour is still possible: a lane saves its searches, the result is the same */
            if (c[0] >> 24) {
                c[1] = map_word(m, cx + 1, cy, cz), c[2] = map_word(m, cx, cy + 1, cz), c[3] = map_word(m, cx + 1, cy + 1, cz);
                c[4] = map_word(m, cx, cy, cz + 1), c[5] = map_word(m, cx + 1, cy, cz + 1), c[6] = map_word(m, cx, cy + 1, cz + 1);
                c[7] = map_word(m, cx + 1, cy + 1, cz + 1);
            }
        }
        if ((c[0] >> 24) && (c[1] >> 24) && (c[2] >> 24) && (c[3] >> 24) && (c[4] >> 24) && (c[5] >> 24) && (c[6] >> 24) &&
            (c[7] >> 24)) {
            const float fx = gx - bx, fy = gy - by, fz = gz - bz;
            return colour_channel(c, 0, fx, fy, fz) | (colour_channel(c, 8, fx, fy, fz) << 8) |
                   (colour_channel(c, 16, fx, fy, fz) << 16) | 0xff000000u;
        }
    }
    const float fi = floorf(ux), fj = floorf(uy), fk = floorf(uz);
    if (!wcol_in_range(fi, fj, fk)) return 0u;
    const uint32_t word = map_word(m, m.anchor[0] + (int)fi, m.anchor[1] + (int)fj, m.anchor[2] + (int)fk);
    return (word >> 24) ? (word | 0xff000000u) : 0u;
}

__global__ __launch_bounds__(256) void k_brick_colours(const oslamk_brick_map m, const float *__restrict__ xyz, uint32_t n,
                                                       uint32_t *__restrict__ out, uint32_t *count)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t word = 0u;
    if (t < n) {
        word = wcol_at(m, xyz[3 * (size_t)t], xyz[3 * (size_t)t + 1], xyz[3 * (size_t)t + 2]);
        out[t] = word;
    }
    const uint32_t n_has = (uint32_t)__popcll(__ballot(word != 0u));
    if ((threadIdx.x & 63) == 0 && n_has) atomicAdd(count, n_has);
}

/* k_colour_view against the map: the pixel's vertex from its z, into the volume frame, wcol_at there */
__global__ __launch_bounds__(256) void k_brick_colour_view(const oslamk_brick_map m, const oslamk_view v, const oslamk_pose P,
                                                           uint32_t *__restrict__ out, uint32_t *count)
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
            word = wcol_at(m, ((M[0] * vx + M[1] * vy) + M[2] * z) + M[3], ((M[4] * vx + M[5] * vy) + M[6] * z) + M[7],
                           ((M[8] * vx + M[9] * vy) + M[10] * z) + M[11]);
        }
        out[i] = word;
    }
    const uint32_t n_has = (uint32_t)__popcll(__ballot(word != 0u));
    if ((threadIdx.x & 63) == 0 && n_has) atomicAdd(count, n_has);
}

extern "C" int oslamk_brick_colour_view(const oslamk_brick_map *map, const oslamk_view *v, const float *T12, uint32_t *out,
                                        uint32_t *count, void *stream)
{
    oslamk_pose P;
    if (!brick_map_ok(map) || !v || !v->z || v->w <= 0 || v->h <= 0 || !T12 || !out || !count) return (int)hipErrorInvalidValue;
    for (int k = 0; k < 12; k++) P.T[k] = T12[k];
    hipLaunchKernelGGL(k_brick_colour_view, dim3((v->w + 31) / 32, (v->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *map, *v, P,
                       out, count);
    return (int)hipGetLastError();
}

extern "C" int oslamk_brick_colours(const oslamk_brick_map *map, const float *xyz, uint32_t n, uint32_t *out, uint32_t *count,
                                    void *stream)
{
    if (!brick_map_ok(map) || !xyz || !out || !count || n == 0u || n > 0x7fffffffu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_brick_colours, dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, *map, xyz, n, out, count);
    return (int)hipGetLastError();
}
