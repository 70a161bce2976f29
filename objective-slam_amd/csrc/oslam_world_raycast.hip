/*
 * oslam_world_raycast.hip -- the whole map, voxel store plus window, ray-cast back into a view from its sparse bricks
 * (semantics: include/oslam.h at oslam_world_raycast; host side: oslam_world_raycast.c).  The map is the table of
 * oslam_world_surface.hip: ascending packed keys, slots, [n][512] bricks with the window written in by k_brick_window.
 *
 *   k_brick_raycast   one thread per pixel in 32 x 8 tiles (k_tsdf_raycast's tiling), so the rays of a wave walk
 *                     neighbouring bricks.  The march, the crossing, the two trilinear reads, the six of the gradient and
 *                     the records of the view are k_tsdf_raycast's, float sequence and grouping unchanged; the slab comes
 *                     from a box in voxel indices, and every read goes through the table.  A lane keeps the brick of its
 *                     last sample (packed key and slot, "absent" being an answer too): with a step of 2 voxels about
 *                     four consecutive samples share a brick, and a ray through empty space pays the coordinate
 *                     arithmetic and one 64-bit compare per sample.  The cache only memoises brick_find, so it cannot
 *                     change a bit.  A trilinear read takes its eight words from one brick where the base's three local
 *                     coordinates are <= 6 (k_brick_colours' split), and goes corner by corner through map_word
 *                     otherwise.  Ray lengths diverge within a wave; hits and normals are counted by ballots and one
 *                     integer atomic per wave.  No LDS, no scratch, no float atomic: two calls give the same bytes.
 * Bounds.  A sample's voxel coordinate and a trilinear base are range-checked in float (finite and below 2^22 in size)
 * before they become ints, so with |A_a| <= 2^20 every global coordinate read is below 2^23 in size and its brick
 * coordinate fits the key's 21 bits; a NaN or an infinite coordinate fails the check and reads as a voxel with w = 0.
 * brick_find gives a slot below m.n or none, and the cache holds nothing but its answers, so every load from the brick
 * array lies inside its n * 512 words; a local index is below 512 by construction, and the in-brick stencil adds at most
 * 73 to a local index of at most 6 + 8 * 6 + 64 * 6 = 438.  The march ends at t > tf or after OSLAMK_WRAY_MAX_STEPS
 * samples; the host refuses the calls in which the second could come first.  A thread's pixel is checked against (w, h)
 * before its stores.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_brick.h"
#include "oslam_kernels.h"
#include "ppf_math.h"

#define WRAY_NO_KEY 0xffffffffffffffffull     /* no brick has it: a key is 63 bits */

/* a lane's memo of brick_find: the key it asked last and the answer (BRK_NONE = absent) */
struct wray_cache {
    uint64_t key;
    uint32_t slot;
};

__device__ __forceinline__ uint32_t wray_find(const oslamk_brick_map &m, wray_cache &c, uint64_t key)
{
    if (key != c.key) {
        c.slot = brick_find(m, key);
        c.key = key;
    }
    return c.slot;
}

/* G at the voxel that holds the voxel coordinate (ux, uy, uz) of the frame of m, 0 (w = 0) outside the range */
__device__ __forceinline__ uint32_t wray_nearest(const oslamk_brick_map &m, wray_cache &c, float ux, float uy, float uz)
{
    const float fi = floorf(ux), fj = floorf(uy), fk = floorf(uz);
    if (!(fabsf(fi) < BRK_COORD_MAX && fabsf(fj) < BRK_COORD_MAX && fabsf(fk) < BRK_COORD_MAX)) return 0u;   /* false for a NaN */
    const int gx = m.anchor[0] + (int)fi, gy = m.anchor[1] + (int)fj, gz = m.anchor[2] + (int)fk;           /* below 2^23 in size */
    const uint32_t slot = wray_find(m, c, OSLAMK_BRICK_KEY(gx >> 3, gy >> 3, gz >> 3));
    return slot == BRK_NONE ? 0u : m.words[(size_t)slot * OSLAMK_BRICK_WORDS + brick_local(gx, gy, gz)];
}

/* brick_trilinear without a tile: the eight corners from the base's brick where the stencil stays inside it, through the
 * table corner by corner otherwise; the arithmetic is tsdf_trilinear's, grouping unchanged */
__device__ __forceinline__ bool wray_trilinear(const oslamk_brick_map &m, float x, float y, float z, float *out)
{
    const float gx = (x - m.origin[0]) * m.inv_voxel - 0.5f;
    const float gy = (y - m.origin[1]) * m.inv_voxel - 0.5f;
    const float gz = (z - m.origin[2]) * m.inv_voxel - 0.5f;
    const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
    if (!(fabsf(bx) < BRK_COORD_MAX && fabsf(by) < BRK_COORD_MAX && fabsf(bz) < BRK_COORD_MAX)) return false;
    const float fx = gx - bx, fy = gy - by, fz = gz - bz;
    const int cx = m.anchor[0] + (int)bx, cy = m.anchor[1] + (int)by, cz = m.anchor[2] + (int)bz;     /* below 2^23 in size */
    uint32_t w000, w100, w010, w110, w001, w101, w011, w111;
    if ((cx & 7) <= 6 && (cy & 7) <= 6 && (cz & 7) <= 6) {
        const uint32_t slot = brick_find(m, OSLAMK_BRICK_KEY(cx >> 3, cy >> 3, cz >> 3));
        if (slot == BRK_NONE) return false;                         /* every corner reads 0 */
        const uint32_t *p = m.words + (size_t)slot * OSLAMK_BRICK_WORDS + brick_local(cx, cy, cz);
        w000 = p[0], w100 = p[1], w010 = p[8], w110 = p[9], w001 = p[64], w101 = p[65], w011 = p[72], w111 = p[73];
    } else {
        w000 = map_word(m, cx, cy, cz), w100 = map_word(m, cx + 1, cy, cz), w010 = map_word(m, cx, cy + 1, cz), w110 = map_word(m, cx + 1, cy + 1, cz);
        w001 = map_word(m, cx, cy, cz + 1), w101 = map_word(m, cx + 1, cy, cz + 1), w011 = map_word(m, cx, cy + 1, cz + 1), w111 = map_word(m, cx + 1, cy + 1, cz + 1);
    }
    if (!((w000 >> 16) && (w100 >> 16) && (w010 >> 16) && (w110 >> 16) && (w001 >> 16) && (w101 >> 16) && (w011 >> 16) &&
          (w111 >> 16)))
        return false;
    const float c00 = tsdf_lerp(tsdf_of(w000), tsdf_of(w100), fx), c10 = tsdf_lerp(tsdf_of(w010), tsdf_of(w110), fx);
    const float c01 = tsdf_lerp(tsdf_of(w001), tsdf_of(w101), fx), c11 = tsdf_lerp(tsdf_of(w011), tsdf_of(w111), fx);
    *out = tsdf_lerp(tsdf_lerp(c00, c10, fy), tsdf_lerp(c01, c11, fy), fz);
    return true;
}

/* one axis of the slab test (tsdf_slab): false when the ray misses the slab [lo, hi] */
__device__ __forceinline__ bool wray_slab(float o, float d, float lo, float hi, float *tn, float *tf)
{
    if (d == 0.0f) return o >= lo && o <= hi;
    const float ta = (lo - o) / d, tb = (hi - o) / d;
    *tn = fmaxf(*tn, fminf(ta, tb));
    *tf = fminf(*tf, fmaxf(ta, tb));
    return true;
}

/* tsdf_march against the map: the crossing of the pixel's ray, t* (> 0), or 0 without a hit */
__device__ __forceinline__ float wray_march(const oslamk_brick_map &m, const oslamk_wray &b, const float o[3], const float d[3],
                                            float z_min, float z_max)
{
    float tn = z_min, tf = z_max;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = m.origin[a] + (float)(b.r_lo[a] + 1) * m.voxel, hi = m.origin[a] + (float)(b.r_hi[a] - 1) * m.voxel;
        if (!wray_slab(o[a], d[a], lo, hi, &tn, &tf)) return 0.0f;
    }
    if (!(tn <= tf)) return 0.0f;
    const float step = 0.5f * b.mu;
    bool have = false;
    float Fp = 0.0f, tp = 0.0f;
    wray_cache c = {WRAY_NO_KEY, BRK_NONE};
    for (int k = 0; k < OSLAMK_WRAY_MAX_STEPS; k++) {
        const float t = tn + (float)k * step;
        if (!(t <= tf)) break;
        const float x = o[0] + d[0] * t, y = o[1] + d[1] * t, z = o[2] + d[2] * t;
        const uint32_t word = wray_nearest(m, c, (x - m.origin[0]) * m.inv_voxel, (y - m.origin[1]) * m.inv_voxel,
                                           (z - m.origin[2]) * m.inv_voxel);
        if ((word >> 16) == 0u) {
            have = false;
            continue;
        }
        const float F = tsdf_of(word);
        if (have && Fp > 0.0f && F < 0.0f) {
            float Ft, Ftdt;
            if (!wray_trilinear(m, o[0] + d[0] * tp, o[1] + d[1] * tp, o[2] + d[2] * tp, &Ft) || !wray_trilinear(m, x, y, z, &Ftdt))
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

__global__ __launch_bounds__(256) void k_brick_raycast(const oslamk_brick_map m, const oslamk_wray box, const oslamk_view v,
                                                       const oslamk_pose P, float *z_out, float *maps, uint32_t *count)
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
        ts = wray_march(m, box, o, d, v.z_min, v.z_max);
        hit = ts > 0.0f;
        if (hit) {
            const float px = o[0] + d[0] * ts, py = o[1] + d[1] * ts, pz = o[2] + d[2] * ts;
            const float h = m.voxel;
            float x0, x1, y0, y1, z0, z1;
            if (wray_trilinear(m, px + h, py, pz, &x1) && wray_trilinear(m, px - h, py, pz, &x0) &&
                wray_trilinear(m, px, py + h, pz, &y1) && wray_trilinear(m, px, py - h, pz, &y0) &&
                wray_trilinear(m, px, py, pz + h, &z1) && wray_trilinear(m, px, py, pz - h, &z0)) {
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

extern "C" int oslamk_brick_raycast(const oslamk_brick_map *map, const oslamk_wray *box, const oslamk_view *v, const float *T12,
                                    float *z_out, float *maps, uint32_t *count, void *stream)
{
    oslamk_pose P;
    if (!brick_map_ok(map) || !box || !(box->mu > 0.0f) || !v || v->w <= 0 || v->h <= 0 || !T12 || !z_out || !maps || !count)
        return (int)hipErrorInvalidValue;
    for (int a = 0; a < 3; a++)
        if (box->r_hi[a] - box->r_lo[a] < 2) return (int)hipErrorInvalidValue;
    for (int k = 0; k < 12; k++) P.T[k] = T12[k];
    hipLaunchKernelGGL(k_brick_raycast, dim3((v->w + 31) / 32, (v->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *map, *box, *v, P,
                       z_out, maps, count);
    return (int)hipGetLastError();
}
