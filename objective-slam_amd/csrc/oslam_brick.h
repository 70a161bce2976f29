/*
 * oslam_brick.h -- what the extractions from sparse 8 x 8 x 8 bricks share (oslam_world_surface.hip: the whole map's
 * surface; oslam_world_mesh.hip: its mesh): the shape of a workgroup, the search of the brick table, the 12 x 12 x 12
 * tile in LDS and its load, the trilinear read against tile and table, the point of a crossing and its normal
 * (include/oslam.h at oslam_world_surface).  Device code, and the check of their launchers.
 */
#ifndef OSLAM_BRICK_H
#define OSLAM_BRICK_H

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"
#include "oslam_surf_edge.h"

#define BRK_T SURF_T
#define BRK_ITEMS 2
#define BRK_TILE 12
#define BRK_TILE_WORDS (BRK_TILE * BRK_TILE * BRK_TILE)
#define BRK_HALO 2
#define BRK_NONE 0xffffffffu
#define BRK_COORD_MAX 4194304.0f      /* 2^22: a trilinear base is an index only below it */

static_assert(BRK_T * BRK_ITEMS == OSLAMK_BRICK_WORDS && BRK_T == 256, "a workgroup owns one brick, two voxels per thread");

/* the first table entry whose key is not below this one; m.n when there is none */
__device__ __forceinline__ uint32_t brick_lower(const oslamk_brick_map &m, uint64_t key)
{
    uint32_t lo = 0, hi = m.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (m.keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* the table entry of the brick with this key, BRK_NONE without one */
__device__ __forceinline__ uint32_t brick_find_entry(const oslamk_brick_map &m, uint64_t key)
{
    const uint32_t lo = brick_lower(m, key);
    return lo < m.n && m.keys[lo] == key ? lo : BRK_NONE;
}

/* the slot of the brick with this key, BRK_NONE without one */
__device__ __forceinline__ uint32_t brick_find(const oslamk_brick_map &m, uint64_t key)
{
    const uint32_t lo = brick_lower(m, key);
    if (lo >= m.n || m.keys[lo] != key) return BRK_NONE;
    const uint32_t slot = m.slots[lo];
    return slot < m.n ? slot : BRK_NONE;
}

__device__ __forceinline__ uint32_t brick_local(int x, int y, int z) { return (uint32_t)((((z & 7) * 8) + (y & 7)) * 8 + (x & 7)); }

/* G at the global voxel g through the table, |g_a| < 2^23: the read of a trilinear corner that lies outside the tile */
__device__ __forceinline__ uint32_t map_word(const oslamk_brick_map &m, int gx, int gy, int gz)
{
    const uint32_t slot = brick_find(m, OSLAMK_BRICK_KEY(gx >> 3, gy >> 3, gz >> 3));
    return slot == BRK_NONE ? 0u : m.words[(size_t)slot * OSLAMK_BRICK_WORDS + brick_local(gx, gy, gz)];
}

__device__ __forceinline__ uint32_t tile_at(const uint32_t *tile, uint32_t t) { return t < (uint32_t)BRK_TILE_WORDS ? tile[t] : 0u; }

/* the brick coordinates of a packed key */
__device__ __forceinline__ void brick_coords(uint64_t key, int kb[3])
{
    kb[0] = (int)(key & 0x1fffffu) - OSLAMK_BRICK_BIAS;
    kb[1] = (int)(key >> 21 & 0x1fffffu) - OSLAMK_BRICK_BIAS;
    kb[2] = (int)(key >> 42 & 0x1fffffu) - OSLAMK_BRICK_BIAS;
}

/* The tile of the brick kb (slot own, or BRK_NONE) for thread tid: 27 lanes find the slots of the brick and its 26
 * neighbours into nb [27] (absent = BRK_NONE, read as zeros), then the workgroup loads the brick with a halo of 2 into
 * tile [BRK_TILE_WORDS].  Every thread of the workgroup runs it; it holds two barriers, the second after the load.  A
 * macro: as a function, forced inline or not, it makes the compiler allocate the registers of k_brick_count and
 * k_brick_emit differently, and their object is to stay what it was byte for byte */
#define BRICK_TILE_LOAD(m, kb, own, tid, nb, tile)                                                                          \
    do {                                                                                                                    \
        if ((tid) < 27u) {                                                                                                  \
            const int dx = (int)((tid) % 3u) - 1, dy = (int)((tid) / 3u % 3u) - 1, dz = (int)((tid) / 9u) - 1;              \
            (nb)[tid] = (tid) == 13u ? (own) : brick_find(m, OSLAMK_BRICK_KEY((kb)[0] + dx, (kb)[1] + dy, (kb)[2] + dz));   \
        }                                                                                                                   \
        __syncthreads();                                                                                                    \
        for (uint32_t t = (tid); t < (uint32_t)BRK_TILE_WORDS; t += BRK_T) {                                                \
            const int cx = (int)(t % BRK_TILE) - BRK_HALO, cy = (int)(t / BRK_TILE % BRK_TILE) - BRK_HALO,                  \
                      cz = (int)(t / (BRK_TILE * BRK_TILE)) - BRK_HALO;                           /* c in -2 .. 9 */        \
            const uint32_t slot = (nb)[((cx + 8) >> 3) + 3 * ((cy + 8) >> 3) + 9 * ((cz + 8) >> 3)];                        \
            (tile)[t] = slot < (m).n ? (m).words[(size_t)slot * OSLAMK_BRICK_WORDS + brick_local(cx, cy, cz)] : 0u;         \
        }                                                                                                                   \
        __syncthreads();                                                                                                    \
    } while (0)

/* tsdf_trilinear against the map: the volume-frame point in the frame of m, the base's range test "finite and below
 * 2^22 in size", the eight corners from the tile (origin tg = the global voxel of tile index 0) or, where the base lies
 * outside it, through the table; the arithmetic is tsdf_trilinear's, grouping unchanged */
__device__ __forceinline__ bool brick_trilinear(const oslamk_brick_map &m, const uint32_t *tile, const int tg[3], float x, float y,
                                                float z, float *out)
{
    const float gx = (x - m.origin[0]) * m.inv_voxel - 0.5f;
    const float gy = (y - m.origin[1]) * m.inv_voxel - 0.5f;
    const float gz = (z - m.origin[2]) * m.inv_voxel - 0.5f;
    const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
    if (!(fabsf(bx) < BRK_COORD_MAX && fabsf(by) < BRK_COORD_MAX && fabsf(bz) < BRK_COORD_MAX)) return false;
    const float fx = gx - bx, fy = gy - by, fz = gz - bz;
    const int cx = m.anchor[0] + (int)bx, cy = m.anchor[1] + (int)by, cz = m.anchor[2] + (int)bz;     /* below 2^23 in size */
    const int tx = cx - tg[0], ty = cy - tg[1], tz = cz - tg[2];
    uint32_t w000, w100, w010, w110, w001, w101, w011, w111;
    if ((unsigned)tx <= (unsigned)(BRK_TILE - 2) && (unsigned)ty <= (unsigned)(BRK_TILE - 2) && (unsigned)tz <= (unsigned)(BRK_TILE - 2)) {
        const uint32_t p = (uint32_t)((tz * BRK_TILE + ty) * BRK_TILE + tx);
        const uint32_t sy = BRK_TILE, sz = BRK_TILE * BRK_TILE;
        w000 = tile_at(tile, p), w100 = tile_at(tile, p + 1), w010 = tile_at(tile, p + sy), w110 = tile_at(tile, p + sy + 1);
        w001 = tile_at(tile, p + sz), w101 = tile_at(tile, p + sz + 1), w011 = tile_at(tile, p + sz + sy), w111 = tile_at(tile, p + sz + sy + 1);
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

/* surf_position against the map: the point P of the crossing on axis a of the voxel with index r = g - anchor */
__device__ __forceinline__ void brick_position(const oslamk_brick_map &m, const int r[3], int a, uint32_t w0, uint32_t w1, float P[3])
{
    const float F0 = tsdf_of(w0), F1 = tsdf_of(w1);
    const float t = F0 / (F0 - F1);
    const float h = m.voxel;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        P[b] = m.origin[b] + ((float)r[b] + 0.5f) * h;
        if (b == a) P[b] = P[b] + t * h;
    }
}

/* surf_normal against the map: the normal at P from six trilinear reads into n; false without a normal */
__device__ __forceinline__ bool brick_normal(const oslamk_brick_map &m, const uint32_t *tile, const int tg[3], const float P[3], float n[3])
{
    const float h = m.voxel;
    float x0, x1, y0, y1, z0, z1;
    if (!(brick_trilinear(m, tile, tg, P[0] + h, P[1], P[2], &x1) && brick_trilinear(m, tile, tg, P[0] - h, P[1], P[2], &x0) &&
          brick_trilinear(m, tile, tg, P[0], P[1] + h, P[2], &y1) && brick_trilinear(m, tile, tg, P[0], P[1] - h, P[2], &y0) &&
          brick_trilinear(m, tile, tg, P[0], P[1], P[2] + h, &z1) && brick_trilinear(m, tile, tg, P[0], P[1], P[2] - h, &z0)))
        return false;
    const float gx = x1 - x0, gy = y1 - y0, gz = z1 - z0;
    const float len = pm_sqrtf((gx * gx + gy * gy) + gz * gz);
    if (!(len > 0.0f && len <= 3.0e38f)) return false;
    n[0] = gx / len;
    n[1] = gy / len;
    n[2] = gz / len;
    return true;
}

/* surf_point against the map: the point of the crossing and its normal into rec (x y z nx ny nz); false without a
 * normal.  The float sequence is surf_position's and surf_normal's */
__device__ __forceinline__ bool brick_point(const oslamk_brick_map &m, const uint32_t *tile, const int tg[3], const int r[3], int a,
                                            uint32_t w0, uint32_t w1, float rec[6])
{
    float P[3], n[3];
    brick_position(m, r, a, w0, w1, P);
    if (!brick_normal(m, tile, tg, P, n)) return false;
    rec[0] = P[0];
    rec[1] = P[1];
    rec[2] = P[2];
    rec[3] = n[0];
    rec[4] = n[1];
    rec[5] = n[2];
    return true;
}

/* the launchers' check of a map */
static inline bool brick_map_ok(const oslamk_brick_map *m)
{
    return m && m->keys && m->slots && m->words && m->n >= 1u && m->n <= OSLAMK_BRICK_MAX && m->voxel > 0.0f && oslamk_shift_ok(m->anchor);
}

#endif /* OSLAM_BRICK_H */
