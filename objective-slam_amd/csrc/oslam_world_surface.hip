/*
 * oslam_world_surface.hip -- the surface of the whole map, voxel store plus window, as points with normals, extracted
 * from sparse 8 x 8 x 8 bricks with no dense box anywhere (semantics: include/oslam.h at oslam_world_surface; host side:
 * oslam_world_surface.c; sums and scans over a workgroup: oslam_block_scan.h; the "seen" rule, the sign test, F, the lerp
 * and the rank of a crossing in its chunk: oslam_surf_edge.h and oslam_tsdf_read.h).  The map on the device is a table
 * of packed brick keys, ascending, with the slot of each entry's brick in an array of [512]-word bricks.
 *
 *   k_brick_window    one workgroup per brick that the window's box overlaps.  One lane finds the brick's slot by binary
 *                     search; every thread then writes the window's word into its two voxels where they lie inside the
 *                     window's box, seen or not, and leaves the others: a brick that store and window share is merged
 *                     voxel by voxel, the window winning.  The window's words never cross the host link.
 *   k_brick_count     one workgroup of 256 threads per table entry, two voxels per thread.  A thread loads its own words
 *                     first; a workgroup none of whose words is seen stores its zero count and returns.  Otherwise 27
 *                     lanes find the slots of the brick and its 26 neighbours (absent = zeros) and the workgroup loads a
 *                     12 x 12 x 12 tile into LDS: the brick with a halo of 2, because P +- voxel puts a trilinear base
 *                     between i - 2 and i + 1 in exact arithmetic when t < 1.  A base outside the tile (t = 1 exactly, a
 *                     stored zero at the edge's far end, gives i + 2; far from the origin float rounding moves a base by
 *                     one) is read through the table instead (map_word), never outside LDS.  The entry's number of
 *                     points goes to counts[blockIdx.x], the crossings are added as integers to totals[0].  The counts
 *                     are scanned by oslamk_surface_scan in chunks of 2^17 entries, each chunk's sum to totals[2 + c].
 *   k_brick_emit      recomputes.  The rank of a point is its rank in the chunk of 256 voxels (surf_chunk_rank: voxel
 *                     order, then axis) plus the points of the first chunk, plus the entry's offset and its scan chunk's
 *                     base: entries ascend by key (bz, by, bx), inside one 3 * (i + 8 * (j + 8 * k)) + a.
 * Bounds.  A table index is below n by the grid and checked again; a slot is checked against n before any load or store
 * through it; a tile index is checked against the tile before every LDS read; a window index is checked against the
 * volume's sides before its load; a rank is checked against the number of points before its stores.  The launchers check
 * the map, the "seen" weight, the anchor and the window's brick box.  No scratch, no float atomics; registers, LDS and
 * occupancy: profiles/r26_kernel_resources_world_surface.txt.
 */
#include <hip/hip_runtime.h>

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

/* the slot of the brick with this key, BRK_NONE without one */
__device__ __forceinline__ uint32_t brick_find(const oslamk_brick_map &m, uint64_t key)
{
    uint32_t lo = 0, hi = m.n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (m.keys[mid] < key) lo = mid + 1; else hi = mid;
    }
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

/* surf_point against the map: the point of the crossing on axis a of the voxel with index r = g - anchor and its normal
 * into rec (x y z nx ny nz); false without a normal.  The float sequence is surf_position's and surf_normal's */
__device__ __forceinline__ bool brick_point(const oslamk_brick_map &m, const uint32_t *tile, const int tg[3], const int r[3], int a,
                                            uint32_t w0, uint32_t w1, float rec[6])
{
    const float F0 = tsdf_of(w0), F1 = tsdf_of(w1);
    const float t = F0 / (F0 - F1);
    const float h = m.voxel;
    float P[3], x0, x1, y0, y1, z0, z1;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        P[b] = m.origin[b] + ((float)r[b] + 0.5f) * h;
        if (b == a) P[b] = P[b] + t * h;
    }
    if (!(brick_trilinear(m, tile, tg, P[0] + h, P[1], P[2], &x1) && brick_trilinear(m, tile, tg, P[0] - h, P[1], P[2], &x0) &&
          brick_trilinear(m, tile, tg, P[0], P[1] + h, P[2], &y1) && brick_trilinear(m, tile, tg, P[0], P[1] - h, P[2], &y0) &&
          brick_trilinear(m, tile, tg, P[0], P[1], P[2] + h, &z1) && brick_trilinear(m, tile, tg, P[0], P[1], P[2] - h, &z0)))
        return false;
    const float gx = x1 - x0, gy = y1 - y0, gz = z1 - z0;
    const float len = pm_sqrtf((gx * gx + gy * gy) + gz * gz);
    if (!(len > 0.0f && len <= 3.0e38f)) return false;
    rec[0] = P[0];
    rec[1] = P[1];
    rec[2] = P[2];
    rec[3] = gx / len;
    rec[4] = gy / len;
    rec[5] = gz / len;
    return true;
}

/* The two passes.  EMIT false: counts[e] = the entry's points, totals[0] += its crossings.  EMIT true: the records to
 * their ranks from offsets[e] + base */
template <bool EMIT>
__device__ __forceinline__ void brick_pass(const oslamk_brick_map &m, uint32_t min_w, uint32_t *counts, uint32_t *totals,
                                           const uint32_t *offsets, uint32_t base, uint32_t n_points, float *out6, int32_t *key_out)
{
    __shared__ uint32_t s_tile[BRK_TILE_WORDS];
    __shared__ uint32_t s_nb[27];
    __shared__ uint32_t s_cnt[BRK_ITEMS][SURF_WAVES];
    const uint32_t e = blockIdx.x, tid = threadIdx.x;
    if (e >= m.n) return;
    const uint64_t key = m.keys[e];
    const uint32_t own = m.slots[e] < m.n ? m.slots[e] : BRK_NONE;
    uint32_t w0[BRK_ITEMS];
    bool any = false;
#pragma unroll
    for (int it = 0; it < BRK_ITEMS; it++) {
        w0[it] = own != BRK_NONE ? m.words[(size_t)own * OSLAMK_BRICK_WORDS + (uint32_t)it * BRK_T + tid] : 0u;
        any |= surf_seen(w0[it], min_w);
    }
    if (!__syncthreads_or(any)) {
        if (!EMIT && tid == 0) counts[e] = 0u;
        return;
    }
    const int kb[3] = {(int)(key & 0x1fffffu) - OSLAMK_BRICK_BIAS, (int)(key >> 21 & 0x1fffffu) - OSLAMK_BRICK_BIAS,
                       (int)(key >> 42 & 0x1fffffu) - OSLAMK_BRICK_BIAS};
    if (tid < 27u) {
        const int dx = (int)(tid % 3u) - 1, dy = (int)(tid / 3u % 3u) - 1, dz = (int)(tid / 9u) - 1;
        s_nb[tid] = tid == 13u ? own : brick_find(m, OSLAMK_BRICK_KEY(kb[0] + dx, kb[1] + dy, kb[2] + dz));
    }
    __syncthreads();
    for (uint32_t t = tid; t < (uint32_t)BRK_TILE_WORDS; t += BRK_T) {
        const int cx = (int)(t % BRK_TILE) - BRK_HALO, cy = (int)(t / BRK_TILE % BRK_TILE) - BRK_HALO, cz = (int)(t / (BRK_TILE * BRK_TILE)) - BRK_HALO;
        const uint32_t slot = s_nb[((cx + 8) >> 3) + 3 * ((cy + 8) >> 3) + 9 * ((cz + 8) >> 3)];           /* c in -2 .. 9 */
        s_tile[t] = slot < m.n ? m.words[(size_t)slot * OSLAMK_BRICK_WORDS + brick_local(cx, cy, cz)] : 0u;
    }
    __syncthreads();
    const int g0[3] = {kb[0] * OSLAMK_BRICK_SIDE, kb[1] * OSLAMK_BRICK_SIDE, kb[2] * OSLAMK_BRICK_SIDE};
    const int tg[3] = {g0[0] - BRK_HALO, g0[1] - BRK_HALO, g0[2] - BRK_HALO};
    const uint32_t stride[3] = {1u, BRK_TILE, BRK_TILE * BRK_TILE};
    uint32_t run = EMIT ? offsets[e] + base : 0u, pts = 0, cross = 0;
    for (int it = 0; it < BRK_ITEMS; it++) {
        const uint32_t l = (uint32_t)it * BRK_T + tid;
        const int ijk[3] = {(int)(l & 7u), (int)(l >> 3 & 7u), (int)(l >> 6)};
        const int g[3] = {g0[0] + ijk[0], g0[1] + ijk[1], g0[2] + ijk[2]};
        const int r[3] = {g[0] - m.anchor[0], g[1] - m.anchor[1], g[2] - m.anchor[2]};
        const uint32_t p = (uint32_t)(((ijk[2] + BRK_HALO) * BRK_TILE + ijk[1] + BRK_HALO) * BRK_TILE + ijk[0] + BRK_HALO);
        uint32_t nb[3] = {0u, 0u, 0u}, mask = 0;
        if (surf_seen(w0[it], min_w)) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                nb[a] = tile_at(s_tile, p + stride[a]);
                if (surf_seen(nb[a], min_w) && surf_neg(w0[it]) != surf_neg(nb[a])) mask |= 1u << a;
            }
        }
        if (!EMIT) {
            cross += (uint32_t)__popc(mask);
#pragma unroll 1
            for (int a = 0; a < 3; a++) {
                float rec[6];
                if ((mask >> a & 1u) && brick_point(m, s_tile, tg, r, a, w0[it], surf_pick(nb, a), rec)) pts++;
            }
        } else {
            float rec[3][6] = {};
            uint32_t has = 0, all;
            /* one axis at a time, as in k_surface_emit; the record goes to its row by selects */
#pragma unroll 1
            for (int a = 0; a < 3; a++) {
                float q[6];
                if (!((mask >> a & 1u) && brick_point(m, s_tile, tg, r, a, w0[it], surf_pick(nb, a), q))) continue;
                has |= 1u << a;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    rec[0][c] = a == 0 ? q[c] : rec[0][c];
                    rec[1][c] = a == 1 ? q[c] : rec[1][c];
                    rec[2][c] = a == 2 ? q[c] : rec[2][c];
                }
            }
            uint32_t rank = run + surf_chunk_rank(has, s_cnt[it], &all);
#pragma unroll
            for (int a = 0; a < 3; a++)
                if (has >> a & 1u) {
                    if (rank < n_points) {
                        float2 *dst = reinterpret_cast<float2 *>(out6 + (size_t)rank * 6);
                        dst[0] = make_float2(rec[a][0], rec[a][1]);
                        dst[1] = make_float2(rec[a][2], rec[a][3]);
                        dst[2] = make_float2(rec[a][4], rec[a][5]);
                        if (key_out) reinterpret_cast<int4 *>(key_out)[rank] = make_int4(g[0], g[1], g[2], a);
                    }
                    rank++;
                }
            run += all;
        }
    }
    if (!EMIT) {
        cross = wave_sum(cross);
        if ((tid & 63u) == 0 && cross) atomicAdd(totals, cross);
        pts = block_sum<SURF_WAVES>(pts, s_cnt[0]);
        if (tid == 0) counts[e] = pts;
    }
}

__global__ __launch_bounds__(BRK_T) void k_brick_count(const oslamk_brick_map m, uint32_t min_w, uint32_t *counts, uint32_t *totals)
{
    brick_pass<false>(m, min_w, counts, totals, nullptr, 0u, 0u, nullptr, nullptr);
}

__global__ __launch_bounds__(BRK_T) void k_brick_emit(const oslamk_brick_map m, uint32_t min_w, const uint32_t *offsets,
                                                      const oslamk_brick_bases bases, uint32_t n_points, float *out6, int32_t *key_out)
{
    brick_pass<true>(m, min_w, nullptr, nullptr, offsets, bases.base[blockIdx.x / OSLAMK_BRICK_SCAN % OSLAMK_BRICK_CHUNKS], n_points, out6,
                     key_out);
}

__global__ __launch_bounds__(BRK_T) void k_brick_window(const oslamk_brick_map m, const oslamk_volume vol, const oslamk_shift3 off,
                                                        const oslamk_shift3 kb0, const oslamk_shift3 nb)
{
    __shared__ uint32_t s_slot;
    const uint32_t e = blockIdx.x, nb0 = (uint32_t)nb.s[0], nb1 = (uint32_t)nb.s[1];
    const int bx = kb0.s[0] + (int)(e % nb0), by = kb0.s[1] + (int)(e / nb0 % nb1), bz = kb0.s[2] + (int)(e / (nb0 * nb1));
    if (threadIdx.x == 0) s_slot = brick_find(m, OSLAMK_BRICK_KEY(bx, by, bz));
    __syncthreads();
    const uint32_t slot = s_slot;
    if (slot >= m.n || bz >= kb0.s[2] + nb.s[2]) return;
#pragma unroll
    for (int it = 0; it < BRK_ITEMS; it++) {
        const uint32_t l = (uint32_t)it * BRK_T + threadIdx.x;
        const int cx = bx * OSLAMK_BRICK_SIDE + (int)(l & 7u) - off.s[0], cy = by * OSLAMK_BRICK_SIDE + (int)(l >> 3 & 7u) - off.s[1],
                  cz = bz * OSLAMK_BRICK_SIDE + (int)(l >> 6) - off.s[2];
        if ((unsigned)cx < (unsigned)vol.nx && (unsigned)cy < (unsigned)vol.ny && (unsigned)cz < (unsigned)vol.nz)
            m.words[(size_t)slot * OSLAMK_BRICK_WORDS + l] = vol.words[((size_t)cz * vol.ny + (size_t)cy) * vol.nx + (size_t)cx];
    }
}

static bool brick_map_ok(const oslamk_brick_map *m)
{
    return m && m->keys && m->slots && m->words && m->n >= 1u && m->n <= OSLAMK_BRICK_MAX && m->voxel > 0.0f && oslamk_shift_ok(m->anchor);
}

extern "C" int oslamk_brick_window(const oslamk_brick_map *map, const oslamk_volume *vol, const int off[3], const int kb0[3],
                                   const int nb[3], void *stream)
{
    if (!brick_map_ok(map) || !vol || !vol->words || !oslamk_sides_ok(vol->nx, vol->ny, vol->nz, 0) || !off || !kb0 || !nb || !oslamk_shift_ok(off))
        return (int)hipErrorInvalidValue;
    const int n[3] = {vol->nx, vol->ny, vol->nz};
    for (int a = 0; a < 3; a++)
        if (kb0[a] != off[a] >> 3 || nb[a] != ((off[a] + n[a] - 1) >> 3) - kb0[a] + 1) return (int)hipErrorInvalidValue;
    const oslamk_shift3 o = {{off[0], off[1], off[2]}}, k = {{kb0[0], kb0[1], kb0[2]}}, b = {{nb[0], nb[1], nb[2]}};
    hipLaunchKernelGGL(k_brick_window, dim3((uint32_t)(nb[0] * nb[1] * nb[2])), dim3(BRK_T), 0, (hipStream_t)stream, *map, *vol, o, k, b);
    return (int)hipGetLastError();
}

extern "C" int oslamk_brick_count(const oslamk_brick_map *map, uint32_t min_weight, uint32_t *counts, uint32_t *totals, void *stream)
{
    if (!brick_map_ok(map) || min_weight < 1u || min_weight > 65535u || !counts || !totals) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_brick_count, dim3(map->n), dim3(BRK_T), 0, (hipStream_t)stream, *map, min_weight, counts, totals);
    hipError_t e = hipGetLastError();
    for (uint32_t c = 0; e == hipSuccess && c * OSLAMK_BRICK_SCAN < map->n; c++) {
        const uint32_t left = map->n - c * OSLAMK_BRICK_SCAN;
        e = (hipError_t)oslamk_surface_scan(counts + (size_t)c * OSLAMK_BRICK_SCAN, left < OSLAMK_BRICK_SCAN ? left : OSLAMK_BRICK_SCAN,
                                            totals + 2 + c, stream);
    }
    return (int)e;
}

extern "C" int oslamk_brick_emit(const oslamk_brick_map *map, uint32_t min_weight, const uint32_t *offsets, const oslamk_brick_bases *bases,
                                 uint32_t n_points, float *out6, int32_t *key_out, void *stream)
{
    if (!brick_map_ok(map) || min_weight < 1u || min_weight > 65535u || !offsets || !bases || !out6 || n_points == 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_brick_emit, dim3(map->n), dim3(BRK_T), 0, (hipStream_t)stream, *map, min_weight, offsets, *bases, n_points, out6,
                       key_out);
    return (int)hipGetLastError();
}
