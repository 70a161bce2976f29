/*
 * oslam_world_surface.hip -- the surface of the whole map, voxel store plus window, as points with normals, extracted
 * from sparse 8 x 8 x 8 bricks with no dense box anywhere (semantics: include/oslam.h at oslam_world_surface; host side:
 * oslam_world_surface.c; sums and scans over a workgroup: oslam_block_scan.h; the "seen" rule, the sign test, F, the lerp
 * and the rank of a crossing in its chunk: oslam_surf_edge.h and oslam_tsdf_read.h; the search of the table, the tile and
 * its load, the trilinear read and the point of a crossing, shared with the map's mesh: oslam_brick.h).  The map on the device is a table
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

#include "oslam_brick.h"
#include "oslam_kernels.h"
#include "oslam_surf_edge.h"

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
    int kb[3];
    brick_coords(key, kb);
    BRICK_TILE_LOAD(m, kb, own, tid, s_nb, s_tile);
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
