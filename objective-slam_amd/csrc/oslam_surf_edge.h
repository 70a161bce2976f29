/*
 * oslam_surf_edge.h -- what the surface extraction (oslam_surface.hip: the whole surface and what a shift loses of it)
 * and the mesh extraction (oslam_mesh.hip) share: the shape of a workgroup's run, the "seen" rule and the integer sign test, the crossings of a voxel's three owned
 * edges, the point of a crossing and its normal (include/oslam.h at oslam_volume_surface), the rank of a crossing in
 * its chunk.  Device code, and the check of their launchers.
 */
#ifndef OSLAM_SURF_EDGE_H
#define OSLAM_SURF_EDGE_H

#include <math.h>
#include <stdint.h>

#include "oslam_block_scan.h"
#include "oslam_kernels.h"
#include "oslam_tsdf_read.h"
#include "ppf_math.h"

#define SURF_T OSLAMK_SURF_THREADS
#define SURF_ITEMS OSLAMK_SURF_ITEMS
#define SURF_WAVES (OSLAMK_SURF_THREADS / 64)

static_assert(OSLAMK_SURF_RUN == SURF_T * SURF_ITEMS && SURF_T % 64 == 0, "a run is whole chunks of whole waves");

__device__ __forceinline__ bool surf_seen(uint32_t word, uint32_t min_w) { return (word >> 16) >= min_w; }
__device__ __forceinline__ bool surf_neg(uint32_t word) { return (int16_t)(word & 0xffffu) < 0; }

/* the crossings of the seen voxel idx (word w0) as a mask of axes; ijk = its coordinates, nb[a] = the neighbour's word
 * where bit a is set */
__device__ __forceinline__ uint32_t surf_crossings(const oslamk_volume &vol, uint32_t idx, uint32_t w0, uint32_t min_w, int ijk[3],
                                                   uint32_t nb[3])
{
    const uint32_t nx = (uint32_t)vol.nx, ny = (uint32_t)vol.ny, row = idx / nx;
    const uint32_t stride[3] = {1u, nx, nx * ny};
    const int n[3] = {vol.nx, vol.ny, vol.nz};
    uint32_t mask = 0;
    ijk[0] = (int)(idx - row * nx);
    ijk[1] = (int)(row % ny);
    ijk[2] = (int)(row / ny);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        nb[a] = 0u;
        if (ijk[a] + 1 < n[a]) {
            nb[a] = vol.words[(size_t)idx + stride[a]];
            if (surf_seen(nb[a], min_w) && surf_neg(w0) != surf_neg(nb[a])) mask |= 1u << a;
        }
    }
    return mask;
}

__device__ __forceinline__ uint32_t surf_pick(const uint32_t nb[3], int a) { return a == 0 ? nb[0] : a == 1 ? nb[1] : nb[2]; }

/* the point P of the crossing on axis a of voxel ijk */
__device__ __forceinline__ void surf_position(const oslamk_volume &vol, const int ijk[3], int a, uint32_t w0, uint32_t w1, float P[3])
{
    const float F0 = tsdf_of(w0), F1 = tsdf_of(w1);
    const float t = F0 / (F0 - F1);
    const float h = vol.voxel;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        P[b] = vol.origin[b] + ((float)ijk[b] + 0.5f) * h;
        if (b == a) P[b] = P[b] + t * h;
    }
}

/* the normal at P from six trilinear reads into n; false without a normal */
__device__ __forceinline__ bool surf_normal(const oslamk_volume &vol, const float P[3], float n[3])
{
    const float h = vol.voxel;
    float x0, x1, y0, y1, z0, z1;
    if (!(tsdf_trilinear(vol, P[0] + h, P[1], P[2], &x1) && tsdf_trilinear(vol, P[0] - h, P[1], P[2], &x0) &&
          tsdf_trilinear(vol, P[0], P[1] + h, P[2], &y1) && tsdf_trilinear(vol, P[0], P[1] - h, P[2], &y0) &&
          tsdf_trilinear(vol, P[0], P[1], P[2] + h, &z1) && tsdf_trilinear(vol, P[0], P[1], P[2] - h, &z0)))
        return false;
    const float gx = x1 - x0, gy = y1 - y0, gz = z1 - z0;
    const float len = pm_sqrtf((gx * gx + gy * gy) + gz * gz);
    if (!(len > 0.0f && len <= 3.0e38f)) return false;
    n[0] = gx / len;
    n[1] = gy / len;
    n[2] = gz / len;
    return true;
}

/* the point of the crossing on axis a of voxel ijk and its normal into rec (x y z nx ny nz); false without a normal */
__device__ __forceinline__ bool surf_point(const oslamk_volume &vol, const int ijk[3], int a, uint32_t w0, uint32_t w1, float rec[6])
{
    float P[3], n[3];
    surf_position(vol, ijk, a, w0, w1, P);
    if (!surf_normal(vol, P, n)) return false;
    rec[0] = P[0];
    rec[1] = P[1];
    rec[2] = P[2];
    rec[3] = n[0];
    rec[4] = n[1];
    rec[5] = n[2];
    return true;
}

/* the linear voxel index of a thread's chunk it of its workgroup's run */
__device__ __forceinline__ uint32_t surf_idx(int it) { return blockIdx.x * (uint32_t)OSLAMK_SURF_RUN + (uint32_t)it * SURF_T + threadIdx.x; }

/* a thread's own words of its workgroup's run (0 = unseen past the end of the volume); true when one of them is seen */
__device__ __forceinline__ bool surf_load(const oslamk_volume &vol, uint32_t n_vox, uint32_t min_w, uint32_t w0[SURF_ITEMS])
{
    bool any = false;
#pragma unroll
    for (int it = 0; it < SURF_ITEMS; it++) {
        const uint32_t idx = surf_idx(it);
        w0[it] = idx < n_vox ? vol.words[idx] : 0u;
        any |= surf_seen(w0[it], min_w);
    }
    return any;
}

/* The rank inside its chunk of the thread's first crossing, and *all = the chunk's crossings.  has: the thread's
 * crossings as a mask of axes; the order is voxel, then axis (the mesh's vertex order is the surface's point order by
 * this one rule).  Three ballots, the lower lanes by popcounts, the lower waves through row (block_before: one barrier) */
__device__ __forceinline__ uint32_t surf_chunk_rank(uint32_t has, uint32_t *row, uint32_t *all)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t bx = __ballot(has & 1u), by = __ballot(has & 2u), bz = __ballot(has & 4u);
    const uint32_t before = block_before<SURF_WAVES>((uint32_t)(__popcll(bx) + __popcll(by) + __popcll(bz)), lane == 0, row, all);
    return before + (uint32_t)(__popcll(bx & below) + __popcll(by & below) + __popcll(bz & below));
}

/* the launchers' check of a volume, the "seen" weight and the number of workgroups; *n_vox = the volume's voxels */
static inline bool surf_launch_ok(const oslamk_volume *vol, uint32_t min_w, uint32_t n_groups, uint32_t *n_vox)
{
    if (!(vol && vol->words && oslamk_sides_ok(vol->nx, vol->ny, vol->nz, 0) && vol->voxel > 0.0f && min_w >= 1u && min_w <= 65535u))
        return false;
    *n_vox = (uint32_t)vol->nx * (uint32_t)vol->ny * (uint32_t)vol->nz;          /* at most 2^27: 3 * n_vox fits uint32 */
    return n_groups == oslamk_surface_groups(vol);
}

#endif /* OSLAM_SURF_EDGE_H */
