/*
 * oslam_tsdf_read.h -- the reads of a TSDF volume that the ray cast (oslam_volume.hip) and the surface extraction
 * (oslam_surface.hip) share: the F of a word and the trilinear F at a volume-frame point (include/oslam.h at
 * oslam_volume_raycast).  Device code only.
 */
#ifndef OSLAM_TSDF_READ_H
#define OSLAM_TSDF_READ_H

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"

__device__ __forceinline__ float tsdf_of(uint32_t word) { return (float)(int16_t)(word & 0xffffu) / 32767.0f; }

__device__ __forceinline__ float tsdf_lerp(float a, float b, float f) { return a * (1.0f - f) + b * f; }

/* the trilinear F at the volume-frame point (x, y, z); false when a corner lies outside the volume or has w = 0 */
__device__ __forceinline__ bool tsdf_trilinear(const oslamk_volume &vol, float x, float y, float z, float *out)
{
    const float gx = (x - vol.origin[0]) * vol.inv_voxel - 0.5f;
    const float gy = (y - vol.origin[1]) * vol.inv_voxel - 0.5f;
    const float gz = (z - vol.origin[2]) * vol.inv_voxel - 0.5f;
    const float bx = floorf(gx), by = floorf(gy), bz = floorf(gz);
    if (!(bx >= 0.0f && bx <= (float)(vol.nx - 2) && by >= 0.0f && by <= (float)(vol.ny - 2) && bz >= 0.0f &&
          bz <= (float)(vol.nz - 2)))
        return false;
    const float fx = gx - bx, fy = gy - by, fz = gz - bz;
    const size_t sx = 1, sy = (size_t)vol.nx, sz = (size_t)vol.nx * vol.ny;
    const uint32_t *p = vol.words + ((size_t)(int)bz * vol.ny + (size_t)(int)by) * vol.nx + (size_t)(int)bx;
    const uint32_t w000 = p[0], w100 = p[sx], w010 = p[sy], w110 = p[sy + sx];
    const uint32_t w001 = p[sz], w101 = p[sz + sx], w011 = p[sz + sy], w111 = p[sz + sy + sx];
    if (!((w000 >> 16) && (w100 >> 16) && (w010 >> 16) && (w110 >> 16) && (w001 >> 16) && (w101 >> 16) && (w011 >> 16) &&
          (w111 >> 16)))
        return false;
    const float c00 = tsdf_lerp(tsdf_of(w000), tsdf_of(w100), fx), c10 = tsdf_lerp(tsdf_of(w010), tsdf_of(w110), fx);
    const float c01 = tsdf_lerp(tsdf_of(w001), tsdf_of(w101), fx), c11 = tsdf_lerp(tsdf_of(w011), tsdf_of(w111), fx);
    *out = tsdf_lerp(tsdf_lerp(c00, c10, fy), tsdf_lerp(c01, c11, fy), fz);
    return true;
}

#endif /* OSLAM_TSDF_READ_H */
