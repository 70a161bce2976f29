/*
 * oslam_depth_normal.h -- the point and the normal of one depth pixel (include/oslam.h at oslam_depth_to_cloud;
 * the statement is oracle/oracle_depth.c), the one source of k_depth_points (oslam_depth.hip: the scene cloud) and
 * k_view_normals (oslam_track.hip: the vertex and normal maps of a view).  Device code only.
 */
#ifndef OSLAM_DEPTH_NORMAL_H
#define OSLAM_DEPTH_NORMAL_H

#include <hip/hip_runtime.h>

#include "ppf_math.h"

struct depth_cam {
    float fx, fy, cx, cy, scale, z_min, z_max, max_jump;
};

__device__ __forceinline__ bool depth_ok(float z, const depth_cam &c) { return z >= c.z_min && z <= c.z_max; }
__device__ __forceinline__ void back_project(int u, int v, float z, const depth_cam &c, float p[3])
{
    p[0] = (((float)u - c.cx) * z) / c.fx;
    p[1] = (((float)v - c.cy) * z) / c.fy;
    p[2] = z;
}

/* pixel (u, v) with depth z and its left, right, upper and lower neighbours' depths, all five valid: false when a
 * neighbour lies farther than max_jump from z or the cross product is zero or not finite; otherwise p and the unit
 * normal n, turned to face the camera */
__device__ __forceinline__ bool depth_point_normal(int u, int v, float z, float zl, float zr, float zu, float zd,
                                                   const depth_cam &c, float p[3], float n[3])
{
    if (!(pm_fabsf(zl - z) <= c.max_jump && pm_fabsf(zr - z) <= c.max_jump && pm_fabsf(zu - z) <= c.max_jump &&
          pm_fabsf(zd - z) <= c.max_jump))
        return false;
    float pl[3], pr[3], pu[3], pd[3];
    back_project(u, v, z, c, p);
    back_project(u - 1, v, zl, c, pl);
    back_project(u + 1, v, zr, c, pr);
    back_project(u, v - 1, zu, c, pu);
    back_project(u, v + 1, zd, c, pd);
    const float ax = pr[0] - pl[0], ay = pr[1] - pl[1], az = pr[2] - pl[2];
    const float bx = pd[0] - pu[0], by = pd[1] - pu[1], bz = pd[2] - pu[2];
    float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = pm_sqrtf(nx * nx + ny * ny + nz * nz);
    if (!(len > 0.0f && len <= 3.0e38f)) return false;
    nx = nx / len;
    ny = ny / len;
    nz = nz / len;
    if (nx * p[0] + ny * p[1] + nz * p[2] > 0.0f) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    n[0] = nx;
    n[1] = ny;
    n[2] = nz;
    return true;
}

#endif /* OSLAM_DEPTH_NORMAL_H */
