/*
 * oslam_icp_core.h -- what the refinement, verification, tracking and camera motion kernels do around the step of
 * oslam_refine_step.h, each piece once.  Device code only; every float sequence here is pinned bit for bit by the
 * sums="f32" restatements of the tests (the units are built with -ffp-contract=off: keep the expression trees).
 *
 *   oslam_icp_transform    q = R p + t and m = R n under the float32 pose (rows of [R | t])
 *   oslam_icp_project      the pixel of q in a view: the z range, the rounding, the range check in float before the
 *                          cast
 *   oslam_icp_gate         a projective correspondence: the pixel's vertex record, has-normal, distance, then its
 *                          normal record and the normal agreement
 *   oslam_icp_block_sums   the fixed-order sum over a workgroup: the wave64 shuffle tree, then the waves in index order
 *                          through an LDS buffer of the caller (one barrier)
 */
#ifndef OSLAM_ICP_CORE_H
#define OSLAM_ICP_CORE_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"

__device__ __forceinline__ void oslam_icp_transform(const float *T, float px, float py, float pz, float nx, float ny,
                                                    float nz, float q[3], float m[3])
{
#pragma unroll
    for (int a = 0; a < 3; a++) {
        q[a] = ((T[4 * a] * px + T[4 * a + 1] * py) + T[4 * a + 2] * pz) + T[4 * a + 3];
        m[a] = (T[4 * a] * nx + T[4 * a + 1] * ny) + T[4 * a + 2] * nz;
    }
}

/* false: q lies outside the view's z range or projects outside the image; otherwise (*u, *vv) lies inside it */
__device__ __forceinline__ bool oslam_icp_project(const oslamk_view &v, const float q[3], int *u, int *vv)
{
    if (!(q[2] >= v.z_min && q[2] <= v.z_max)) return false;
    const float fu = floorf(((q[0] * v.fx) / q[2] + v.cx) + 0.5f);
    const float fv = floorf(((q[1] * v.fy) / q[2] + v.cy) + 0.5f);
    if (!(fu >= 0.0f && fu < (float)v.w && fv >= 0.0f && fv < (float)v.h)) return false;
    *u = (int)fu;
    *vv = (int)fv;
    return true;
}

/* pix: a pixel inside the maps.  true: *a and *b = its vertex and normal records; b is not loaded when the distance
 * gate fails */
__device__ __forceinline__ bool oslam_icp_gate(const float4 *maps, int pix, const float q[3], const float m[3],
                                               float r2, float min_dot, float4 *a_out, float4 *b_out)
{
    const float4 a = maps[2 * (size_t)pix];
    if (a.w == 0.0f) return false;                 /* the pixel has no normal */
    const float dx = a.x - q[0], dy = a.y - q[1], dz = a.z - q[2];
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(d2 <= r2)) return false;
    const float4 b = maps[2 * (size_t)pix + 1];
    const float dot = (m[0] * b.x + m[1] * b.y) + m[2] * b.z;
    if (!(dot >= min_dot)) return false;
    *a_out = a;
    *b_out = b;
    return true;
}

/* s[0 .. NS), NS <= NC, are summed over each wave by a shuffle tree, the same for every term; lane 0 of wave w stores
 * s[0 .. NC) as row w of sh (the columns from NS on as its lane 0 holds them); a barrier; thread k < NC returns column
 * k summed over the waves in index order, the others 0.  Every thread of the workgroup calls it, the same number of
 * times; sh is the caller's (two of them taken in turn make one barrier per call enough). */
template <int NS, int NW, int NC>
__device__ __forceinline__ float oslam_icp_block_sums(float (&s)[NC], float (&sh)[NW][NC])
{
    static_assert(NS <= NC, "the summed terms are columns of the row");
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; k++) {
        float v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        s[k] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NC; k++) sh[tid >> 6][k] = s[k];
    }
    __syncthreads();
    if (tid >= NC) return 0.0f;
    float x = sh[0][tid];
#pragma unroll
    for (int w = 1; w < NW; w++) x += sh[w][tid];
    return x;
}

#endif /* OSLAM_ICP_CORE_H */
