/*
 * oslam_verify_class.h -- the class of one model point against a view (include/oslam.h at oslam_verify), the one
 * source of k_verify (oslam_verify.hip) and k_claim (oslam_arbitrate.hip).  Device code only.
 *
 * RESID = false is k_verify's body.  RESID = true also returns what a claim needs: the point's pixel (valid for the
 * classes 2..5) and the smallest fabsf(z_o - p'z) over the valid pixels of its window (INFINITY without one; <= tol
 * exactly when the class is SUPPORTED).  The class does not depend on RESID: the extra minimum reads the same
 * differences the SUPPORTED test reads.
 * Bounds: a point reads at most (2 window + 1)^2 <= 49 floats of the z image, all inside it (the window is clipped);
 * the pixel is range-checked in float before it becomes an int.
 */
#ifndef OSLAM_VERIFY_CLASS_H
#define OSLAM_VERIFY_CLASS_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"

/* point i of member d (i < d->m.n) -> 0 BACK .. 5 UNKNOWN */
template <bool RESID>
__device__ __forceinline__ int oslam_verify_class(const oslamk_view &v, const oslamk_verify_member *d, int i, int window,
                                                  int *u_out, int *v_out, float *resid_out)
{
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = d->T[k];
    const float px = d->m.px[i], py = d->m.py[i], pz = d->m.pz[i];
    const float nx = d->m.nx[i], ny = d->m.ny[i], nz = d->m.nz[i];
    const float qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const float qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const float qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    const float mx = (T[0] * nx + T[1] * ny) + T[2] * nz;
    const float my = (T[4] * nx + T[5] * ny) + T[6] * nz;
    const float mz = (T[8] * nx + T[9] * ny) + T[10] * nz;
    if ((mx * qx + my * qy) + mz * qz >= 0.0f) return 0;               /* BACK */
    bool in = qz >= v.z_min && qz <= v.z_max;
    float fu = 0.0f, fv = 0.0f;
    if (in) {
        fu = floorf(((qx * v.fx) / qz + v.cx) + 0.5f);
        fv = floorf(((qy * v.fy) / qz + v.cy) + 0.5f);
        in = fu >= 0.0f && fu < (float)v.w && fv >= 0.0f && fv < (float)v.h;
    }
    if (!in) return 1;                                                 /* OUT */
    const int u = (int)fu, vv = (int)fv;
    const int u0 = max(u - window, 0), u1 = min(u + window, v.w - 1);
    const int v0 = max(vv - window, 0), v1 = min(vv + window, v.h - 1);
    const float tol = d->tol, lim = qz - tol;
    bool sup = false, near = false, any = false;
    float r = INFINITY;
    for (int y = v0; y <= v1; y++) {
        const float *row = v.z + (size_t)y * v.w;
        for (int x = u0; x <= u1; x++) {
            const float zo = row[x];
            if (zo > 0.0f) {
                any = true;
                if (fabsf(zo - qz) <= tol) sup = true;
                if (zo < lim) near = true;
                if (RESID) r = fminf(r, fabsf(zo - qz));
            }
        }
    }
    if (RESID) {
        *u_out = u;
        *v_out = vv;
        *resid_out = r;
    }
    return sup ? 2 : near ? 3 : any ? 4 : 5;                           /* SUPPORTED, OCCLUDED, CONFLICT, UNKNOWN */
}

#endif /* OSLAM_VERIFY_CLASS_H */
