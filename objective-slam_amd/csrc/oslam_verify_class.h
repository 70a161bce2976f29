/*
 * oslam_verify_class.h -- the class of one model point against a view (include/oslam.h at oslam_verify), the one
 * source of k_verify (oslam_verify.hip) and k_claim (oslam_arbitrate.hip).  Device code only.
 *
 * RESID = false is k_verify's body.  RESID = true also returns what a claim needs: the point's pixel (valid for the
 * classes 2..5) and the smallest fabsf(z_o - p'z) over the valid pixels of its window (INFINITY without one; <= tol
 * exactly when the class is SUPPORTED).  The class does not depend on RESID: the extra minimum reads the same
 * differences the SUPPORTED test reads.
 * The transform and the pixel are oslam_icp_core.h's; the window walk and the classes are here.
 * Bounds: a point reads at most (2 window + 1)^2 <= 49 floats of the z image, all inside it (the window is clipped);
 * the pixel is range-checked in float before it becomes an int (oslam_icp_project).
 */
#ifndef OSLAM_VERIFY_CLASS_H
#define OSLAM_VERIFY_CLASS_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_icp_core.h"
#include "oslam_kernels.h"

/* point i of member d (i < d->m.n) -> 0 BACK .. 5 UNKNOWN */
template <bool RESID>
__device__ __forceinline__ int oslam_verify_class(const oslamk_view &v, const oslamk_verify_member *d, int i, int window,
                                                  int *u_out, int *v_out, float *resid_out)
{
    float q[3], m[3];
    int u, vv;
    oslam_icp_transform(d->T, d->m.px[i], d->m.py[i], d->m.pz[i], d->m.nx[i], d->m.ny[i], d->m.nz[i], q, m);
    if ((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2] >= 0.0f) return 0;   /* BACK */
    if (!oslam_icp_project(v, q, &u, &vv)) return 1;                   /* OUT */
    const float qz = q[2];
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
