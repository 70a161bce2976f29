/*
 * oslam_refine_step.h -- the Gauss-Newton step of the point-to-plane ICP (include/oslam.h at oslam_refine, "Step"), the
 * one source of the refinement kernels (oslam_refine.hip: correspondences from the scene grid), of k_track
 * (oslam_track.hip: correspondences from the depth image) and of k_ego_step (oslam_ego.hip: from another view's maps).
 * What surrounds the step -- transform, projection, gates, the block's fixed-order sums -- is oslam_icp_core.h.
 * Device code only.
 *
 *   oslam_refine_point_sums   the 29 terms of one correspondence: J^T J upper triangle (21, row-major), J^T r (6), 1, r^2
 *   oslam_refine_step         the sums in double -> damped Cholesky, Rodrigues, the pose update about the transformed
 *                             centroid and Gram-Schmidt; one thread
 */
#ifndef OSLAM_REFINE_STEP_H
#define OSLAM_REFINE_STEP_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"

/* transformed model point q, its correspondence a (point) and b (normal), c = the transformed centroid (float32) */
__device__ __forceinline__ void oslam_refine_point_sums(float qx, float qy, float qz, const float4 a, const float4 b,
                                                        const float *c, float *s)
{
    const float ex = qx - a.x, ey = qy - a.y, ez = qz - a.z;
    const float r = (b.x * ex + b.y * ey) + b.z * ez;
    const float ux = qx - c[0], uy = qy - c[1], uz = qz - c[2];
    float J[6];
    J[0] = uy * b.z - uz * b.y;
    J[1] = uz * b.x - ux * b.z;
    J[2] = ux * b.y - uy * b.x;
    J[3] = b.x;
    J[4] = b.y;
    J[5] = b.z;
    int k = 0;
#pragma unroll
    for (int u = 0; u < 6; u++)
#pragma unroll
        for (int v = u; v < 6; v++) s[k++] = J[u] * J[v];
#pragma unroll
    for (int u = 0; u < 6; u++) s[21 + u] = J[u] * r;
    s[27] = 1.0f;
    s[28] = r * r;
}

__device__ inline void oslam_rot_apply(const double R[9], const double x[3], double y[3])
{
    for (int a = 0; a < 3; a++) y[a] = (R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2];
}

/* S: the OSLAMK_REFINE_SUMS sums in double.  T: rows of [R | t] in double, cm: the model centroid.  Returns 0 with
 * nothing changed when fewer than 6 correspondences or a failed factorisation stop the member; otherwise 1 with T
 * stepped, Tf = its float32 rounding, c = float32(T cm), *th = |omega| and *vn = |v|. */
__device__ inline int oslam_refine_step(const double *S, double *T, const double *cm, float *Tf, float *cf, double *th_out,
                                        double *vn_out)
{
    if (S[27] < 6.0) return 0;
    double A[36], x[6], L[36];
    int k = 0;
    for (int u = 0; u < 6; u++)
        for (int v = u; v < 6; v++) {
            A[6 * u + v] = S[k];
            A[6 * v + u] = S[k];
            k++;
        }
    const double mu = 1e-6 * (((((A[0] + A[7]) + A[14]) + A[21]) + A[28]) + A[35]) / 6.0;
    for (int u = 0; u < 6; u++) A[7 * u] += mu;
    /* Cholesky A = L L^T */
    for (int u = 0; u < 6; u++) {
        for (int v = 0; v <= u; v++) {
            double t = A[6 * u + v];
            for (int q = 0; q < v; q++) t -= L[6 * u + q] * L[6 * v + q];
            if (u == v) {
                if (!(t > 0.0)) return 0;
                L[7 * u] = sqrt(t);
            } else {
                L[6 * u + v] = t / L[7 * v];
            }
        }
    }
    double y[6];
    for (int u = 0; u < 6; u++) {
        double t = -S[21 + u];                      /* b = -sum J^T r */
        for (int q = 0; q < u; q++) t -= L[6 * u + q] * y[q];
        y[u] = t / L[7 * u];
    }
    for (int u = 5; u >= 0; u--) {
        double t = y[u];
        for (int q = u + 1; q < 6; q++) t -= L[6 * q + u] * x[q];
        x[u] = t / L[7 * u];
    }

    /* dR = Rodrigues(omega) */
    const double th = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    double dR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th > 0.0) {
        const double kx = x[0] / th, ky = x[1] / th, kz = x[2] / th;
        const double cs = cos(th), sn = sin(th), vc = 1.0 - cs;
        dR[0] = cs + kx * kx * vc;      dR[1] = kx * ky * vc - kz * sn; dR[2] = kx * kz * vc + ky * sn;
        dR[3] = ky * kx * vc + kz * sn; dR[4] = cs + ky * ky * vc;      dR[5] = ky * kz * vc - kx * sn;
        dR[6] = kz * kx * vc - ky * sn; dR[7] = kz * ky * vc + kx * sn; dR[8] = cs + kz * kz * vc;
    }
    double R[9], t[3], c[3], Rn[9], tn[3], dRc[3], dRt[3];
    for (int a = 0; a < 3; a++) {
        R[3 * a] = T[4 * a]; R[3 * a + 1] = T[4 * a + 1]; R[3 * a + 2] = T[4 * a + 2];
        t[a] = T[4 * a + 3];
    }
    oslam_rot_apply(R, cm, c);
    for (int a = 0; a < 3; a++) c[a] += t[a];
    oslam_rot_apply(dR, c, dRc);
    oslam_rot_apply(dR, t, dRt);
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++)
            Rn[3 * a + b] = (dR[3 * a] * R[b] + dR[3 * a + 1] * R[3 + b]) + dR[3 * a + 2] * R[6 + b];
        tn[a] = dRt[a] + ((c[a] - dRc[a]) + x[3 + a]);
    }
    /* Gram-Schmidt over the columns x, y, z */
    for (int col = 0; col < 3; col++) {
        for (int prev = 0; prev < col; prev++) {
            const double p = (Rn[prev] * Rn[col] + Rn[3 + prev] * Rn[3 + col]) + Rn[6 + prev] * Rn[6 + col];
            for (int a = 0; a < 3; a++) Rn[3 * a + col] -= p * Rn[3 * a + prev];
        }
        const double nrm = sqrt((Rn[col] * Rn[col] + Rn[3 + col] * Rn[3 + col]) + Rn[6 + col] * Rn[6 + col]);
        for (int a = 0; a < 3; a++) Rn[3 * a + col] /= nrm;
    }
    for (int a = 0; a < 3; a++) {
        T[4 * a] = Rn[3 * a]; T[4 * a + 1] = Rn[3 * a + 1]; T[4 * a + 2] = Rn[3 * a + 2];
        T[4 * a + 3] = tn[a];
    }
    for (int q = 0; q < 12; q++) Tf[q] = (float)T[q];
    oslam_rot_apply(Rn, cm, c);
    for (int a = 0; a < 3; a++) cf[a] = (float)(c[a] + tn[a]);
    *th_out = th;
    *vn_out = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    return 1;
}

#endif /* OSLAM_REFINE_STEP_H */
