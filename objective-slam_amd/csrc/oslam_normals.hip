/*
 * oslam_normals.hip -- the normal estimation's kernel (semantics: include/oslam.h at oslam_cloud_normals; host side:
 * oslam_normals.c).  The neighbourhood grid is the refinement stage's (oslamk_refine_grid_build, oslam_refine.hip).
 *
 *   k_normals      one thread per grid position, not per input index: thread k takes pts[k] and writes to the input index
 *                  in its .w, so the threads of a wave walk the same cells.  The 27-cell walk sums the ten int64 moments
 *                  of the rule (exact, whatever the order inside a cell); then the covariance, the Jacobi sweeps fully
 *                  unrolled on scalars, validity, sign and the stores.  No LDS, no float atomics, no indexed local arrays.
 *
 * Every double operation is + - * / sqrt or a comparison, each correctly rounded, and -ffp-contract=off keeps them apart:
 * the results equal tests/normals_ref.py bit for bit.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam.h"
#include "oslam_kernels.h"

/* the cell coordinate of oslam_refine.hip's grid kernels: far outside (or NaN) gives a cell the walk clamps away */
__device__ __forceinline__ int normals_axis(float x, double lo, double inv, int dim)
{
    double f = floor(((double)x - lo) * inv);
    f = fmin(fmax(f, -2.0), (double)dim + 1.0);
    return (int)f;
}

/* one Jacobi rotation in the plane (p, q); r is the third index.  vNp / vNq: row N of V */
__device__ __forceinline__ void jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                              double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    const double tt = 1.0 / (at + sqrt(theta * theta + 1.0));
    const double t = theta < 0.0 ? -tt : tt;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
    x = v0p; y = v0q;
    v0p = c * x - s * y;
    v0q = s * x + c * y;
    x = v1p; y = v1q;
    v1p = c * x - s * y;
    v1q = s * x + c * y;
    x = v2p; y = v2q;
    v2p = c * x - s * y;
    v2q = s * x + c * y;
}

__global__ __launch_bounds__(OSLAMK_NORMALS_THREADS) void k_normals(const oslamk_grid g, const oslamk_normals_args a)
{
    const int k = (int)(blockIdx.x * OSLAMK_NORMALS_THREADS + threadIdx.x);
    if (k >= g.n) return;
    const float4 *pts = reinterpret_cast<const float4 *>(g.pts);
    const float4 me = pts[2 * (size_t)k];
    const size_t idx = (size_t)__float_as_int(me.w);
    const float px = me.x, py = me.y, pz = me.z;

    const int cx = normals_axis(px, g.lo[0], g.inv_edge, g.dim[0]);
    const int cy = normals_axis(py, g.lo[1], g.inv_edge, g.dim[1]);
    const int cz = normals_axis(pz, g.lo[2], g.inv_edge, g.dim[2]);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
    const int y0 = max(cy - 1, 0), y1 = min(cy + 1, g.dim[1] - 1);
    const int z0 = max(cz - 1, 0), z1 = min(cz + 1, g.dim[2] - 1);

    int64_t n = 0, sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    if (x0 <= x1 && y0 <= y1 && z0 <= z1) {
        for (int zz = z0; zz <= z1; zz++)
            for (int yy = y0; yy <= y1; yy++) {
                const uint32_t row = ((uint32_t)zz * (uint32_t)g.dim[1] + (uint32_t)yy) * (uint32_t)g.dim[0];
                const uint32_t e = g.start[row + (uint32_t)x1 + 1u];
                for (uint32_t j = g.start[row + (uint32_t)x0]; j < e; j++) {
                    const float4 b = pts[2 * (size_t)j];
                    const float dx = b.x - px, dy = b.y - py, dz = b.z - pz;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 <= a.r2)) continue;
                    /* |d_a| <= radius (1 + a few ulp): |q_a| <= 16385 and every product fits an int32 */
                    const int32_t qx = (int32_t)rintf(dx * a.scale);
                    const int32_t qy = (int32_t)rintf(dy * a.scale);
                    const int32_t qz = (int32_t)rintf(dz * a.scale);
                    n += 1;
                    sx += qx;
                    sy += qy;
                    sz += qz;
                    sxx += qx * qx;
                    sxy += qx * qy;
                    sxz += qx * qz;
                    syy += qy * qy;
                    syz += qy * qz;
                    szz += qz * qz;
                }
            }
    }
    if (a.moments) {
        int64_t *m = a.moments + 10 * idx;
        m[0] = n;   m[1] = sx;  m[2] = sy;  m[3] = sz;  m[4] = sxx;
        m[5] = sxy; m[6] = sxz; m[7] = syy; m[8] = syz; m[9] = szz;
    }

    float onx = 0.0f, ony = 0.0f, onz = 0.0f, ocurv = 0.0f;
    uint8_t ovalid = 0;
    if (n >= a.min_neighbours) {
        const double dn = (double)n;
        const double mx = (double)sx / dn, my = (double)sy / dn, mz = (double)sz / dn;
        double a00 = (double)sxx / dn - mx * mx, a01 = (double)sxy / dn - mx * my, a02 = (double)sxz / dn - mx * mz;
        double a11 = (double)syy / dn - my * my, a12 = (double)syz / dn - my * mz, a22 = (double)szz / dn - mz * mz;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
        for (int s = 0; s < OSLAM_NORMALS_SWEEPS; s++) {
            jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        const double lo01 = a00 < a11 ? a00 : a11, hi01 = a00 < a11 ? a11 : a00;
        const double lmin = lo01 < a22 ? lo01 : a22;
        const double lmax = hi01 < a22 ? a22 : hi01;
        const double h2 = hi01 < a22 ? hi01 : a22;
        const double lmid = lo01 < h2 ? h2 : lo01;
        if (lmid > a.line_ratio * lmax) {
            double nx, ny, nz;
            if (a00 <= a11 && a00 <= a22) { nx = v00; ny = v10; nz = v20; }
            else if (a11 <= a22)          { nx = v01; ny = v11; nz = v21; }
            else                          { nx = v02; ny = v12; nz = v22; }
            const double len = sqrt((nx * nx + ny * ny) + nz * nz);
            nx = nx / len;
            ny = ny / len;
            nz = nz / len;
            if (a.orient) {
                const double dot = (nx * (a.view[0] - (double)px) + ny * (a.view[1] - (double)py)) + nz * (a.view[2] - (double)pz);
                if (dot < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
            }
            const double sum = (a00 + a11) + a22;
            onx = (float)nx;
            ony = (float)ny;
            onz = (float)nz;
            ocurv = sum == 0.0 ? 0.0f : (float)(lmin / sum);
            ovalid = 1;
        }
    }
    a.nrm[3 * idx] = onx;
    a.nrm[3 * idx + 1] = ony;
    a.nrm[3 * idx + 2] = onz;
    a.curvature[idx] = ocurv;
    a.valid[idx] = ovalid;
}

extern "C" int oslamk_normals(const oslamk_grid *g, const oslamk_normals_args *a, void *stream)
{
    if (g->n <= 0 || !a->nrm || !a->curvature || !a->valid) return (int)hipErrorInvalidValue;
    const unsigned nb = (unsigned)(((size_t)g->n + OSLAMK_NORMALS_THREADS - 1) / OSLAMK_NORMALS_THREADS);
    hipLaunchKernelGGL(k_normals, dim3(nb), dim3(OSLAMK_NORMALS_THREADS), 0, (hipStream_t)stream, *g, *a);
    return (int)hipGetLastError();
}
