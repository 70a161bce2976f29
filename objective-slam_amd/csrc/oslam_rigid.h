/*
 * oslam_rigid.h -- the host stages' arithmetic on poses and clouds, once: the all-zero test, the inverse and the
 * product of rigid transforms in double, a transform applied to a point, and a cloud's mean and extent.  Host only,
 * static inline, no I/O, no error text and no HIP: tests/native/rigid_check.c includes it alone and holds every
 * function to the bits of the expressions it replaced.  The GPU tests compare poses bit for bit, so the order of the
 * operations written here is part of the contract; a caller rounds to float where its result is one.
 *
 * A pose is float[16] or its first 12 elements, rows of [R | t]; "12 doubles" are the same rows in double.
 */
#ifndef OSLAM_RIGID_H
#define OSLAM_RIGID_H

#include <stddef.h>

/* an all-zero pose marks a skipped member: -0.0f is zero, a NaN is not */
static inline int oslam_is_zero_pose(const float T[16])
{
    int k;
    for (k = 0; k < 16; k++)
        if (T[k] != 0.0f) return 0;
    return 1;
}

/* rows of the inverse of the rigid T: [R^T | -(R^T t)] */
static inline void oslam_rigid_inverse(const float T[16], double inv[12])
{
    int a, b;
    for (a = 0; a < 3; a++) {
        for (b = 0; b < 3; b++) inv[4 * a + b] = (double)T[4 * b + a];
        inv[4 * a + 3] = -(((double)T[a] * (double)T[3] + (double)T[4 + a] * (double)T[7]) + (double)T[8 + a] * (double)T[11]);
    }
}

/* out = A * B, all three rows of [R | t]; out overlaps neither */
static inline void oslam_rigid_product(const double A[12], const double B[12], double out[12])
{
    int a, b;
    for (a = 0; a < 3; a++)
        for (b = 0; b < 4; b++) {
            double x = (A[4 * a] * B[b] + A[4 * a + 1] * B[4 + b]) + A[4 * a + 2] * B[8 + b];
            if (b == 3) x += A[4 * a + 3];
            out[4 * a + b] = x;
        }
}

/* out = float32(double(A) * double(B)): the same product over the widened elements, rounded once */
static inline void oslam_rigid_product_f(const float A[16], const float B[16], float out[12])
{
    double Ad[12], Bd[12], P[12];
    int a;
    for (a = 0; a < 12; a++) {
        Ad[a] = (double)A[a];
        Bd[a] = (double)B[a];
    }
    oslam_rigid_product(Ad, Bd, P);
    for (a = 0; a < 12; a++) out[a] = (float)P[a];
}

/* out = R p + t */
static inline void oslam_rigid_apply(const double T[12], const double p[3], double out[3])
{
    int a;
    for (a = 0; a < 3; a++) out[a] = ((T[4 * a] * p[0] + T[4 * a + 1] * p[1]) + T[4 * a + 2] * p[2]) + T[4 * a + 3];
}

/* The shape of the cloud xyz[n][3]: its mean (summed in double in index order, divided by (double)n), the float
 * rounding of the mean, and the largest side of its bounding box.  A cloud without points has no mean (0/0): its
 * shape is all zero, and xyz is not read. */
static inline void oslam_cloud_shape(const float *xyz, size_t n, double mean[3], float mean_f[3], float *extent)
{
    float lo[3], hi[3];
    size_t i;
    int a;
    mean[0] = mean[1] = mean[2] = 0.0;
    mean_f[0] = mean_f[1] = mean_f[2] = 0.0f;
    *extent = 0.0f;
    if (n == 0) return;
    for (a = 0; a < 3; a++) lo[a] = hi[a] = xyz[a];
    for (i = 0; i < n; i++)
        for (a = 0; a < 3; a++) {
            const float x = xyz[3 * i + a];
            mean[a] += (double)x;
            if (x < lo[a]) lo[a] = x;
            if (x > hi[a]) hi[a] = x;
        }
    for (a = 0; a < 3; a++) {
        mean[a] /= (double)n;
        mean_f[a] = (float)mean[a];
    }
    *extent = hi[0] - lo[0];
    if (hi[1] - lo[1] > *extent) *extent = hi[1] - lo[1];
    if (hi[2] - lo[2] > *extent) *extent = hi[2] - lo[2];
}

#endif /* OSLAM_RIGID_H */
