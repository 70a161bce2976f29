/*
 * rigid_check.c -- csrc/oslam_rigid.h included alone and held, bit for bit, to the expressions it replaced.  Built and
 * run by tests/test_rigid_host.py, once with the library's flags and once under the address and undefined-behaviour
 * sanitizers.  The functions named old_* are literal copies of the host stages' code before the header existed; they
 * are the statement of the contract (the GPU tests compare the poses made with them bit for bit), so they stay as they
 * are when the header changes.  Exit status 0 and "rigid_check ok" when every comparison holds.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oslam_rigid.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "rigid_check: line %d: %s\n", __LINE__, #c);      \
            return 1;                                                         \
        }                                                                     \
    } while (0)
#define SAME(a, b) (memcmp((a), (b), sizeof(a)) == 0 && sizeof(a) == sizeof(b))

/* ---- the expressions as they stood ---- */
/* oslam_verify.c oslam_is_zero_pose, oslam_refine.c is_zero_pose, oslam_instances.c is_zero: one text */
static int old_is_zero_pose(const float T[16])
{
    int k;
    for (k = 0; k < 16; k++)
        if (T[k] != 0.0f) return 0;
    return 1;
}

/* oslam_volume.c invert_rigid */
static void old_invert_rigid(const float T[16], float inv[12])
{
    int a, b;
    for (a = 0; a < 3; a++) {
        for (b = 0; b < 3; b++) inv[4 * a + b] = T[4 * b + a];
        inv[4 * a + 3] = (float)-(((double)T[a] * (double)T[3] + (double)T[4 + a] * (double)T[7]) + (double)T[8 + a] * (double)T[11]);
    }
}

/* oslam_volume.c pose_product */
static void old_pose_product(const float T_prev[16], const float T[16], float T_out[16])
{
    int a, b;
    for (a = 0; a < 3; a++)
        for (b = 0; b < 4; b++) {
            double x = ((double)T_prev[4 * a] * (double)T[b] + (double)T_prev[4 * a + 1] * (double)T[4 + b]) +
                       (double)T_prev[4 * a + 2] * (double)T[8 + b];
            if (b == 3) x += (double)T_prev[4 * a + 3];
            T_out[4 * a + b] = (float)x;
        }
    T_out[12] = T_out[13] = T_out[14] = 0.0f;
    T_out[15] = 1.0f;
}

/* oslam_tracker.c predict, on one track T and the accumulated camera Twc */
static void old_predict(float T[16], double Twc[16], const float C[16])
{
    double W[16], inv[12];
    int a, b;
    {
        float N[12];
        for (a = 0; a < 3; a++)
            for (b = 0; b < 4; b++) {
                double x = ((double)C[4 * a] * (double)T[b] + (double)C[4 * a + 1] * (double)T[4 + b]) +
                           (double)C[4 * a + 2] * (double)T[8 + b];
                if (b == 3) x += (double)C[4 * a + 3];
                N[4 * a + b] = (float)x;
            }
        for (a = 0; a < 12; a++)
            if (N[a] != T[a]) T[a] = N[a];      /* an element whose value does not change keeps its bits */
    }
    for (a = 0; a < 3; a++) {
        for (b = 0; b < 3; b++) inv[4 * a + b] = (double)C[4 * b + a];
        inv[4 * a + 3] = -(((double)C[a] * (double)C[3] + (double)C[4 + a] * (double)C[7]) + (double)C[8 + a] * (double)C[11]);
    }
    memcpy(W, Twc, sizeof W);
    for (a = 0; a < 3; a++)
        for (b = 0; b < 4; b++) {
            double x = (W[4 * a] * inv[b] + W[4 * a + 1] * inv[4 + b]) + W[4 * a + 2] * inv[8 + b];
            if (b == 3) x += W[4 * a + 3];
            Twc[4 * a + b] = x;
        }
}

/* oslam_refine.c set_pose (the descriptor's T, Tf and c from its cm) */
static void old_set_pose(double dT[12], float dTf[12], float dc[3], const double cm[3], const float T[16])
{
    double c[3];
    int a;
    for (a = 0; a < 12; a++) {
        dT[a] = (double)T[a];
        dTf[a] = T[a];
    }
    for (a = 0; a < 3; a++) {
        c[a] = ((dT[4 * a] * cm[0] + dT[4 * a + 1] * cm[1]) + dT[4 * a + 2] * cm[2]) + dT[4 * a + 3];
        dc[a] = (float)c[a];
    }
}

/* oslam_track.c set_member (the pose part; its centroid loop is old_centroid's) */
static void old_set_member(double dT[12], float dc[3], const double cm[3], const float T[16])
{
    int a;
    for (a = 0; a < 12; a++) dT[a] = (double)T[a];
    for (a = 0; a < 3; a++)
        dc[a] = (float)(((dT[4 * a] * cm[0] + dT[4 * a + 1] * cm[1]) + dT[4 * a + 2] * cm[2]) + dT[4 * a + 3]);
}

/* oslam_refine.c centroid, and the same loop inline in oslam_track.c set_member */
static void old_centroid(const float *h_xyz, size_t n, double cm[3])
{
    size_t i;
    int a;
    cm[0] = cm[1] = cm[2] = 0.0;
    for (i = 0; i < n; i++)
        for (a = 0; a < 3; a++) cm[a] += (double)h_xyz[3 * i + a];
    for (a = 0; a < 3; a++) cm[a] /= (double)n;
}

/* oslam_instances.c oslam_model_shape */
static void old_model_shape(const float *h_xyz, size_t n, float inst_c[3], float *inst_extent)
{
    double cm[3] = {0.0, 0.0, 0.0};
    float lo[3], hi[3], ext;
    size_t i;
    int a;
    for (a = 0; a < 3; a++) lo[a] = hi[a] = h_xyz[a];
    for (i = 0; i < n; i++)
        for (a = 0; a < 3; a++) {
            const float x = h_xyz[3 * i + a];
            cm[a] += (double)x;
            if (x < lo[a]) lo[a] = x;
            if (x > hi[a]) hi[a] = x;
        }
    for (a = 0; a < 3; a++) inst_c[a] = (float)(cm[a] / (double)n);
    ext = hi[0] - lo[0];
    if (hi[1] - lo[1] > ext) ext = hi[1] - lo[1];
    if (hi[2] - lo[2] > ext) ext = hi[2] - lo[2];
    *inst_extent = 1.0f * ext;
}

/* oslam_refine.c oslam_refine_check_rigid without the error text: the inputs below must be poses the library takes */
static int is_rigid(const float T[16])
{
    int a, b, k;
    double det;
    for (k = 0; k < 16; k++)
        if (!isfinite(T[k])) return 0;
    if (T[12] != 0.0f || T[13] != 0.0f || T[14] != 0.0f || T[15] != 1.0f) return 0;
    for (a = 0; a < 3; a++)
        for (b = 0; b < 3; b++) {
            double dot = 0.0;
            for (k = 0; k < 3; k++) dot += (double)T[4 * k + a] * (double)T[4 * k + b];
            if (fabs(dot - (a == b ? 1.0 : 0.0)) > 1e-3) return 0;
        }
    det = (double)T[0] * ((double)T[5] * T[10] - (double)T[6] * T[9]) - (double)T[1] * ((double)T[4] * T[10] - (double)T[6] * T[8]) +
          (double)T[2] * ((double)T[4] * T[9] - (double)T[5] * T[8]);
    return det > 0.0;
}

/* ---- inputs ---- */
static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static double uniform(void)                     /* xorshift64*, in [0, 1) */
{
    g_seed ^= g_seed >> 12;
    g_seed ^= g_seed << 25;
    g_seed ^= g_seed >> 27;
    return (double)((g_seed * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

/* a rotation from a random unit quaternion scaled by `scale`, a translation of up to t_max in each axis */
static void random_pose(float T[16], double scale, double t_max)
{
    double q[4], n = 0.0, R[9];
    int a;
    do {
        for (a = 0; a < 4; a++) q[a] = 2.0 * uniform() - 1.0;
        n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    } while (n < 1e-3 || n > 1.0);
    n = sqrt(n);
    for (a = 0; a < 4; a++) q[a] /= n;
    R[0] = 1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3]);
    R[1] = 2.0 * (q[1] * q[2] - q[0] * q[3]);
    R[2] = 2.0 * (q[1] * q[3] + q[0] * q[2]);
    R[3] = 2.0 * (q[1] * q[2] + q[0] * q[3]);
    R[4] = 1.0 - 2.0 * (q[1] * q[1] + q[3] * q[3]);
    R[5] = 2.0 * (q[2] * q[3] - q[0] * q[1]);
    R[6] = 2.0 * (q[1] * q[3] - q[0] * q[2]);
    R[7] = 2.0 * (q[2] * q[3] + q[0] * q[1]);
    R[8] = 1.0 - 2.0 * (q[1] * q[1] + q[2] * q[2]);
    memset(T, 0, 16 * sizeof(float));
    for (a = 0; a < 3; a++) {
        T[4 * a] = (float)(scale * R[3 * a]);
        T[4 * a + 1] = (float)(scale * R[3 * a + 1]);
        T[4 * a + 2] = (float)(scale * R[3 * a + 2]);
        T[4 * a + 3] = (float)(t_max * (2.0 * uniform() - 1.0));
    }
    T[15] = 1.0f;
}

/* every function of the header that takes poses, on the pair (A, B), a camera chain Twc and a centroid cm */
static int check_pair(const float A[16], const float B[16], double Twc[16], const double cm[3])
{
    float inv_old[12], inv_new[12], P_old[16], P_new[16], track_old[16], track_new[16], N[12];
    float Tf_old[12], c_old[3], c_trk[3], c_new[3];
    double inv_d[12], Twc_old[16], W[12], T_old[12], T_trk[12], T_new[12], c_d[3];
    int a;
    CHECK(is_rigid(A) && is_rigid(B));
    /* the inverse, as oslam_volume_integrate rounds it */
    old_invert_rigid(A, inv_old);
    oslam_rigid_inverse(A, inv_d);
    for (a = 0; a < 12; a++) inv_new[a] = (float)inv_d[a];
    CHECK(SAME(inv_old, inv_new));
    /* the product of floats, as oslam_volume_track closes it */
    old_pose_product(A, B, P_old);
    oslam_rigid_product_f(A, B, P_new);
    P_new[12] = P_new[13] = P_new[14] = 0.0f;
    P_new[15] = 1.0f;
    CHECK(SAME(P_old, P_new));
    /* the tracker's predict: the track B moved by the camera A under the keep-the-bits rule, the camera accumulated */
    memcpy(track_old, B, sizeof track_old);
    memcpy(track_new, B, sizeof track_new);
    memcpy(Twc_old, Twc, sizeof Twc_old);
    old_predict(track_old, Twc_old, A);
    oslam_rigid_product_f(A, track_new, N);
    for (a = 0; a < 12; a++)
        if (N[a] != track_new[a]) track_new[a] = N[a];
    oslam_rigid_inverse(A, inv_d);
    memcpy(W, Twc, sizeof W);
    oslam_rigid_product(W, inv_d, Twc);
    CHECK(SAME(track_old, track_new));
    CHECK(memcmp(Twc_old, Twc, sizeof Twc_old) == 0);
    /* the centroid under a pose, as the refinement and the tracking descriptors hold it */
    old_set_pose(T_old, Tf_old, c_old, cm, A);
    old_set_member(T_trk, c_trk, cm, A);
    for (a = 0; a < 12; a++) T_new[a] = (double)A[a];
    oslam_rigid_apply(T_new, cm, c_d);
    for (a = 0; a < 3; a++) c_new[a] = (float)c_d[a];
    CHECK(SAME(T_old, T_new) && SAME(T_trk, T_new) && memcmp(Tf_old, A, sizeof Tf_old) == 0);
    CHECK(SAME(c_old, c_new) && SAME(c_trk, c_new));
    return 0;
}

static int check_shape(size_t n)
{
    float *xyz = (float *)malloc(sizeof(float) * 3 * n), c_old[3], c_new[3], ext_old, ext_new;
    double cm_old[3], cm_new[3];
    size_t i;
    CHECK(xyz);
    for (i = 0; i < 3 * n; i++)                 /* magnitudes 1e-3 and 1e3, both signs, mixed within a point */
        xyz[i] = (float)((uniform() < 0.5 ? 1e-3 : 1e3) * (2.0 * uniform() - 1.0));
    old_centroid(xyz, n, cm_old);
    old_model_shape(xyz, n, c_old, &ext_old);
    oslam_cloud_shape(xyz, n, cm_new, c_new, &ext_new);
    free(xyz);
    CHECK(SAME(cm_old, cm_new) && SAME(c_old, c_new) && memcmp(&ext_old, &ext_new, sizeof ext_old) == 0);
    return 0;
}

int main(void)
{
    static const float special[][3] = {             /* translations with -0.0f and denormals */
        {-0.0f, 0.0f, -0.0f}, {1e-42f, -1e-45f, -0.0f}, {-1e-40f, 1e3f, 1.4e-45f}, {-0.0f, -0.0f, -0.0f}};
    static const size_t clouds[] = {1, 2, 3, 1501};
    float I[16], A[16], B[16], Z[16];
    double Twc[16], cm[3] = {0.0, 0.0, 0.0};
    float cf[3], ext;
    size_t k, s;
    int a;

    /* ---- the all-zero test ---- */
    memset(Z, 0, sizeof Z);
    CHECK(oslam_is_zero_pose(Z) == 1 && old_is_zero_pose(Z) == 1);
    for (a = 0; a < 16; a++) {
        memset(Z, 0, sizeof Z);
        Z[a] = -0.0f;
        CHECK(oslam_is_zero_pose(Z) == 1 && old_is_zero_pose(Z) == 1);
        Z[a] = NAN;
        CHECK(oslam_is_zero_pose(Z) == 0 && old_is_zero_pose(Z) == 0);
        Z[a] = 1.4e-45f;
        CHECK(oslam_is_zero_pose(Z) == 0 && old_is_zero_pose(Z) == 0);
    }

    /* ---- rigid inputs ---- */
    memset(I, 0, sizeof I);
    I[0] = I[5] = I[10] = I[15] = 1.0f;
    memset(Twc, 0, sizeof Twc);
    Twc[0] = Twc[5] = Twc[10] = Twc[15] = 1.0;
    if (check_pair(I, I, Twc, cm)) return 1;
    memcpy(B, I, sizeof B);
    for (k = 0; k < 10000; k++) {               /* the camera chain Twc runs on through all of them */
        random_pose(A, 1.0, 1e3);
        for (a = 0; a < 3; a++) cm[a] = (k & 1 ? 1e3 : 1e-3) * (2.0 * uniform() - 1.0);
        if (check_pair(A, B, Twc, cm) || check_pair(A, I, Twc, cm) || check_pair(I, A, Twc, cm)) return 1;
        memcpy(B, A, sizeof B);
    }
    /* rotations just inside the 1e-3 orthonormality tolerance: scaled by 1 +- 4.9e-4 (the squared length of a column
     * is then off by 9.8e-4), which check_pair proves with is_rigid */
    memset(Twc, 0, sizeof Twc);
    Twc[0] = Twc[5] = Twc[10] = Twc[15] = 1.0;
    for (k = 0; k < 1000; k++) {
        random_pose(A, k & 1 ? 1.0 + 4.9e-4 : 1.0 - 4.9e-4, 1e3);
        if (check_pair(A, B, Twc, cm)) return 1;
        memcpy(B, A, sizeof B);
    }
    /* -0.0f and denormals in the translation, under the identity (whose zeros then meet them) and under rotations */
    for (s = 0; s < sizeof special / sizeof special[0]; s++) {
        float J[16];
        memcpy(J, I, sizeof J);
        random_pose(A, 1.0, 1.0);
        for (a = 0; a < 3; a++) J[4 * a + 3] = A[4 * a + 3] = special[s][a];
        J[1] = J[6] = J[8] = -0.0f;
        memset(Twc, 0, sizeof Twc);
        Twc[0] = Twc[5] = Twc[10] = Twc[15] = 1.0;
        if (check_pair(J, J, Twc, cm) || check_pair(A, J, Twc, cm) || check_pair(J, A, Twc, cm) ||
            check_pair(A, A, Twc, cm))
            return 1;
    }

    /* ---- shapes ---- */
    for (s = 0; s < sizeof clouds / sizeof clouds[0]; s++)
        if (check_shape(clouds[s])) return 1;
    /* no points: all zero, and the cloud is not read */
    cm[0] = cf[0] = ext = 1.0f;
    oslam_cloud_shape(NULL, 0, cm, cf, &ext);
    CHECK(cm[0] == 0.0 && cm[1] == 0.0 && cm[2] == 0.0 && cf[0] == 0.0f && cf[1] == 0.0f && cf[2] == 0.0f && ext == 0.0f);

    printf("rigid_check ok\n");
    return 0;
}
