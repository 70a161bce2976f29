/*
 * oslam_cloud.c -- clouds: the host and device copies of a model or scene cloud (cloud_buf), and the
 * stand-alone voxel grid and depth-to-cloud calls.
 */

#include "oslam_internal.h"

void oslam_cloud_free(cloud_buf *c)
{
    free(c->h_xyz);
    free(c->h_nrm);
    if (c->d_soa) oslam_dev_free(c->d_soa);
    memset(c, 0, sizeof *c);
}

oslamk_cloud oslam_soa_cloud(const float *d_soa, size_t n)
{
    const oslamk_cloud k = {d_soa, d_soa + n, d_soa + 2 * n, d_soa + 3 * n, d_soa + 4 * n, d_soa + 5 * n, (int)n};
    return k;
}

/* [n][6] (x y z nx ny nz per point) -> packed [n][3] positions and normals */
static void split6(const float *p6, size_t n, float *xyz, float *nrm)
{
    size_t i;
    for (i = 0; i < n; i++) {
        memcpy(xyz + 3 * i, p6 + 6 * i, 3 * sizeof(float));
        memcpy(nrm + 3 * i, p6 + 6 * i + 3, 3 * sizeof(float));
    }
}

/* A cloud's packed host copies and its structure of arrays in HBM, from host buffers (AoS with a stride,
 * scene.cu:28-40,68-69) or from a cloud that already lies in HBM as [n][6] (d_aos6: what the depth and voxel kernels
 * write; the structure of arrays is made on the device and one copy comes back for the host-side arrays). */
int oslam_cloud_make(cloud_buf *c, const float *xyz, const float *nrm, size_t stride, const float *d_aos6, size_t n)
{
    int rc = OSLAM_OK;
    float *h6 = NULL;                 /* the structure of arrays to upload, or the [n][6] copy of d_aos6 */
    size_t i;
    memset(c, 0, sizeof *c);
    c->n = (int)n;
    c->h_xyz = (float *)malloc(sizeof(float) * 3 * n);
    c->h_nrm = (float *)malloc(sizeof(float) * 3 * n);
    h6 = (float *)malloc(sizeof(float) * 6 * n);
    if (!c->h_xyz || !c->h_nrm || !h6) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    HIPCHK((hipError_t)oslam_dev_alloc((void **)&c->d_soa, sizeof(float) * 6 * n));
    if (d_aos6) {
        KCHK(oslamk_aos6_to_soa(d_aos6, n, c->d_soa, oslam_stream()));
        HIPCHK(hipMemcpyAsync(h6, d_aos6, sizeof(float) * 6 * n, hipMemcpyDeviceToHost, (hipStream_t)oslam_stream()));
        HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
        split6(h6, n, c->h_xyz, c->h_nrm);
    } else {
        for (i = 0; i < n; i++) {
            const float *p = (const float *)((const char *)xyz + i * stride);
            const float *q = (const float *)((const char *)nrm + i * stride);
            int a;
            for (a = 0; a < 3; a++) {
                c->h_xyz[3 * i + a] = p[a];
                c->h_nrm[3 * i + a] = q[a];
                h6[(size_t)a * n + i] = p[a];
                h6[(size_t)(3 + a) * n + i] = q[a];
            }
        }
        HIPCHK(hipMemcpy(c->d_soa, h6, sizeof(float) * 6 * n, hipMemcpyHostToDevice));
    }
    c->k = oslam_soa_cloud(c->d_soa, n);
done:
    free(h6);
    if (rc != OSLAM_OK) oslam_cloud_free(c);
    return rc;
}

/* ------------------------------------------------------------------------ */
int oslam_voxel_grid(const float *xyz, const float *nrm, size_t n, size_t stride_bytes, float leaf,
                     int dev, float *xyz_out, float *nrm_out, size_t cap, size_t *n_out)
{
    int rc = OSLAM_OK, k, devsel;
    cloud_buf c;
    float *d_out = NULL, *h_out = NULL;
    uint32_t nv = 0;
    memset(&c, 0, sizeof c);
    if (!xyz || !nrm || !xyz_out || !nrm_out || !n_out || stride_bytes < 12 || !(leaf > 0.0f) || n == 0 ||
        n > 0x7fffffffu)
        return fail(OSLAM_E_INVALID, "bad voxel grid arguments");
    *n_out = 0;
    rc = oslam_pick_device(dev, &devsel);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_cloud_make(&c, xyz, nrm, stride_bytes, NULL, n);
    if (rc != OSLAM_OK) return rc;
    HIPCHK((hipError_t)oslam_dev_alloc((void **)&d_out, sizeof(float) * 6 * n));
    k = oslamk_voxel_grid(c.k, leaf, d_out, &nv, oslam_stream());
    if (k == -1) { rc = fail(OSLAM_E_LIMIT, "leaf size too small for the cloud extent (voxel count overflows int32)"); goto done; }
    if (k != 0) { rc = fail(OSLAM_E_DEVICE, hipGetErrorString((hipError_t)k)); goto done; }
    if (nv > cap) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    h_out = (float *)malloc(sizeof(float) * 6 * (nv ? nv : 1));
    if (!h_out) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    if (nv) HIPCHK(hipMemcpy(h_out, d_out, sizeof(float) * 6 * nv, hipMemcpyDeviceToHost));
    split6(h_out, nv, xyz_out, nrm_out);
    *n_out = nv;
done:
    free(h_out);
    oslam_dev_free(d_out);
    oslam_cloud_free(&c);
    return rc;
}

/* ------------------------------------------------------------------------ */
int oslam_depth_points(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam, int dev,
                       void **d_img, float **d_pts6, uint32_t *np)
{
    int rc = OSLAM_OK, k, devsel;
    const size_t n_pix = (size_t)width * (size_t)height, px_bytes = depth_is_u16 ? 2 : 4;
    *d_img = NULL;
    *d_pts6 = NULL;
    *np = 0;
    if (!depth || !cam || width < 3 || height < 3 || width > 16384 || height > 16384 || !(cam->fx > 0.0f) ||
        !(cam->fy > 0.0f) || !(cam->depth_scale > 0.0f) || !(cam->z_max >= cam->z_min) || !(cam->z_min > 0.0f) ||
        !(cam->max_jump >= 0.0f))
        return fail(OSLAM_E_INVALID, "bad depth image arguments");
    rc = oslam_pick_device(dev, &devsel);
    if (rc != OSLAM_OK) return rc;
    HIPCHK((hipError_t)oslam_dev_alloc(d_img, n_pix * px_bytes));
    HIPCHK((hipError_t)oslam_dev_alloc((void **)d_pts6, sizeof(float) * 6 * n_pix));
    HIPCHK(hipMemcpyAsync(*d_img, depth, n_pix * px_bytes, hipMemcpyHostToDevice, (hipStream_t)oslam_stream()));
    k = oslamk_depth_to_cloud(*d_img, depth_is_u16 != 0, width, height, cam->fx, cam->fy, cam->cx, cam->cy, cam->depth_scale,
                              cam->z_min, cam->z_max, cam->max_jump, *d_pts6, np, oslam_stream());
    if (k != 0) rc = fail(OSLAM_E_DEVICE, hipGetErrorString((hipError_t)k));
done:
    return rc;
}

int oslam_depth_to_cloud(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam,
                         int dev, float *xyz_out, float *nrm_out, size_t cap, size_t *n_out)
{
    int rc;
    void *d_img;
    float *d_out, *h_out = NULL;
    uint32_t np;
    if (!xyz_out || !nrm_out || !n_out) return fail(OSLAM_E_INVALID, "bad depth image arguments");
    *n_out = 0;
    rc = oslam_depth_points(depth, depth_is_u16, width, height, cam, dev, &d_img, &d_out, &np);
    if (rc != OSLAM_OK) goto done;
    if (np > cap) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    h_out = (float *)malloc(sizeof(float) * 6 * (np ? np : 1));
    if (!h_out) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    if (np) HIPCHK(hipMemcpy(h_out, d_out, sizeof(float) * 6 * np, hipMemcpyDeviceToHost));
    split6(h_out, np, xyz_out, nrm_out);
    *n_out = np;
done:
    free(h_out);
    oslam_dev_free(d_img);
    oslam_dev_free(d_out);
    return rc;
}
