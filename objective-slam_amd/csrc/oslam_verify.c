/*
 * oslam_verify.c -- verification against a depth image (include/oslam.h at oslam_verify): the host side of the kernels
 * in oslam_verify.hip.  A view is the image as float z on the device; a call checks its arguments, uploads one
 * descriptor per member (its pose, its tolerance and the model's device cloud), zeroes the counters, runs k_verify
 * once for every member and reads the counters back with one host wait.  Views are made here for every stage
 * (oslam_view_new: oslam_view_create, the ray cast, a pyramid's levels), and here is the check of a list of poses and
 * models that verification, refinement, arbitration and tracking share (oslam_check_poses, oslam_check_handles).
 */
#include <math.h>

#include "oslam_internal.h"

int oslam_view_camera_ok(const oslam_camera *cam, int width, int height, int with_depth_scale, int with_max_jump)
{
    if (width < 1 || height < 1 || width > 16384 || height > 16384 || !isfinite(cam->fx) || !isfinite(cam->fy) ||
        !isfinite(cam->cx) || !isfinite(cam->cy) || !(cam->fx > 0.0f) || !(cam->fy > 0.0f) || !(cam->z_max >= cam->z_min) ||
        !(cam->z_min > 0.0f) || !isfinite(cam->z_max))
        return 0;
    if (with_depth_scale && (!(cam->depth_scale > 0.0f) || !isfinite(cam->depth_scale))) return 0;
    if (with_max_jump && (!(cam->max_jump >= 0.0f) || !isfinite(cam->max_jump))) return 0;
    return 1;
}

int oslam_view_new(int dev, int width, int height, const oslam_camera *cam, oslam_view **out)
{
    int rc = OSLAM_OK;
    oslam_view *v = (oslam_view *)calloc(1, sizeof *v);
    *out = NULL;
    if (!v) return fail(OSLAM_E_NOMEM, "host allocation failed");
    v->dev = dev;
    v->k.w = width;
    v->k.h = height;
    v->k.fx = cam->fx;
    v->k.fy = cam->fy;
    v->k.cx = cam->cx;
    v->k.cy = cam->cy;
    v->k.z_min = cam->z_min;
    v->k.z_max = cam->z_max;
    v->max_jump = cam->max_jump;
    /* the z image lives as long as the view: its own block, not one of the kept scratch blocks */
    HIPCHK(hipMalloc((void **)&v->d_z, sizeof(float) * (size_t)width * (size_t)height));
    v->k.z = v->d_z;
    *out = v;
done:
    if (rc != OSLAM_OK) free(v);
    return rc;
}

void oslam_view_camera(const oslam_view *v, oslam_camera *cam)
{
    memset(cam, 0, sizeof *cam);
    cam->fx = v->k.fx;
    cam->fy = v->k.fy;
    cam->cx = v->k.cx;
    cam->cy = v->k.cy;
    cam->depth_scale = 1.0f;
    cam->z_min = v->k.z_min;
    cam->z_max = v->k.z_max;
    cam->max_jump = v->max_jump;
}

int oslam_view_create(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam, int dev,
                      oslam_view **out)
{
    int rc = OSLAM_OK, devsel;
    const size_t n_pix = (size_t)width * (size_t)height, px_bytes = depth_is_u16 ? 2 : 4;
    void *d_raw = NULL;
    oslam_view *v = NULL;
    if (out) *out = NULL;
    if (!depth || !cam || !out || !oslam_view_camera_ok(cam, width, height, 1, 0))
        return fail(OSLAM_E_INVALID, "bad view arguments");
    rc = oslam_pick_device(dev, &devsel);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_view_new(devsel, width, height, cam, &v);
    if (rc != OSLAM_OK) return rc;
    HIPCHK((hipError_t)oslam_dev_alloc(&d_raw, n_pix * px_bytes));
    HIPCHK(hipMemcpyAsync(d_raw, depth, n_pix * px_bytes, hipMemcpyHostToDevice, (hipStream_t)oslam_stream()));
    KCHK(oslamk_view_z(d_raw, depth_is_u16 != 0, width, height, cam->depth_scale, cam->z_min, cam->z_max, v->d_z,
                       oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)oslam_stream());
    oslam_dev_free(d_raw);
    if (rc != OSLAM_OK) {
        oslam_view_destroy(v);
        return rc;
    }
    *out = v;
    return OSLAM_OK;
}

int oslam_view_destroy(oslam_view *v)
{
    if (!v) return fail(OSLAM_E_INVALID, "view is NULL");
    /* every call that read the image ended with a synchronisation of its stream */
    if (hipSetDevice(v->dev) == hipSuccess) {
        oslam_track_release_maps(v);
        oslam_colour_release_view(v);
        (void)hipFree(v->d_z);
    }
    free(v);
    return OSLAM_OK;
}

int oslam_verify_params_default(oslam_verify_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->depth_tol = 1.0f;
    p->window = 1;
    p->min_view_fitness = 0.92f;
    p->min_coverage = 0.5f;
    p->min_supported = 50;
    return OSLAM_OK;
}

int oslam_verify_check_params(const oslam_verify_params *vp, oslam_verify_params *out)
{
    if (vp) *out = *vp;
    else oslam_verify_params_default(out);
    if (!isfinite(out->depth_tol) || !isfinite(out->min_view_fitness) || !isfinite(out->min_coverage))
        return fail(OSLAM_E_INVALID, "verify parameters must be finite");
    if (!(out->depth_tol > 0.0f)) return fail(OSLAM_E_INVALID, "depth_tol must be > 0");
    if (out->window > 3) return fail(OSLAM_E_INVALID, "window above 3");
    if (out->min_view_fitness < 0.0f || out->min_view_fitness > 1.0f || out->min_coverage < 0.0f || out->min_coverage > 1.0f)
        return fail(OSLAM_E_INVALID, "min_view_fitness and min_coverage must lie in [0, 1]");
    return OSLAM_OK;
}

int oslam_view_check_pair(const oslam_model *m, const oslam_view *v)
{
    if (m->unusable) return fail(OSLAM_E_INVALID, "this model lost its key tables with its database: it can only be destroyed");
    if (m->dev != v->dev) return fail(OSLAM_E_INVALID, "model and view live on different devices");
    return OSLAM_OK;
}

int oslam_check_poses(oslam_model *const *ms, const float *T, size_t n, int hypotheses)
{
    size_t j;
    int rc;
    if (hypotheses && (n == 0 || n > OSLAM_ARBITRATE_MAX_HYPOTHESES))
        return fail(OSLAM_E_INVALID, "the number of hypotheses must lie in 1..OSLAM_ARBITRATE_MAX_HYPOTHESES");
    for (j = 0; j < n; j++) {
        if (ms && !ms[j]) return fail(OSLAM_E_INVALID, "NULL model");
        if (oslam_is_zero_pose(T + 16 * j)) continue;
        rc = oslam_refine_check_rigid(T + 16 * j);
        if (rc != OSLAM_OK) return rc;
    }
    return OSLAM_OK;
}

int oslam_check_handles(oslam_model *const *ms, const float *T, size_t n, const oslam_view *v)
{
    size_t j;
    int rc;
    for (j = 0; j < n; j++) {
        if (oslam_is_zero_pose(T + 16 * j)) continue;
        rc = oslam_view_check_pair(ms[j], v);
        if (rc != OSLAM_OK) return rc;
    }
    return OSLAM_OK;
}

void oslam_verify_fill_result(oslam_verify_result *r, const uint32_t *c, const oslam_verify_params *p)
{
    const uint32_t sx = c[2] + c[4], sox = sx + c[3];
    r->back = c[0];
    r->out = c[1];
    r->supported = c[2];
    r->occluded = c[3];
    r->conflict = c[4];
    r->unknown = c[5];
    r->view_fitness = sx ? (float)r->supported / (float)sx : 0.0f;
    r->coverage = sox ? (float)r->supported / (float)sox : 0.0f;
    r->found = r->supported >= p->min_supported && r->view_fitness >= p->min_view_fitness && r->coverage >= p->min_coverage;
}

void oslam_verify_set_member(oslamk_verify_member *d, const oslam_model *m, const float T[16], float depth_tol)
{
    int a;
    d->m = m->c.k;
    for (a = 0; a < 12; a++) d->T[a] = T[a];
    d->tol = (float)((double)depth_tol * (double)m->d_dist);
    d->n_blocks = (uint32_t)(((size_t)m->c.n + OSLAMK_VERIFY_THREADS - 1) / OSLAMK_VERIFY_THREADS);
}

/* members ms[0 .. n) with T [n][16] (all-zero = skipped) against view v: one memset, one kernel, one copy back */
int oslam_verify_members(oslam_model *const *ms, size_t n, const oslam_view *v, const float *T, const oslam_verify_params *p,
                         oslam_verify_result *res)
{
    int rc = OSLAM_OK;
    const double t0 = now_ms();
    size_t j, max_blocks = 0, off_cnt, bytes;
    oslamk_verify_member *h = NULL;
    uint32_t *cnt = NULL, launches = 0;
    char *dev = NULL;
    void *stream = oslam_stream();

    memset(res, 0, sizeof *res * n);
    if (n > 65535) return fail(OSLAM_E_LIMIT, "more than 65535 members in one verification");
    off_cnt = align256(sizeof *h * (n ? n : 1));
    bytes = off_cnt + sizeof(uint32_t) * OSLAMK_VERIFY_CLASSES * (n ? n : 1);
    h = (oslamk_verify_member *)calloc(n ? n : 1, sizeof *h);
    cnt = (uint32_t *)calloc((n ? n : 1) * OSLAMK_VERIFY_CLASSES, sizeof *cnt);
    if (!h || !cnt) { free(h); free(cnt); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    for (j = 0; j < n; j++)
        if (!oslam_is_zero_pose(T + 16 * j)) {
            oslam_verify_set_member(&h[j], ms[j], T + 16 * j, p->depth_tol);
            if (h[j].n_blocks > max_blocks) max_blocks = h[j].n_blocks;
        }
    if (max_blocks == 0) goto done;             /* every member skipped: no device work */
    if (hipSetDevice(v->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    KCHK(oslam_dev_alloc((void **)&dev, bytes));
    HIPCHK(hipMemcpyAsync(dev, h, sizeof *h * n, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(dev + off_cnt, 0, sizeof(uint32_t) * OSLAMK_VERIFY_CLASSES * n, (hipStream_t)stream));
    KCHK(oslamk_verify(&v->k, (const oslamk_verify_member *)dev, (uint32_t)n, (uint32_t)max_blocks, (int)p->window,
                       (uint32_t *)(dev + off_cnt), NULL, stream));
    launches++;
    HIPCHK(hipMemcpyAsync(cnt, dev + off_cnt, sizeof(uint32_t) * OSLAMK_VERIFY_CLASSES * n, hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (j = 0; j < n; j++)
        if (h[j].n_blocks) oslam_verify_fill_result(&res[j], cnt + OSLAMK_VERIFY_CLASSES * j, p);
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);    /* nothing may still use the block */
    if (dev) oslam_dev_free(dev);
    if (rc == OSLAM_OK) {
        const float ms_total = (float)(now_ms() - t0);
        for (j = 0; j < n; j++) {
            res[j].launches = launches;
            res[j].ms_total = ms_total;
        }
    }
    free(h);
    free(cnt);
    return rc;
}

int oslam_verify(oslam_model *m, const oslam_view *v, const float T[16], const oslam_verify_params *vp,
                 oslam_verify_result *res)
{
    oslam_verify_params p;
    int rc;
    if (!m || !v || !T || !res) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_verify_check_params(vp, &p);
    if (rc == OSLAM_OK) rc = oslam_refine_check_rigid(T);
    if (rc == OSLAM_OK) rc = oslam_view_check_pair(m, v);
    if (rc != OSLAM_OK) return rc;
    return oslam_verify_members(&m, 1, v, T, &p, res);
}

int oslam_db_verify(oslam_db *db, const oslam_view *v, const float *T, const oslam_verify_params *vp,
                    oslam_verify_result *res)
{
    oslam_verify_params p;
    int rc;
    if (!db || !v || !T || !res) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_verify_check_params(vp, &p);
    if (rc == OSLAM_OK) rc = oslam_check_poses(NULL, T, db->n, 0);
    if (rc == OSLAM_OK) rc = oslam_check_handles(db->models, T, db->n, v);
    if (rc != OSLAM_OK) return rc;
    return oslam_verify_members(db->models, db->n, v, T, &p, res);
}

int oslam_verify_classes(oslam_model *m, const oslam_view *v, const float T[16], const oslam_verify_params *vp,
                         uint8_t *class_out)
{
    oslam_verify_params p;
    oslamk_verify_member h;
    char *dev = NULL;
    void *stream = oslam_stream();
    size_t M, off_cls;
    int rc;
    if (!m || !v || !T || !class_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_verify_check_params(vp, &p);
    if (rc == OSLAM_OK) rc = oslam_refine_check_rigid(T);
    if (rc == OSLAM_OK) rc = oslam_view_check_pair(m, v);
    if (rc != OSLAM_OK) return rc;
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    M = (size_t)m->c.n;
    memset(&h, 0, sizeof h);
    oslam_verify_set_member(&h, m, T, p.depth_tol);
    off_cls = align256(sizeof h);
    KCHK(oslam_dev_alloc((void **)&dev, off_cls + M));
    HIPCHK(hipMemcpyAsync(dev, &h, sizeof h, hipMemcpyHostToDevice, (hipStream_t)stream));
    KCHK(oslamk_verify(&v->k, (const oslamk_verify_member *)dev, 1, h.n_blocks, (int)p.window, NULL,
                       (uint8_t *)(dev + off_cls), stream));
    HIPCHK(hipMemcpyAsync(class_out, dev + off_cls, M, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    if (dev) oslam_dev_free(dev);
    return rc;
}
