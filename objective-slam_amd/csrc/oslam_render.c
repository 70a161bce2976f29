/*
 * oslam_render.c -- hypotheses rendered into a labelled depth view, and views masked by it (include/oslam.h at
 * oslam_render_create and oslam_view_mask): the host side of the kernels in oslam_render.hip.  A render owns a genuine
 * oslam_view (oslam_view_new: the z image and the caller's camera; its maps are built on first use by the tracking
 * stage's path) and one block with the label image and the hypotheses' tolerances.  A call checks its arguments,
 * uploads one block (k_verify's descriptor per hypothesis, its splat radius, and the zeroed counters), presets the keys
 * with one memset, runs k_render_splat and k_render_resolve back to back and reads the counters back with one host wait.
 * oslam_view_mask is one memset, k_view_mask and one copy back.
 */
#include <math.h>

#include "oslam_internal.h"

int oslam_render_params_default(oslam_render_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->footprint = 0.75f;
    p->max_splat = OSLAM_RENDER_MAX_SPLAT;
    p->depth_tol = 1.0f;
    return OSLAM_OK;
}

int oslam_render_check_params(const oslam_render_params *rp, oslam_render_params *out)
{
    if (rp) *out = *rp;
    else oslam_render_params_default(out);
    if (!isfinite(out->footprint) || !isfinite(out->depth_tol)) return fail(OSLAM_E_INVALID, "render parameters must be finite");
    if (!(out->footprint > 0.0f)) return fail(OSLAM_E_INVALID, "footprint must be > 0");
    if (out->max_splat > OSLAM_RENDER_MAX_SPLAT) return fail(OSLAM_E_INVALID, "max_splat above OSLAM_RENDER_MAX_SPLAT");
    if (!(out->depth_tol > 0.0f)) return fail(OSLAM_E_INVALID, "depth_tol must be > 0");
    return OSLAM_OK;
}

int oslam_mask_params_default(oslam_mask_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->mode = OSLAM_MASK_REMOVE;
    p->dilate = 2;
    p->only = -1;
    return OSLAM_OK;
}

static void release(oslam_render *r)
{
    /* every call that read the images ended with a synchronisation of its stream */
    if (r->view) oslam_view_destroy(r->view);
    if (r->d_labels && hipSetDevice(r->dev) == hipSuccess) (void)hipFree(r->d_labels);
    free(r);
}

/* what every entry point checks before a handle is read: the parameters, the count and the poses, the camera */
static int render_check(oslam_model *const *ms, const float *T, size_t H, const oslam_camera *cam, int width, int height,
                        const oslam_render_params *rp, oslam_render_params *p)
{
    int rc = oslam_render_check_params(rp, p);
    if (rc == OSLAM_OK) rc = oslam_check_poses(ms, T, H, 1);
    if (rc == OSLAM_OK && !oslam_view_camera_ok(cam, width, height, 1, 1))
        rc = fail(OSLAM_E_INVALID, "bad render camera or size");
    return rc;
}

/* hypotheses ms[0 .. H) with T [H][16] (all-zero = skipped), all arguments checked; dev: the device when every one is
 * skipped, where an empty render lives (-1: device 0, bound here) */
static int render_members(oslam_model *const *ms, const float *T, size_t H, int dev, const oslam_camera *cam, int width,
                          int height, const oslam_render_params *p, oslam_render **out, oslam_render_result *res)
{
    int rc = OSLAM_OK, any = 0;
    const double t0 = now_ms();
    const size_t n_pix = (size_t)width * (size_t)height;
    size_t h, max_blocks = 0, off_rho, off_cnt, up_bytes, off_keys;
    char *up = NULL, *d_up = NULL;
    oslamk_verify_member *hm;
    float *rho;
    uint32_t *cnt = NULL, launches = 0;
    oslam_render *r = NULL;
    void *stream = oslam_stream();

    for (h = 0; h < H; h++) {
        if (oslam_is_zero_pose(T + 16 * h)) continue;
        if (ms[h]->unusable)
            return fail(OSLAM_E_INVALID, "this model lost its key tables with its database: it can only be destroyed");
        if (any && ms[h]->dev != dev) return fail(OSLAM_E_INVALID, "the models live on different devices");
        dev = ms[h]->dev;
        any = 1;
    }
    if (dev < 0) {
        rc = oslam_pick_device(0, &dev);
        if (rc != OSLAM_OK) return rc;
    }
    off_rho = align256(sizeof *hm * H);
    off_cnt = off_rho + align256(sizeof(float) * H);
    up_bytes = off_cnt + align256(sizeof(uint32_t) * 2 * H);     /* drawn[H], pixels[H] */
    off_keys = up_bytes;
    up = (char *)calloc(1, up_bytes);
    cnt = (uint32_t *)calloc(2 * H, sizeof *cnt);
    r = (oslam_render *)calloc(1, sizeof *r);
    if (!up || !cnt || !r) { free(up); free(cnt); free(r); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    hm = (oslamk_verify_member *)up;
    rho = (float *)(up + off_rho);
    for (h = 0; h < H; h++)
        if (!oslam_is_zero_pose(T + 16 * h)) {
            oslam_verify_set_member(&hm[h], ms[h], T + 16 * h, p->depth_tol);
            rho[h] = (float)((double)p->footprint * (double)ms[h]->d_dist);
            if (hm[h].n_blocks > max_blocks) max_blocks = hm[h].n_blocks;
        }
    r->dev = dev;
    r->n_hyp = H;
    if (hipSetDevice(dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    rc = oslam_view_new(dev, width, height, cam, &r->view);
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipMalloc((void **)&r->d_labels, align256(sizeof(int32_t) * n_pix) + sizeof(float) * H));
    r->d_tol = (float *)((char *)r->d_labels + align256(sizeof(int32_t) * n_pix));
    KCHK(oslam_dev_alloc((void **)&d_up, off_keys + sizeof(uint64_t) * n_pix));
    HIPCHK(hipMemcpyAsync(d_up, up, up_bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(d_up + off_keys, 0xff, sizeof(uint64_t) * n_pix, (hipStream_t)stream));
    if (max_blocks) {                           /* every hypothesis skipped: nothing to splat, the render is empty */
        KCHK(oslamk_render_splat(&r->view->k, (const oslamk_verify_member *)d_up, (const float *)(d_up + off_rho),
                                 (uint32_t)H, (uint32_t)max_blocks, (int)p->max_splat, p->keep_back,
                                 (unsigned long long *)(d_up + off_keys), (uint32_t *)(d_up + off_cnt), stream));
        launches++;
    }
    KCHK(oslamk_render_resolve((const unsigned long long *)(d_up + off_keys), width, height,
                               (const oslamk_verify_member *)d_up, (uint32_t)H, r->view->d_z, r->d_labels, r->d_tol,
                               (uint32_t *)(d_up + off_cnt) + H, stream));
    launches++;
    HIPCHK(hipMemcpyAsync(cnt, d_up + off_cnt, sizeof(uint32_t) * 2 * H, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (res) {
        const float ms_total = (float)(now_ms() - t0);
        for (h = 0; h < H; h++) {
            res[h].drawn = cnt[h];
            res[h].pixels = cnt[H + h];
            res[h].launches = launches;
            res[h].ms_total = ms_total;
        }
    }
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);    /* nothing may still use the blocks */
    if (d_up) oslam_dev_free(d_up);
    free(up);
    free(cnt);
    if (rc != OSLAM_OK) release(r);
    else *out = r;
    return rc;
}

int oslam_render_create(oslam_model *const *models, const float *T, size_t H, const oslam_camera *cam, int width,
                        int height, const oslam_render_params *rp, oslam_render **out, oslam_render_result *res)
{
    oslam_render_params p;
    int rc;
    if (out) *out = NULL;
    if (!models || !T || !cam || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = render_check(models, T, H, cam, width, height, rp, &p);
    if (rc != OSLAM_OK) return rc;
    if (res) memset(res, 0, sizeof *res * H);
    return render_members(models, T, H, -1, cam, width, height, &p, out, res);
}

int oslam_db_render(oslam_db *db, const uint32_t *member, const float *T, size_t H, const oslam_camera *cam, int width,
                    int height, const oslam_render_params *rp, oslam_render **out, oslam_render_result *res)
{
    oslam_render_params p;
    oslam_model **ms;
    size_t h;
    int rc;
    if (out) *out = NULL;
    if (!db || !member || !T || !cam || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = render_check(NULL, T, H, cam, width, height, rp, &p);    /* the members' models are not looked up yet */
    if (rc != OSLAM_OK) return rc;
    for (h = 0; h < H; h++)
        if (member[h] >= db->n) return fail(OSLAM_E_INVALID, "member index outside the database");
    if (res) memset(res, 0, sizeof *res * H);
    ms = (oslam_model **)malloc(sizeof *ms * H);
    if (!ms) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (h = 0; h < H; h++) ms[h] = db->models[member[h]];
    rc = render_members(ms, T, H, db->dev, cam, width, height, &p, out, res);
    free(ms);
    return rc;
}

int oslam_render_view(oslam_render *r, oslam_view **view_out)
{
    if (view_out) *view_out = NULL;
    if (!r || !view_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!r->view) return fail(OSLAM_E_INVALID, "the render has no view");
    *view_out = r->view;
    return OSLAM_OK;
}

int oslam_render_labels(oslam_render *r, int32_t *labels_out)
{
    int rc = OSLAM_OK;
    if (!r || !labels_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!r->view || !r->d_labels) return fail(OSLAM_E_INVALID, "the render has no labels");
    if (hipSetDevice(r->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    HIPCHK(hipMemcpy(labels_out, r->d_labels, sizeof(int32_t) * (size_t)r->view->k.w * (size_t)r->view->k.h,
                     hipMemcpyDeviceToHost));
done:
    return rc;
}

int oslam_render_destroy(oslam_render *r)
{
    if (!r) return fail(OSLAM_E_INVALID, "render is NULL");
    release(r);
    return OSLAM_OK;
}

int oslam_view_info(const oslam_view *v, oslam_camera *cam_out, int *width_out, int *height_out)
{
    if (!v || !cam_out || !width_out || !height_out) return fail(OSLAM_E_INVALID, "NULL argument");
    oslam_view_camera(v, cam_out);
    *width_out = v->k.w;
    *height_out = v->k.h;
    return OSLAM_OK;
}

/* bit for bit: -0.0f and 0.0f differ, as the kernels' arithmetic on them may */
static int same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }

int oslam_view_mask(const oslam_view *v, const oslam_render *r, const oslam_mask_params *mp, oslam_view **out,
                    oslam_mask_result *res)
{
    int rc = OSLAM_OK;
    const double t0 = now_ms();
    oslam_mask_params p;
    oslam_camera cam;
    oslam_view *o = NULL;
    const oslamk_view *a, *b;
    uint32_t *d_cnt = NULL, cnt[3] = {0, 0, 0};
    void *stream = oslam_stream();

    if (out) *out = NULL;
    if (!v || !r || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (mp) p = *mp;
    else oslam_mask_params_default(&p);
    if (p.mode != OSLAM_MASK_REMOVE && p.mode != OSLAM_MASK_KEEP) return fail(OSLAM_E_INVALID, "mode must be OSLAM_MASK_REMOVE or OSLAM_MASK_KEEP");
    if (p.dilate > OSLAM_MASK_MAX_DILATE) return fail(OSLAM_E_INVALID, "dilate above OSLAM_MASK_MAX_DILATE");
    if (p.only < -1) return fail(OSLAM_E_INVALID, "only must be -1 or a hypothesis index");
    if (!r->view || !r->d_labels) return fail(OSLAM_E_INVALID, "the render has no images");
    if (p.only >= 0 && (size_t)p.only >= r->n_hyp) return fail(OSLAM_E_INVALID, "only names no hypothesis of the render");
    a = &v->k;
    b = &r->view->k;
    if (v->dev != r->dev) return fail(OSLAM_E_INVALID, "view and render live on different devices");
    if (a->w != b->w || a->h != b->h) return fail(OSLAM_E_INVALID, "view and render differ in size");
    if (!same_bits(a->fx, b->fx) || !same_bits(a->fy, b->fy) || !same_bits(a->cx, b->cx) || !same_bits(a->cy, b->cy) ||
        !same_bits(a->z_min, b->z_min) || !same_bits(a->z_max, b->z_max))
        return fail(OSLAM_E_INVALID, "view and render differ in camera");
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_view_camera(v, &cam);
    rc = oslam_view_new(v->dev, a->w, a->h, &cam, &o);
    if (rc != OSLAM_OK) return rc;
    KCHK(oslam_dev_alloc((void **)&d_cnt, 256));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof cnt, (hipStream_t)stream));
    KCHK(oslamk_view_mask(a, b->z, r->d_labels, r->d_tol, p.mode, (int)p.dilate, p.only, o->d_z, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (res) {
        memset(res, 0, sizeof *res);
        res->valid_in = cnt[0];
        res->object_pixels = cnt[1];
        res->valid_out = cnt[2];
        res->launches = 1;
        res->ms_total = (float)(now_ms() - t0);
    }
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    if (d_cnt) oslam_dev_free(d_cnt);
    if (rc != OSLAM_OK) oslam_view_destroy(o);
    else *out = o;
    return rc;
}
