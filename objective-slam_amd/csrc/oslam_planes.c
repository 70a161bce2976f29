/*
 * oslam_planes.c -- the dominant planes of a view, and views without them (include/oslam.h at oslam_view_planes): the
 * host side of the kernels in oslam_planes.hip.  A planes object owns the label image on the device and host copies of
 * the plane records and of the rounds' counts and moments.  A call checks its arguments, builds the view's maps when they
 * do not exist yet, presets the labels and zeroes the call's block with two memsets, enqueues the four kernels of every
 * round (oslamk_planes_find) and reads the block back with one host wait: the end of the search is decided on the device.
 * oslam_view_remove_planes is one memset, k_planes_mask and one copy back.
 */
#include <math.h>

#include "oslam_internal.h"

int oslam_planes_params_default(oslam_planes_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->dist_tol = 0.02f;
    p->min_normal_dot = 0.9f;
    p->label_min_dot = 0.0f;
    p->max_planes = 4;
    p->min_pixels = 0;
    return OSLAM_OK;
}

static int check_params(const oslam_planes_params *pp, oslam_planes_params *p)
{
    if (pp) *p = *pp;
    else oslam_planes_params_default(p);
    if (!isfinite(p->dist_tol) || !(p->dist_tol > 0.0f) || !isfinite(16.0f / p->dist_tol))
        return fail(OSLAM_E_INVALID, "dist_tol must be finite and > 0 (and 16 / dist_tol a finite float)");
    if (!(p->min_normal_dot >= -1.0f && p->min_normal_dot <= 1.0f) || !(p->label_min_dot >= -1.0f && p->label_min_dot <= 1.0f))
        return fail(OSLAM_E_INVALID, "min_normal_dot and label_min_dot must lie in [-1, 1]");
    if (p->max_planes < 1 || p->max_planes > OSLAM_PLANES_MAX) return fail(OSLAM_E_INVALID, "max_planes must lie in 1..OSLAM_PLANES_MAX");
    return OSLAM_OK;
}

static void release(oslam_planes *p)
{
    /* every call that read the labels ended with a synchronisation of its stream */
    if (p->d_labels && hipSetDevice(p->dev) == hipSuccess) (void)hipFree(p->d_labels);
    free(p);
}

int oslam_view_planes(oslam_view *v, const oslam_planes_params *pp, oslam_planes **out, oslam_planes_result *res)
{
    int rc = OSLAM_OK, built = 0, locked = 0;
    const double t0 = now_ms();
    oslam_planes_params p;
    oslam_planes *o = NULL;
    oslamk_planes_block *h_blk = NULL, *d_blk = NULL;
    oslamk_planes_args ka;
    size_t n_pix;
    uint32_t r, k;
    void *stream = oslam_stream();

    if (out) *out = NULL;
    if (!v || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_params(pp, &p);
    if (rc != OSLAM_OK) return rc;
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    if (v->k.w < 1 || v->k.h < 1 || !v->d_z) return fail(OSLAM_E_INVALID, "the view has no image");
    n_pix = (size_t)v->k.w * (size_t)v->k.h;
    o = (oslam_planes *)calloc(1, sizeof *o);
    h_blk = (oslamk_planes_block *)malloc(sizeof *h_blk);
    if (!o || !h_blk) { free(o); free(h_blk); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    o->dev = v->dev;
    o->w = v->k.w;
    o->h = v->k.h;
    o->max_planes = p.max_planes;
    /* takes its turn with the calls on volumes and views: the shared stream, the kept scratch blocks, the maps */
    oslam_volume_lock();
    locked = 1;
    rc = oslam_track_view_maps(v, &built);
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipMalloc((void **)&o->d_labels, sizeof(int32_t) * n_pix));
    KCHK(oslam_dev_alloc((void **)&d_blk, sizeof *d_blk));
    HIPCHK(hipMemsetAsync(o->d_labels, 0xff, sizeof(int32_t) * n_pix, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(d_blk, 0, sizeof *d_blk, (hipStream_t)stream));
    memset(&ka, 0, sizeof ka);
    ka.v = v->k;
    ka.maps = v->d_maps;
    ka.labels = o->d_labels;
    ka.blk = d_blk;
    ka.dist_tol = p.dist_tol;
    ka.min_normal_dot = p.min_normal_dot;
    ka.label_min_dot = p.label_min_dot;
    ka.scale = 16.0f / p.dist_tol;
    ka.min_pixels = p.min_pixels ? p.min_pixels : (uint32_t)(n_pix / 50);
    ka.line_ratio = (double)0.01f;
    KCHK(oslamk_planes_find(&ka, p.max_planes, stream));
    HIPCHK(hipMemcpyAsync(h_blk, d_blk, sizeof *h_blk, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));

    o->n_planes = h_blk->n_planes;
    memcpy(o->planes, h_blk->rec, sizeof o->planes);
    memcpy(o->counts, h_blk->counts, sizeof o->counts);
    memcpy(o->moments, h_blk->moments, sizeof o->moments);
    if (res) {
        memset(res, 0, sizeof *res);
        res->n_planes = o->n_planes;
        res->valid_in = h_blk->valid_in;
        for (r = 0, k = 0; r < o->n_planes; r++) k += o->planes[r].pixels;
        res->labelled = k;
        res->launches = 4 * p.max_planes + (built ? 1u : 0u);
        res->ms_total = (float)(now_ms() - t0);
    }
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    if (d_blk) oslam_dev_free(d_blk);
    if (locked) oslam_volume_unlock();
    free(h_blk);
    if (rc != OSLAM_OK) release(o);
    else *out = o;
    return rc;
}

int oslam_planes_get(const oslam_planes *p, oslam_plane *planes_out, size_t cap, size_t *n_out)
{
    if (!p || !n_out || (cap && !planes_out)) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = p->n_planes;
    if (p->n_planes > cap) return fail(OSLAM_E_LIMIT, "output capacity too small");
    if (p->n_planes) memcpy(planes_out, p->planes, sizeof(oslam_plane) * p->n_planes);
    return OSLAM_OK;
}

int oslam_planes_labels(oslam_planes *p, int32_t *labels_out)
{
    int rc = OSLAM_OK;
    if (!p || !labels_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!p->d_labels) return fail(OSLAM_E_INVALID, "the planes object has no labels");
    if (hipSetDevice(p->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    HIPCHK(hipMemcpy(labels_out, p->d_labels, sizeof(int32_t) * (size_t)p->w * (size_t)p->h, hipMemcpyDeviceToHost));
done:
    return rc;
}

int oslam_planes_rounds(oslam_planes *p, uint32_t *counts_out, int64_t *moments_out)
{
    if (!p || (!counts_out && !moments_out)) return fail(OSLAM_E_INVALID, "NULL argument");
    if (p->max_planes < 1 || p->max_planes > OSLAM_PLANES_MAX) return fail(OSLAM_E_INVALID, "not a planes object");
    if (counts_out) memcpy(counts_out, p->counts, sizeof(uint32_t) * OSLAMK_PLANES_CAND * p->max_planes);
    if (moments_out) memcpy(moments_out, p->moments, sizeof(int64_t) * 10 * p->max_planes);
    return OSLAM_OK;
}

int oslam_view_remove_planes(const oslam_view *v, const oslam_planes *p, int mode, int32_t only, oslam_view **out,
                             oslam_mask_result *res)
{
    int rc = OSLAM_OK;
    const double t0 = now_ms();
    oslam_camera cam;
    oslam_view *o = NULL;
    uint32_t *d_cnt = NULL, cnt[3] = {0, 0, 0};
    void *stream = oslam_stream();

    if (out) *out = NULL;
    if (!v || !p || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (mode != OSLAM_MASK_REMOVE && mode != OSLAM_MASK_KEEP) return fail(OSLAM_E_INVALID, "mode must be OSLAM_MASK_REMOVE or OSLAM_MASK_KEEP");
    if (only < -1) return fail(OSLAM_E_INVALID, "only must be -1 or a plane index");
    if (v->dev != p->dev) return fail(OSLAM_E_INVALID, "view and planes live on different devices");
    if (v->k.w != p->w || v->k.h != p->h) return fail(OSLAM_E_INVALID, "view and planes differ in size");
    if (only >= 0 && (uint32_t)only >= p->n_planes) return fail(OSLAM_E_INVALID, "only names no plane of the object");
    if (!p->d_labels || !v->d_z) return fail(OSLAM_E_INVALID, "the view or the planes object has no image");
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_view_camera(v, &cam);
    rc = oslam_view_new(v->dev, v->k.w, v->k.h, &cam, &o);
    if (rc != OSLAM_OK) return rc;
    KCHK(oslam_dev_alloc((void **)&d_cnt, 256));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof cnt, (hipStream_t)stream));
    KCHK(oslamk_planes_mask(&v->k, p->d_labels, mode, only, o->d_z, d_cnt, stream));
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

int oslam_planes_destroy(oslam_planes *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "planes is NULL");
    release(p);
    return OSLAM_OK;
}
