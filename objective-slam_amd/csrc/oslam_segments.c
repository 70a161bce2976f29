/*
 * oslam_segments.c -- the connected regions of a view (include/oslam.h at oslam_view_segments): the host side of the
 * kernels in oslam_segments.hip.  A segments object owns the root image and the label image on the device and a host
 * copy of the segment records.  A call checks its arguments, zeroes the call's block and the count array with two
 * memsets, enqueues the six kernels (oslamk_segments_find) and reads the head of the block back with one host wait; the
 * records' centroids and sides are made here from the integers the kernels left.  oslam_view_select_segments is one
 * memset, k_planes_mask on the label image and one copy back.
 */
#include <math.h>
#include <stdio.h>

#include "oslam_internal.h"

int oslam_segments_params_default(oslam_segments_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->max_step = 0.0f;
    p->rel_step = 0.0f;
    p->min_pixels = 0;
    p->max_segments = 16;
    return OSLAM_OK;
}

static int check_params(const oslam_segments_params *sp, oslam_segments_params *p)
{
    if (sp) *p = *sp;
    else oslam_segments_params_default(p);
    if (!isfinite(p->max_step) || p->max_step < 0.0f) return fail(OSLAM_E_INVALID, "max_step must be finite and >= 0");
    if (!isfinite(p->rel_step) || p->rel_step < 0.0f) return fail(OSLAM_E_INVALID, "rel_step must be finite and >= 0");
    if (p->max_segments < 1 || p->max_segments > OSLAM_SEGMENTS_MAX)
        return fail(OSLAM_E_INVALID, "max_segments must lie in 1..OSLAM_SEGMENTS_MAX");
    return OSLAM_OK;
}

static void release(oslam_segments *s)
{
    /* every call that read the images ended with a synchronisation of its stream */
    if (!s) return;
    if ((s->d_roots || s->d_labels) && hipSetDevice(s->dev) == hipSuccess) {
        if (s->d_roots) (void)hipFree(s->d_roots);
        if (s->d_labels) (void)hipFree(s->d_labels);
    }
    free(s);
}

/* the record of one segment from the integers of the device */
static void make_record(oslam_segment *o, const oslamk_seg_acc *a, int w, int h)
{
    int k;
    memset(o, 0, sizeof *o);
    o->pixels = a->pixels;
    o->root = a->root;
    o->u0 = (uint16_t)a->u0;
    o->v0 = (uint16_t)a->v0;
    o->u1 = (uint16_t)a->u1;
    o->v1 = (uint16_t)a->v1;
    for (k = 0; k < 3; k++)
        o->centroid[k] = a->n ? (float)(((double)(int64_t)a->s[k] / (double)a->n) / 8192.0) : 0.0f;
    o->sides = (a->u0 == 0 ? 1u : 0u) | (a->v0 == 0 ? 2u : 0u) | (a->u1 == (uint32_t)w - 1u ? 4u : 0u) |
               (a->v1 == (uint32_t)h - 1u ? 8u : 0u);
}

int oslam_view_segments(const oslam_view *v, const oslam_planes *planes, const oslam_segments_params *sp, oslam_segments **out,
                        oslam_segments_result *res)
{
    int rc = OSLAM_OK, locked = 0;
    const double t0 = now_ms();
    const size_t head = offsetof(oslamk_seg_block, cand);
    oslam_segments_params p;
    oslam_segments *o = NULL;
    oslamk_seg_block *h_blk = NULL, *d_blk = NULL;
    uint32_t *d_tcount = NULL, *d_count = NULL;
    oslamk_seg_args ka;
    size_t n_pix;
    uint32_t k, labelled = 0;
    char msg[160];
    void *stream = oslam_stream();

    if (out) *out = NULL;
    if (!v || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_params(sp, &p);
    if (rc != OSLAM_OK) return rc;
    if (p.max_step == 0.0f) p.max_step = v->max_jump;
    if (!isfinite(p.max_step) || !(p.max_step > 0.0f)) return fail(OSLAM_E_INVALID, "max_step is 0 and the view has no max_jump");
    if (planes) {
        if (v->dev != planes->dev) return fail(OSLAM_E_INVALID, "view and planes live on different devices");
        if (v->k.w != planes->w || v->k.h != planes->h) return fail(OSLAM_E_INVALID, "view and planes differ in size");
    }
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    if (v->k.w < 1 || v->k.h < 1 || !v->d_z || (planes && !planes->d_labels)) return fail(OSLAM_E_INVALID, "the view or the planes object has no image");
    n_pix = (size_t)v->k.w * (size_t)v->k.h;
    o = (oslam_segments *)calloc(1, sizeof *o);
    h_blk = (oslamk_seg_block *)malloc(head);
    if (!o || !h_blk) { free(o); free(h_blk); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    o->dev = v->dev;
    o->w = v->k.w;
    o->h = v->k.h;
    /* takes its turn with the calls on volumes and views: the shared stream and the kept scratch blocks */
    oslam_volume_lock();
    locked = 1;
    HIPCHK(hipMalloc((void **)&o->d_roots, sizeof(uint32_t) * n_pix));
    HIPCHK(hipMalloc((void **)&o->d_labels, sizeof(int32_t) * n_pix));
    KCHK(oslam_dev_alloc((void **)&d_blk, sizeof *d_blk));
    KCHK(oslam_dev_alloc((void **)&d_tcount, sizeof(uint32_t) * n_pix));
    KCHK(oslam_dev_alloc((void **)&d_count, sizeof(uint32_t) * n_pix));
    HIPCHK(hipMemsetAsync(d_blk, 0, head, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(d_count, 0, sizeof(uint32_t) * n_pix, (hipStream_t)stream));
    memset(&ka, 0, sizeof ka);
    ka.v = v->k;
    ka.plane_labels = planes ? planes->d_labels : NULL;
    ka.L = o->d_roots;
    ka.tcount = d_tcount;
    ka.count = d_count;
    ka.labels = o->d_labels;
    ka.blk = d_blk;
    ka.max_step = p.max_step;
    ka.rel_step = p.rel_step;
    ka.min_pixels = p.min_pixels ? p.min_pixels : (uint32_t)(n_pix / 1000 > 1 ? n_pix / 1000 : 1);
    ka.max_segments = p.max_segments;
    KCHK(oslamk_segments_find(&ka, stream));
    HIPCHK(hipMemcpyAsync(h_blk, d_blk, head, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));

    if (h_blk->n_candidates > OSLAMK_SEG_CAND) {
        if (res) {
            res->n_components = h_blk->n_components;
            res->n_candidates = h_blk->n_candidates;
        }
        snprintf(msg, sizeof msg, "%u of %u components pass min_pixels: more than OSLAM_SEGMENTS_CANDIDATES",
                 (unsigned)h_blk->n_candidates, (unsigned)h_blk->n_components);
        rc = fail(OSLAM_E_LIMIT, msg);
        goto done;
    }
    o->n_segments = h_blk->n_candidates < p.max_segments ? h_blk->n_candidates : p.max_segments;
    for (k = 0; k < o->n_segments; k++) {
        make_record(&o->seg[k], &h_blk->acc[k], o->w, o->h);
        labelled += o->seg[k].pixels;
    }
    if (res) {
        memset(res, 0, sizeof *res);
        res->n_segments = o->n_segments;
        res->n_components = h_blk->n_components;
        res->n_candidates = h_blk->n_candidates;
        res->valid_in = h_blk->valid_in;
        res->labelled = labelled;
        res->launches = OSLAM_SEGMENTS_LAUNCHES;
        res->ms_total = (float)(now_ms() - t0);
    }
done:
    if (rc == OSLAM_E_DEVICE) (void)hipStreamSynchronize((hipStream_t)stream);
    if (d_count) oslam_dev_free(d_count);
    if (d_tcount) oslam_dev_free(d_tcount);
    if (d_blk) oslam_dev_free(d_blk);
    if (locked) oslam_volume_unlock();
    free(h_blk);
    if (rc != OSLAM_OK) release(o);
    else *out = o;
    return rc;
}

int oslam_segments_get(const oslam_segments *s, oslam_segment *out, size_t cap, size_t *n_out)
{
    if (!s || !n_out || (cap && !out)) return fail(OSLAM_E_INVALID, "NULL argument");
    if (s->n_segments > OSLAM_SEGMENTS_MAX) return fail(OSLAM_E_INVALID, "not a segments object");
    *n_out = s->n_segments;
    if (s->n_segments > cap) return fail(OSLAM_E_LIMIT, "output capacity too small");
    if (s->n_segments) memcpy(out, s->seg, sizeof(oslam_segment) * s->n_segments);
    return OSLAM_OK;
}

static int copy_image(oslam_segments *s, const void *d_src, void *dst)
{
    int rc = OSLAM_OK;
    if (!s || !dst) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!d_src) return fail(OSLAM_E_INVALID, "the segments object has no image");
    if (hipSetDevice(s->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    HIPCHK(hipMemcpy(dst, d_src, sizeof(int32_t) * (size_t)s->w * (size_t)s->h, hipMemcpyDeviceToHost));
done:
    return rc;
}

int oslam_segments_labels(oslam_segments *s, int32_t *labels_out)
{
    return copy_image(s, s ? s->d_labels : NULL, labels_out);
}

/* the device's "not in" is all ones: -1 as int32 */
int oslam_segments_roots(oslam_segments *s, int32_t *roots_out)
{
    return copy_image(s, s ? s->d_roots : NULL, roots_out);
}

int oslam_view_select_segments(const oslam_view *v, const oslam_segments *s, int mode, int32_t only, oslam_view **out,
                               oslam_mask_result *res)
{
    int rc = OSLAM_OK;
    const double t0 = now_ms();
    oslam_camera cam;
    oslam_view *o = NULL;
    uint32_t *d_cnt = NULL, cnt[3] = {0, 0, 0};
    void *stream = oslam_stream();

    if (out) *out = NULL;
    if (!v || !s || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (mode != OSLAM_MASK_REMOVE && mode != OSLAM_MASK_KEEP) return fail(OSLAM_E_INVALID, "mode must be OSLAM_MASK_REMOVE or OSLAM_MASK_KEEP");
    if (only < -1) return fail(OSLAM_E_INVALID, "only must be -1 or a segment index");
    if (v->dev != s->dev) return fail(OSLAM_E_INVALID, "view and segments live on different devices");
    if (v->k.w != s->w || v->k.h != s->h) return fail(OSLAM_E_INVALID, "view and segments differ in size");
    if (only >= 0 && (uint32_t)only >= s->n_segments) return fail(OSLAM_E_INVALID, "only names no segment of the object");
    if (!s->d_labels || !v->d_z) return fail(OSLAM_E_INVALID, "the view or the segments object has no image");
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_view_camera(v, &cam);
    rc = oslam_view_new(v->dev, v->k.w, v->k.h, &cam, &o);
    if (rc != OSLAM_OK) return rc;
    KCHK(oslam_dev_alloc((void **)&d_cnt, 256));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof cnt, (hipStream_t)stream));
    /* the label image fits k_planes_mask as it stands: object = label >= 0, or == only */
    KCHK(oslamk_planes_mask(&v->k, s->d_labels, mode, only, o->d_z, d_cnt, stream));
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

int oslam_segments_destroy(oslam_segments *s)
{
    if (!s) return fail(OSLAM_E_INVALID, "segments is NULL");
    release(s);
    return OSLAM_OK;
}
