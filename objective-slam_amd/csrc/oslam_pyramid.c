/*
 * oslam_pyramid.c -- depth image pyramids (include/oslam.h at oslam_pyramid_create): the host side of the kernel in
 * oslam_pyramid.hip.  A pyramid borrows its base view as level 0 and owns the coarser levels, each a genuine oslam_view
 * (oslam_view_new: a z image and a camera; its maps are built on first use by the tracking stage's path).  Creating one
 * enqueues one k_pyr_down per coarser level back to back and waits once.  Coarse-to-fine camera motion over two pyramids is
 * oslam_pyramid_egomotion in oslam_ego.c; frame-to-model tracking over them is oslam_volume_track_pyramid in
 * oslam_volume.c.
 */
#include <math.h>

#include "oslam_internal.h"

int oslam_pyramid_params_default(oslam_pyramid_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->n_levels = 3;
    p->depth_band = 0.09f;
    return OSLAM_OK;
}

int oslam_pyramid_check_params(const oslam_pyramid_params *pp, oslam_pyramid_params *out)
{
    if (pp) *out = *pp;
    else oslam_pyramid_params_default(out);
    if (out->n_levels < 1 || out->n_levels > 3) return fail(OSLAM_E_INVALID, "n_levels must lie in 1..3");
    if (!isfinite(out->depth_band) || !(out->depth_band > 0.0f)) return fail(OSLAM_E_INVALID, "depth_band must be finite and > 0");
    return OSLAM_OK;
}

/* gives back the levels the pyramid owns; every call that read them ended with a synchronisation of its stream */
static void release(oslam_pyramid *pyr)
{
    unsigned k;
    for (k = 1; k < pyr->n_levels; k++)
        if (pyr->level[k]) oslam_view_destroy(pyr->level[k]);
    free(pyr);
}

int oslam_pyramid_create(oslam_view *base, const oslam_pyramid_params *pp, oslam_pyramid **out)
{
    int rc;
    unsigned k;
    oslam_pyramid_params p;
    oslam_pyramid *pyr;
    void *stream = oslam_stream();
    if (out) *out = NULL;
    if (!base || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_pyramid_check_params(pp, &p);
    if (rc != OSLAM_OK) return rc;
    if (hipSetDevice(base->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    pyr = (oslam_pyramid *)calloc(1, sizeof *pyr);
    if (!pyr) return fail(OSLAM_E_NOMEM, "host allocation failed");
    pyr->dev = base->dev;
    pyr->n_levels = p.n_levels;
    pyr->level[0] = base;
    for (k = 1; k < p.n_levels; k++) {
        const oslam_view *f = pyr->level[k - 1];
        oslam_camera cam;
        oslam_view_camera(f, &cam);
        cam.fx *= 0.5f;
        cam.fy *= 0.5f;
        cam.cx *= 0.5f;
        cam.cy *= 0.5f;
        cam.max_jump *= 2.0f;
        rc = oslam_view_new(base->dev, (f->k.w + 1) / 2, (f->k.h + 1) / 2, &cam, &pyr->level[k]);
        if (rc != OSLAM_OK) goto done;
        KCHK(oslamk_pyr_down(&f->k, p.depth_band, pyr->level[k]->d_z, stream));
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
done:
    if (rc != OSLAM_OK) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        release(pyr);
        return rc;
    }
    *out = pyr;
    return OSLAM_OK;
}

int oslam_pyramid_destroy(oslam_pyramid *pyr)
{
    if (!pyr) return fail(OSLAM_E_INVALID, "pyramid is NULL");
    release(pyr);
    return OSLAM_OK;
}

int oslam_pyramid_level(oslam_pyramid *pyr, unsigned k, oslam_view **view_out)
{
    if (view_out) *view_out = NULL;
    if (!pyr || !view_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (k >= 3 || k >= pyr->n_levels) return fail(OSLAM_E_INVALID, "the pyramid has no such level");
    *view_out = pyr->level[k];
    return OSLAM_OK;
}
