/*
 * oslam_bilateral.c -- the bilateral filter of a view's depth image (include/oslam.h at oslam_view_bilateral): the host
 * side of the kernel in oslam_bilateral.hip.  The result is a genuine oslam_view (oslam_view_new: a z image and the
 * input's camera; its maps are built on first use by the tracking stage's path).  A call is one memset of the two
 * counters, k_bilateral, one small copy back and one host wait.
 */
#include <math.h>

#include "oslam_gauss_table.h"
#include "oslam_internal.h"

int oslam_bilateral_params_default(oslam_bilateral_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->radius = 6;
    p->sigma_space = 4.5f;
    p->sigma_depth = 0.03f;
    return OSLAM_OK;
}

int oslam_gauss_table(unsigned i, float *w_out)
{
    static const uint32_t bits[OSLAM_GAUSS_N] = {OSLAM_GAUSS_BITS_FLAT};
    if (i >= OSLAM_GAUSS_N || !w_out) return fail(OSLAM_E_INVALID, "the index must lie in 0..287 and the output must be given");
    memcpy(w_out, &bits[i], sizeof *w_out);
    return OSLAM_OK;
}

int oslam_view_bilateral(const oslam_view *v, const oslam_bilateral_params *bp, oslam_view **out, oslam_bilateral_result *res)
{
    int rc = OSLAM_OK;
    const double t0 = now_ms();
    oslam_bilateral_params p;
    oslam_camera cam;
    oslam_view *o = NULL;
    uint32_t *d_cnt = NULL, cnt[2] = {0, 0};
    float inv_s, inv_r;
    void *stream = oslam_stream();

    if (out) *out = NULL;
    if (!v || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (bp) p = *bp;
    else oslam_bilateral_params_default(&p);
    if (p.radius < 1 || p.radius > OSLAM_BILATERAL_MAX_RADIUS) return fail(OSLAM_E_INVALID, "radius must lie in 1..OSLAM_BILATERAL_MAX_RADIUS");
    if (!isfinite(p.sigma_space) || !(p.sigma_space > 0.0f)) return fail(OSLAM_E_INVALID, "sigma_space must be finite and > 0");
    if (!isfinite(p.sigma_depth) || !(p.sigma_depth > 0.0f)) return fail(OSLAM_E_INVALID, "sigma_depth must be finite and > 0");
    inv_s = (float)(1.0 / ((double)p.sigma_space * (double)p.sigma_space));
    inv_r = (float)(1.0 / ((double)p.sigma_depth * (double)p.sigma_depth));
    if (!isfinite(inv_s) || !isfinite(inv_r)) return fail(OSLAM_E_INVALID, "a sigma so small that 1 / sigma^2 is not a finite float");
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_view_camera(v, &cam);
    rc = oslam_view_new(v->dev, v->k.w, v->k.h, &cam, &o);
    if (rc != OSLAM_OK) return rc;
    KCHK(oslam_dev_alloc((void **)&d_cnt, 256));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof cnt, (hipStream_t)stream));
    KCHK(oslamk_bilateral(&v->k, (int)p.radius, inv_s, inv_r, o->d_z, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (res) {
        memset(res, 0, sizeof *res);
        res->valid = cnt[0];
        res->taps = cnt[1];
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
