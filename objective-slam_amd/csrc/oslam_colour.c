/*
 * oslam_colour.c -- colour next to the TSDF (include/oslam.h at oslam_volume_integrate_colour): the host side of the
 * kernels in oslam_colour.hip.  A view can carry a registered colour image and a volume a colour buffer of one word per
 * voxel; an integration with colour is oslam_volume_integrate plus one launch in the same call (the body is
 * oslam_volume_integrate_views of oslam_volume.c), and the colour comes back at points (oslam_volume_colours) or into a
 * view's colour image (oslam_volume_paint_view).  The shift of the colour buffer is in oslam_window.c with the TSDF's.
 * Every call here that reads or writes a colour image or a colour buffer holds the volume lock.
 */
#include <math.h>

#include "oslam_internal.h"

/* ---- a colour image on a view ---- */
int oslam_view_has_colour(const oslam_view *v) { return v && v->d_colour ? 1 : 0; }

void oslam_colour_release_view(oslam_view *v)
{
    if (v->d_colour) (void)hipFree(v->d_colour);
    v->d_colour = NULL;
}

int oslam_view_set_colour(oslam_view *v, const uint8_t *rgb, size_t row_stride_bytes, const uint8_t *valid)
{
    int rc = OSLAM_OK, fresh = 0;
    size_t w, h, x, y, stride;
    uint32_t *words = NULL, *d_new = NULL;
    if (!v || !rgb) return fail(OSLAM_E_INVALID, "NULL argument");
    w = (size_t)v->k.w;
    h = (size_t)v->k.h;
    stride = row_stride_bytes ? row_stride_bytes : 3 * w;
    if (stride < 3 * w) return fail(OSLAM_E_INVALID, "row_stride_bytes is smaller than a row of the image");
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    words = (uint32_t *)malloc(sizeof(uint32_t) * (w * h + 1));
    if (!words) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (y = 0; y < h; y++) {
        const uint8_t *row = rgb + y * stride;
        for (x = 0; x < w; x++) {
            const int has = !valid || valid[y * w + x];
            words[y * w + x] = has ? (uint32_t)row[3 * x] | (uint32_t)row[3 * x + 1] << 8 | (uint32_t)row[3 * x + 2] << 16 | 0xff000000u : 0u;
        }
    }
    oslam_volume_lock();
    d_new = v->d_colour;
    if (!d_new) {
        /* the image lives as long as the view: its own block, as the z image */
        HIPCHK(hipMalloc((void **)&d_new, sizeof(uint32_t) * w * h));
        fresh = 1;
    }
    HIPCHK(hipMemcpy(d_new, words, sizeof(uint32_t) * w * h, hipMemcpyHostToDevice));
    v->d_colour = d_new;
    fresh = 0;
done:
    if (fresh && d_new) (void)hipFree(d_new);
    oslam_volume_unlock();
    free(words);
    return rc;
}

int oslam_view_colour(oslam_view *v, uint32_t *rgba_out)
{
    int rc = OSLAM_OK;
    if (!v || !rgba_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!v->d_colour) return fail(OSLAM_E_INVALID, "the view has no colour");
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    HIPCHK(hipMemcpy(rgba_out, v->d_colour, sizeof(uint32_t) * (size_t)v->k.w * (size_t)v->k.h, hipMemcpyDeviceToHost));
done:
    oslam_volume_unlock();
    return rc;
}

/* ---- a colour buffer on a volume ---- */
int oslam_colour_params_default(oslam_colour_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->max_weight = 8;         /* the integer mean moves only when |pixel - mean| >= (wc + 1) / 2: DESIGN.md 7t */
    p->band = 0.0f;
    return OSLAM_OK;
}

int oslam_volume_colour_enable(oslam_volume *vol, const oslam_colour_params *cp)
{
    int rc = OSLAM_OK;
    oslam_colour_params p;
    uint32_t *words = NULL;
    if (!vol) return fail(OSLAM_E_INVALID, "volume is NULL");
    if (cp) p = *cp; else oslam_colour_params_default(&p);
    if (p.max_weight < 1 || p.max_weight > 255) return fail(OSLAM_E_INVALID, "max_weight of the colours must lie in 1..255");
    if (!isfinite(p.band) || p.band < 0.0f) return fail(OSLAM_E_INVALID, "band must be finite and not negative");
    if (p.band > vol->p.mu) return fail(OSLAM_E_INVALID, "band must not exceed the volume's mu");
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    if (vol->colour.words) { rc = fail(OSLAM_E_INVALID, "the volume has colour already"); goto done; }
    if (hipMalloc((void **)&words, oslam_volume_bytes(&vol->p)) != hipSuccess) {
        (void)hipGetLastError();
        words = NULL;
        rc = fail(OSLAM_E_NOMEM, "no device memory for the colour buffer");
        goto done;
    }
    HIPCHK(hipMemsetAsync(words, 0, oslam_volume_bytes(&vol->p), (hipStream_t)oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    vol->colour.words = words;
    vol->colour.band = p.band == 0.0f ? vol->p.mu : p.band;
    vol->colour.max_weight = p.max_weight;
    words = NULL;
done:
    if (words) (void)hipFree(words);
    oslam_volume_unlock();
    return rc;
}

/* the two taps: the whole colour buffer down (words_out) or up (words_in) */
static int colour_words_copy(oslam_volume *vol, uint32_t *words_out, const uint32_t *words_in)
{
    int rc = OSLAM_OK;
    if (!vol || (!words_out && !words_in)) return fail(OSLAM_E_INVALID, "NULL argument");
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    if (!vol->colour.words) { rc = fail(OSLAM_E_INVALID, "the volume has no colour"); goto done; }
    if (words_out) HIPCHK(hipMemcpy(words_out, vol->colour.words, oslam_volume_bytes(&vol->p), hipMemcpyDeviceToHost));
    else HIPCHK(hipMemcpy(vol->colour.words, words_in, oslam_volume_bytes(&vol->p), hipMemcpyHostToDevice));
done:
    oslam_volume_unlock();
    return rc;
}

int oslam_volume_colour_words(oslam_volume *vol, uint32_t *words_out) { return colour_words_copy(vol, words_out, NULL); }

int oslam_volume_set_colour_words(oslam_volume *vol, const uint32_t *words) { return colour_words_copy(vol, NULL, words); }

/* ---- integration ---- */
int oslam_volume_integrate_colour(oslam_volume *vol, const oslam_view *v, const oslam_view *c, const float T_vol_cam[16],
                                  oslam_integrate_result *res, uint32_t *coloured_out)
{
    int rc;
    if (!vol || !v || !c || !T_vol_cam) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_refine_check_rigid(T_vol_cam);
    if (rc != OSLAM_OK) return rc;
    if (coloured_out) *coloured_out = 0;
    if (vol->dev != v->dev || vol->dev != c->dev) return fail(OSLAM_E_INVALID, "volume and view live on different devices");
    if (!c->d_colour) return fail(OSLAM_E_INVALID, "the colour view has no colour");
    if (c->k.w != v->k.w || c->k.h != v->k.h || memcmp(&c->k.fx, &v->k.fx, sizeof(float)) != 0 ||
        memcmp(&c->k.fy, &v->k.fy, sizeof(float)) != 0 || memcmp(&c->k.cx, &v->k.cx, sizeof(float)) != 0 ||
        memcmp(&c->k.cy, &v->k.cy, sizeof(float)) != 0)
        return fail(OSLAM_E_INVALID, "the colour view's size and intrinsics must be the depth view's");
    if (!vol->colour.words) return fail(OSLAM_E_INVALID, "the volume has no colour");
    return oslam_volume_integrate_views(vol, v, c, T_vol_cam, res, coloured_out);
}

/* ---- reading colour back ---- */
int oslam_volume_colours(oslam_volume *vol, const float *xyz, size_t n, size_t stride_bytes, uint8_t *rgb_out, uint8_t *valid_out,
                         size_t *n_valid_out)
{
    int rc = OSLAM_OK;
    const size_t stride = stride_bytes ? stride_bytes : 3 * sizeof(float);
    float *h_xyz = NULL, *d_xyz = NULL;
    uint32_t *d_out = NULL, *d_cnt = NULL, *h_out = NULL, n_valid = 0;
    size_t i;
    void *stream = oslam_stream();
    if (!vol) return fail(OSLAM_E_INVALID, "volume is NULL");
    if (n && (!xyz || !rgb_out || !valid_out)) return fail(OSLAM_E_INVALID, "NULL argument");
    if (stride < 3 * sizeof(float) || stride % sizeof(float) != 0)
        return fail(OSLAM_E_INVALID, "stride_bytes must be a multiple of 4 and at least 12");
    if (n > 0x7fffffffu) return fail(OSLAM_E_INVALID, "at most 2^31 - 1 points");
    if (n_valid_out) *n_valid_out = 0;
    if (!vol->colour.words) return fail(OSLAM_E_INVALID, "the volume has no colour");
    if (n == 0) return OSLAM_OK;
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    h_out = (uint32_t *)malloc(sizeof(uint32_t) * n);
    if (stride != 3 * sizeof(float)) h_xyz = (float *)malloc(sizeof(float) * 3 * n);
    if (!h_out || (stride != 3 * sizeof(float) && !h_xyz)) {
        free(h_out);
        free(h_xyz);
        return fail(OSLAM_E_NOMEM, "host allocation failed");
    }
    for (i = 0; h_xyz && i < n; i++) memcpy(h_xyz + 3 * i, (const char *)xyz + i * stride, 3 * sizeof(float));
    oslam_volume_lock();
    KCHK(oslam_dev_alloc((void **)&d_xyz, sizeof(float) * 3 * n));
    KCHK(oslam_dev_alloc((void **)&d_out, sizeof(uint32_t) * n));
    KCHK(oslam_counters_open(&d_cnt, 0, stream));
    HIPCHK(hipMemcpyAsync(d_xyz, h_xyz ? h_xyz : xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, (hipStream_t)stream));
    KCHK(oslamk_colour_points(&vol->k, vol->colour.words, d_xyz, (uint32_t)n, d_out, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(h_out, d_out, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(&n_valid, d_cnt, sizeof n_valid, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (i = 0; i < n; i++) {
        rgb_out[3 * i] = (uint8_t)(h_out[i] & 0xffu);
        rgb_out[3 * i + 1] = (uint8_t)((h_out[i] >> 8) & 0xffu);
        rgb_out[3 * i + 2] = (uint8_t)((h_out[i] >> 16) & 0xffu);
        valid_out[i] = (uint8_t)(h_out[i] >> 24 != 0u);
    }
    if (n_valid_out) *n_valid_out = n_valid;
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    oslam_volume_unlock();
    if (d_cnt) oslam_dev_free(d_cnt);
    if (d_out) oslam_dev_free(d_out);
    if (d_xyz) oslam_dev_free(d_xyz);
    free(h_out);
    free(h_xyz);
    return rc;
}

int oslam_volume_paint_view(oslam_volume *vol, const float T_vol_cam[16], oslam_view *v, uint32_t *painted_out)
{
    int rc, fresh = 0;
    uint32_t *d_cnt = NULL, *d_img = NULL, painted = 0;
    void *stream = oslam_stream();
    if (!vol || !T_vol_cam || !v) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_refine_check_rigid(T_vol_cam);
    if (rc != OSLAM_OK) return rc;
    if (painted_out) *painted_out = 0;
    if (vol->dev != v->dev) return fail(OSLAM_E_INVALID, "volume and view live on different devices");
    if (!vol->colour.words) return fail(OSLAM_E_INVALID, "the volume has no colour");
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    d_img = v->d_colour;
    if (!d_img) {
        HIPCHK(hipMalloc((void **)&d_img, sizeof(uint32_t) * (size_t)v->k.w * (size_t)v->k.h));
        fresh = 1;
    }
    KCHK(oslam_counters_open(&d_cnt, 0, stream));
    KCHK(oslamk_colour_view(&vol->k, vol->colour.words, &v->k, T_vol_cam, d_img, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(&painted, d_cnt, sizeof painted, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    v->d_colour = d_img;
    fresh = 0;
    if (painted_out) *painted_out = painted;
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    if (fresh && d_img) (void)hipFree(d_img);
    oslam_volume_unlock();
    if (d_cnt) oslam_dev_free(d_cnt);
    return rc;
}
