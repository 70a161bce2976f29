/*
 * oslam_world_colour.c -- the colour at points of the whole map, colour store plus coloured window (include/oslam.h at
 * oslam_world_colours): the host side of k_brick_colours in oslam_world_colour.hip.  A call builds the map of
 * oslam_world_surface.c with colour words in its bricks (oslam_world_map_open, plane OSLAM_MAP_COLOUR), sends the points
 * up as oslam_volume_colours does, runs one kernel and unpacks the words, under the volume lock and the store's.
 * oslam_world_paint_view builds the same map and runs k_brick_colour_view over a view's pixels, as
 * oslam_volume_paint_view does with the volume alone.
 */
#include "oslam_internal.h"
#include "oslam_world.h"

int oslam_world_colours(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, const float *xyz, size_t n,
                        size_t stride_bytes, uint8_t *rgb_out, uint8_t *valid_out, size_t *n_valid_out)
{
    int rc = OSLAM_OK, launched = 0, opened = 0;
    const size_t stride = stride_bytes ? stride_bytes : 3 * sizeof(float);
    float *h_xyz = NULL, *d_xyz = NULL;
    uint32_t *d_out = NULL, *d_cnt = NULL, *h_out = NULL, n_valid = 0;
    size_t i;
    oslam_world_surface_params p;
    oslam_world_map wm;
    void *stream = oslam_stream();
    if (!w) return fail(OSLAM_E_INVALID, "world is NULL");
    if (n && (!xyz || !rgb_out || !valid_out)) return fail(OSLAM_E_INVALID, "NULL argument");
    if (stride < 3 * sizeof(float) || stride % sizeof(float) != 0)
        return fail(OSLAM_E_INVALID, "stride_bytes must be a multiple of 4 and at least 12");
    if (n > 0x7fffffffu) return fail(OSLAM_E_INVALID, "at most 2^31 - 1 points");
    rc = oslam_world_surface_check_params(sp, &p);
    if (rc != OSLAM_OK) return rc;
    if (!oslam_world_coloured(w)) return fail(OSLAM_E_INVALID, "the voxel store keeps no colour");
    memset(&wm, 0, sizeof wm);
    if (n) {                                                        /* before the locks: nothing below them allocates host memory */
        h_out = (uint32_t *)malloc(sizeof(uint32_t) * n);
        if (stride != 3 * sizeof(float)) h_xyz = (float *)malloc(sizeof(float) * 3 * n);
        if (!h_out || (stride != 3 * sizeof(float) && !h_xyz)) {
            free(h_out);
            free(h_xyz);
            return fail(OSLAM_E_NOMEM, "host allocation failed");
        }
        for (i = 0; h_xyz && i < n; i++) memcpy(h_xyz + 3 * i, (const char *)xyz + i * stride, 3 * sizeof(float));
    }
    oslam_volume_lock();
    oslam_world_lock(w);
    if (vol && !vol->colour.words) { rc = fail(OSLAM_E_INVALID, "the volume has no colour"); goto done; }
    if (vol && !oslam_world_compatible(w, vol->p.voxel, vol->p.origin)) {
        rc = fail(OSLAM_E_INVALID, "the voxel store was made for another voxel size or origin");
        goto done;
    }
    if (n_valid_out) *n_valid_out = 0;
    if (n == 0) goto done;
    memset(rgb_out, 0, 3 * n);
    memset(valid_out, 0, n);
    rc = oslam_world_map_open(w, vol, &p, OSLAM_MAP_COLOUR, stream, &wm);
    if (rc != OSLAM_OK || wm.bricks == 0) goto done;                /* an empty map: no colour anywhere, no device call */
    opened = launched = 1;
    KCHK(oslam_dev_alloc((void **)&d_xyz, sizeof(float) * 3 * n));
    KCHK(oslam_dev_alloc((void **)&d_out, sizeof(uint32_t) * n));
    KCHK(oslam_counters_open(&d_cnt, 0, stream));
    HIPCHK(hipMemcpyAsync(d_xyz, h_xyz ? h_xyz : xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, (hipStream_t)stream));
    KCHK(oslamk_brick_colours(&wm.m, d_xyz, (uint32_t)n, d_out, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(h_out, d_out, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(&n_valid, d_cnt, sizeof n_valid, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    launched = 0;
    for (i = 0; i < n; i++) {
        rgb_out[3 * i] = (uint8_t)(h_out[i] & 0xffu);
        rgb_out[3 * i + 1] = (uint8_t)((h_out[i] >> 8) & 0xffu);
        rgb_out[3 * i + 2] = (uint8_t)((h_out[i] >> 16) & 0xffu);
        valid_out[i] = (uint8_t)(h_out[i] >> 24 != 0u);
    }
    if (n_valid_out) *n_valid_out = n_valid;
done:
    if (launched) (void)hipStreamSynchronize((hipStream_t)stream);
    oslam_world_unlock(w);
    oslam_volume_unlock();
    if (d_cnt) oslam_dev_free(d_cnt);
    if (d_out) oslam_dev_free(d_out);
    if (d_xyz) oslam_dev_free(d_xyz);
    if (opened) oslam_world_map_close(&wm);
    free(h_out);
    free(h_xyz);
    return rc;
}

int oslam_world_paint_view(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, const float T_vol_cam[16],
                           oslam_view *v, uint32_t *painted_out)
{
    int rc, fresh = 0, launched = 0, opened = 0;
    uint32_t *d_cnt = NULL, *d_img = NULL, painted = 0;
    oslam_world_surface_params p;
    oslam_world_map wm;
    void *stream = oslam_stream();
    if (!w || !T_vol_cam || !v) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_refine_check_rigid(T_vol_cam);
    if (rc == OSLAM_OK) rc = oslam_world_surface_check_params(sp, &p);
    if (rc != OSLAM_OK) return rc;
    if (painted_out) *painted_out = 0;
    if (vol && vol->dev != v->dev) return fail(OSLAM_E_INVALID, "volume and view live on different devices");
    if (!oslam_world_coloured(w)) return fail(OSLAM_E_INVALID, "the voxel store keeps no colour");
    p.dev = v->dev;                                                 /* a map without a volume goes where the view is */
    memset(&wm, 0, sizeof wm);
    oslam_volume_lock();
    oslam_world_lock(w);
    if (vol && !vol->colour.words) { rc = fail(OSLAM_E_INVALID, "the volume has no colour"); goto done; }
    rc = oslam_world_map_open(w, vol, &p, OSLAM_MAP_COLOUR, stream, &wm);
    if (rc != OSLAM_OK) goto done;
    if (wm.bricks == 0) {                                           /* an empty map: no colour anywhere, no launch */
        rc = oslam_pick_device(v->dev, &wm.dev);
        if (rc != OSLAM_OK) goto done;
    } else
        opened = launched = 1;
    d_img = v->d_colour;
    if (!d_img) {
        HIPCHK(hipMalloc((void **)&d_img, sizeof(uint32_t) * (size_t)v->k.w * (size_t)v->k.h));
        fresh = 1;
    }
    launched = 1;
    if (wm.bricks == 0)
        HIPCHK(hipMemsetAsync(d_img, 0, sizeof(uint32_t) * (size_t)v->k.w * (size_t)v->k.h, (hipStream_t)stream));
    else {
        KCHK(oslam_counters_open(&d_cnt, 0, stream));
        KCHK(oslamk_brick_colour_view(&wm.m, &v->k, T_vol_cam, d_img, d_cnt, stream));
        HIPCHK(hipMemcpyAsync(&painted, d_cnt, sizeof painted, hipMemcpyDeviceToHost, (hipStream_t)stream));
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    launched = 0;
    v->d_colour = d_img;
    fresh = 0;
    if (painted_out) *painted_out = painted;
done:
    if (launched) (void)hipStreamSynchronize((hipStream_t)stream);
    if (fresh && d_img) (void)hipFree(d_img);
    oslam_world_unlock(w);
    oslam_volume_unlock();
    if (d_cnt) oslam_dev_free(d_cnt);
    if (opened) oslam_world_map_close(&wm);
    return rc;
}
