/*
 * oslam_world_raycast.c -- the whole map, voxel store plus window, ray-cast back into a view (include/oslam.h at
 * oslam_world_raycast): the host side of k_brick_raycast in oslam_world_raycast.hip.  A call checks its arguments, derives
 * the box in force (by default the bounding box of the table's bricks, from the store's keys and the window's brick range,
 * on the host), builds the map of oslam_world_surface.c with TSDF words in its bricks (oslam_world_map_open), allocates
 * the view as oslam_volume_raycast does, runs one kernel and reads the two counters back with one host wait, under the
 * volume lock and the store's.  oslam_world_track is oslam_volume_track's glue with this ray cast at its head.
 */
#include <math.h>

#include "oslam_internal.h"
#include "oslam_window.h"
#include "oslam_world.h"

#define WRAY_BOX_MAX (OSLAMK_SHIFT_MAX + 520)   /* 8 * (the largest brick coordinate of a store + 1) */

int oslam_world_raycast_params_default(oslam_world_raycast_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    return OSLAM_OK;
}

/* the checks that need neither handle: *out = the parameters in force but for the defaults the map decides */
static int check_args(const oslam_world_raycast_params *rp, const float *T, const oslam_camera *cam, int width, int height,
                      oslam_world_raycast_params *out)
{
    int rc, a;
    if (rp) *out = *rp; else oslam_world_raycast_params_default(out);
    if (!oslam_view_camera_ok(cam, width, height, 0, 1)) return fail(OSLAM_E_INVALID, "bad ray cast camera or size");
    rc = oslam_refine_check_rigid(T);
    if (rc != OSLAM_OK) return rc;
    if (out->anchor_set && !oslamk_shift_ok(out->anchor)) return fail(OSLAM_E_INVALID, "an anchor is at most 2^20 voxels");
    for (a = 0; out->box_set && a < 3; a++) {
        if (out->box_lo[a] < -WRAY_BOX_MAX || out->box_lo[a] > WRAY_BOX_MAX || out->box_hi[a] < -WRAY_BOX_MAX ||
            out->box_hi[a] > WRAY_BOX_MAX)
            return fail(OSLAM_E_INVALID, "a box corner is at most 2^20 + 520 voxels");
        if (out->box_hi[a] - out->box_lo[a] < 2) return fail(OSLAM_E_INVALID, "a box is at least 2 voxels wide on every axis");
    }
    if (!isfinite(out->mu) || out->mu < 0.0f) return fail(OSLAM_E_INVALID, "mu must be finite and not negative");
    return OSLAM_OK;
}

/* what one ray cast leaves besides the view */
typedef struct wray_run {
    uint32_t hits, normals, bricks, window_bricks, launches;
    int32_t anchor[3], box_lo[3], box_hi[3];
} wray_run;

/* The ray cast after check_args, with the volume lock held; the store's is taken here.  dev: the device of a map without a
 * volume.  Every device block but the view is freed */
static int world_raycast(oslam_world *w, oslam_volume *vol, const oslam_world_raycast_params *p, int dev, const float T[16],
                         const oslam_camera *cam, int width, int height, oslam_view **out, wray_run *o)
{
    int rc = OSLAM_OK, a, launched = 0, opened = 0, kb0[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
    const size_t n_pix = (size_t)width * (size_t)height;
    float voxel, origin0[3], mu, step;
    int32_t *skeys = NULL;
    size_t ns, nw = 0, i;
    uint32_t *d_cnt = NULL, cnt[2] = {0, 0};
    oslam_view *v = NULL;
    oslam_world_surface_params sp;
    oslam_world_map wm;
    oslamk_wray box;
    void *stream = oslam_stream();
    memset(o, 0, sizeof *o);
    memset(&wm, 0, sizeof wm);
    oslam_world_lock(w);
    oslam_world_frame(w, &voxel, origin0);
    if (vol && !oslam_world_compatible(w, vol->p.voxel, vol->p.origin)) {
        rc = fail(OSLAM_E_INVALID, "the voxel store was made for another voxel size or origin");
        goto done;
    }
    if (p->mu == 0.0f && !vol) { rc = fail(OSLAM_E_INVALID, "mu must be given without a volume"); goto done; }
    mu = p->mu == 0.0f ? vol->p.mu : p->mu;
    if (p->mu != 0.0f && !(mu >= 2.0f * voxel)) { rc = fail(OSLAM_E_INVALID, "mu must be at least 2 voxels"); goto done; }
    step = 0.5f * mu;
    if ((double)(cam->z_max - cam->z_min) / (double)step >= 65535.0) {
        rc = fail(OSLAM_E_LIMIT, "a ray takes at most 65535 steps of mu / 2 between z_min and z_max");
        goto done;
    }
    /* the bounding box of the table's bricks: the store's keys united with the window's brick range */
    ns = oslam_world_brick_count(w);
    if (vol) {
        const unsigned sides[3] = {vol->p.nx, vol->p.ny, vol->p.nz};
        oslam_window_bricks(sides, vol->off, kb0, nb);
        nw = (size_t)nb[0] * (size_t)nb[1] * (size_t)nb[2];
    }
    for (a = 0; a < 3; a++) {
        o->anchor[a] = p->anchor_set ? p->anchor[a] : vol ? vol->off[a] : 0;
        o->box_lo[a] = p->box_lo[a];
        o->box_hi[a] = p->box_hi[a];
    }
    if (!p->box_set && ns + nw > 0) {
        int32_t lo[3], hi[3];
        if (ns) {
            skeys = (int32_t *)malloc(sizeof(int32_t) * 3 * ns);
            if (!skeys) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
            oslam_world_brick_keys(w, skeys);
        }
        for (a = 0; a < 3; a++) {
            lo[a] = nw ? kb0[a] : skeys[a];
            hi[a] = nw ? kb0[a] + nb[a] - 1 : skeys[a];
            for (i = 0; i < ns; i++) {
                if (skeys[3 * i + a] < lo[a]) lo[a] = skeys[3 * i + a];
                if (skeys[3 * i + a] > hi[a]) hi[a] = skeys[3 * i + a];
            }
            o->box_lo[a] = 8 * lo[a];
            o->box_hi[a] = 8 * (hi[a] + 1);
        }
    }
    oslam_world_surface_params_default(&sp);
    sp.anchor_set = 1;
    memcpy(sp.anchor, o->anchor, sizeof sp.anchor);
    sp.dev = dev;
    rc = oslam_world_map_open(w, vol, &sp, OSLAM_MAP_TSDF, stream, &wm);
    if (rc != OSLAM_OK) goto done;
    o->bricks = wm.bricks;
    o->window_bricks = wm.window_bricks;
    o->launches = wm.launches;
    if (wm.bricks == 0) {                                           /* an empty map: a view of zeros, no launch */
        rc = oslam_pick_device(dev, &wm.dev);
        if (rc != OSLAM_OK) goto done;
    } else
        opened = launched = 1;
    rc = oslam_view_new(wm.dev, width, height, cam, &v);
    if (rc != OSLAM_OK) goto done;
    KCHK(oslam_dev_alloc((void **)&v->d_maps, sizeof(float) * 8 * n_pix));
    launched = 1;
    if (wm.bricks == 0) {
        HIPCHK(hipMemsetAsync(v->d_z, 0, sizeof(float) * n_pix, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(v->d_maps, 0, sizeof(float) * 8 * n_pix, (hipStream_t)stream));
    } else {
        for (a = 0; a < 3; a++) {
            box.r_lo[a] = o->box_lo[a] - o->anchor[a];
            box.r_hi[a] = o->box_hi[a] - o->anchor[a];
        }
        box.mu = mu;
        KCHK(oslam_counters_open(&d_cnt, 0, stream));
        KCHK(oslamk_brick_raycast(&wm.m, &box, &v->k, T, v->d_z, v->d_maps, d_cnt, stream));
        o->launches++;
        HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, (hipStream_t)stream));
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    launched = 0;
    o->hits = cnt[0];
    o->normals = cnt[1];
done:
    if (launched) (void)hipStreamSynchronize((hipStream_t)stream);
    oslam_world_unlock(w);
    if (d_cnt) oslam_dev_free(d_cnt);
    if (opened) oslam_world_map_close(&wm);
    free(skeys);
    if (rc != OSLAM_OK) {
        if (v) oslam_view_destroy(v);
        return rc;
    }
    *out = v;
    return OSLAM_OK;
}

static void fill_result(oslam_world_raycast_result *res, const wray_run *o, double t0)
{
    res->hits = o->hits;
    res->normals = o->normals;
    res->bricks = o->bricks;
    res->window_bricks = o->window_bricks;
    res->launches = o->launches;
    memcpy(res->anchor, o->anchor, sizeof res->anchor);
    memcpy(res->box_lo, o->box_lo, sizeof res->box_lo);
    memcpy(res->box_hi, o->box_hi, sizeof res->box_hi);
    res->ms_total = (float)(now_ms() - t0);
}

int oslam_world_raycast(oslam_world *w, oslam_volume *vol, const oslam_world_raycast_params *rp, const float T_vol_cam[16],
                        const oslam_camera *cam, int width, int height, oslam_view **view_out, oslam_world_raycast_result *res)
{
    int rc;
    const double t0 = now_ms();
    oslam_world_raycast_params p;
    wray_run o;
    if (view_out) *view_out = NULL;
    if (!w || !T_vol_cam || !cam || !view_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_args(rp, T_vol_cam, cam, width, height, &p);
    if (rc != OSLAM_OK) return rc;
    if (res) memset(res, 0, sizeof *res);
    oslam_volume_lock();
    rc = world_raycast(w, vol, &p, p.dev, T_vol_cam, cam, width, height, view_out, &o);
    oslam_volume_unlock();
    if (rc == OSLAM_OK && res) fill_result(res, &o, t0);
    return rc;
}

int oslam_world_track(oslam_world *w, oslam_volume *vol, const oslam_world_raycast_params *rp, oslam_view *v,
                      const float T_vol_cam_prev[16], const oslam_egomotion_params *ep, float T_vol_cam_out[16],
                      oslam_egomotion_result *ego_res)
{
    int rc;
    const double t0 = now_ms();
    oslam_egomotion_params p;
    oslam_egomotion_result er;
    oslam_world_raycast_params q;
    oslam_camera cam;
    oslam_view *model = NULL;
    wray_run o;
    float T[16];
    if (!w || !v || !T_vol_cam_prev || !T_vol_cam_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_ego_check_params(ep, &p);
    if (rc != OSLAM_OK) return rc;
    oslam_view_camera(v, &cam);
    rc = check_args(rp, T_vol_cam_prev, &cam, v->k.w, v->k.h, &q);
    if (rc != OSLAM_OK) return rc;
    if (vol && vol->dev != v->dev) return fail(OSLAM_E_INVALID, "volume and view live on different devices");
    oslam_volume_lock();
    rc = world_raycast(w, vol, &q, v->dev, T_vol_cam_prev, &cam, v->k.w, v->k.h, &model, &o);
    if (rc == OSLAM_OK) rc = oslam_view_egomotion(v, model, NULL, &p, T, &er);
    oslam_volume_unlock();
    if (model) oslam_view_destroy(model);
    if (rc != OSLAM_OK) return rc;
    oslam_rigid_product_f(T_vol_cam_prev, T, T_vol_cam_out);      /* the element order of oslam_tracker_step_cam */
    T_vol_cam_out[12] = T_vol_cam_out[13] = T_vol_cam_out[14] = 0.0f;
    T_vol_cam_out[15] = 1.0f;
    if (ego_res) {
        *ego_res = er;
        ego_res->launches += o.launches;                            /* the map's and the ray cast's */
        ego_res->ms_total = (float)(now_ms() - t0);
    }
    return OSLAM_OK;
}
