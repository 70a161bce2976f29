/*
 * oslam_volume.c -- fusion of depth views into a TSDF volume and the ray cast back into a view (include/oslam.h at
 * oslam_volume_integrate): the host side of the kernels in oslam_volume.hip.  A call checks its arguments, zeroes a
 * counter block, runs one kernel and reads the counters back with one host wait.  oslam_volume_track is glue over the
 * ray cast and oslam_view_egomotion, oslam_volume_track_pyramid over the ray cast, a pyramid of it and
 * oslam_pyramid_egomotion (one body, track_from_raycast); oslam_view_to_cloud runs the depth front end's compaction
 * over a view's maps.  Here too: a volume's parameters, create, destroy and reset, the view read-backs, the voxel get and
 * set, and the volume lock that every call on a volume takes.  The moving window (oslam_volume_shift,
 * oslam_volume_shift_world, the pack's tap, oslam_volume_follow) is oslam_window.c, its arithmetic oslam_window.h.  The
 * extraction of the fused volume, or of what a shift loses, as a cloud or a triangle list is oslam_surface.c (kernels:
 * oslam_surface.hip and oslam_mesh.hip).  The limits of a volume's sides are oslam_kernels.h's.  A volume with colour
 * (oslam_colour.c) gets its colour pass from the integration's body here, in the same call.
 */
#include <math.h>
#include <pthread.h>

#include "oslam_internal.h"
#include "oslam_window.h"

/* calls on volumes, oslam_view_to_cloud and oslam_view_maps take turns.  Lock order: g_vol_mu, then the lock of oslam_view_egomotion, then the views' maps */
static pthread_mutex_t g_vol_mu = PTHREAD_MUTEX_INITIALIZER;
void oslam_volume_lock(void) { pthread_mutex_lock(&g_vol_mu); }
void oslam_volume_unlock(void) { pthread_mutex_unlock(&g_vol_mu); }

int oslam_volume_params_default(oslam_volume_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->nx = p->ny = p->nz = 256;
    p->voxel = 0.02f;
    p->origin[0] = p->origin[1] = -128.0f * 0.02f;
    p->origin[2] = 0.0f;
    p->mu = 4.0f * 0.02f;
    p->max_weight = 128;
    return OSLAM_OK;
}

static int check_params(const oslam_volume_params *p)
{
    if (!isfinite(p->voxel) || !isfinite(p->mu) || !isfinite(p->origin[0]) || !isfinite(p->origin[1]) || !isfinite(p->origin[2]))
        return fail(OSLAM_E_INVALID, "volume parameters must be finite");
    if (!oslamk_sides_ok(p->nx, p->ny, p->nz, 3))
        return fail(OSLAM_E_INVALID, "voxels per side must lie in 16..512 and be a multiple of 8");
    if (!(p->voxel > 0.0f)) return fail(OSLAM_E_INVALID, "voxel must be > 0");
    if (!(p->mu >= 2.0f * p->voxel)) return fail(OSLAM_E_INVALID, "mu must be at least 2 voxels");
    if (p->max_weight < 1 || p->max_weight > 65535) return fail(OSLAM_E_INVALID, "max_weight must lie in 1..65535");
    if (!isfinite(1.0f / p->voxel) || !isfinite(512.0f * p->voxel)) return fail(OSLAM_E_INVALID, "voxel out of the float range");
    return OSLAM_OK;
}

int oslam_volume_create(const oslam_volume_params *p, int dev, oslam_volume **out)
{
    int rc, devsel;
    oslam_volume *vol;
    if (out) *out = NULL;
    if (!p || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_params(p);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_pick_device(dev, &devsel);
    if (rc != OSLAM_OK) return rc;
    vol = (oslam_volume *)calloc(1, sizeof *vol);
    if (!vol) return fail(OSLAM_E_NOMEM, "host allocation failed");
    vol->dev = devsel;
    vol->p = *p;
    /* the volume lives as long as the handle: its own block, not one of the kept scratch blocks */
    HIPCHK(hipMalloc((void **)&vol->k.words, oslam_volume_bytes(p)));
    HIPCHK(hipMemsetAsync(vol->k.words, 0, oslam_volume_bytes(p), (hipStream_t)oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    vol->k.nx = (int)p->nx;
    vol->k.ny = (int)p->ny;
    vol->k.nz = (int)p->nz;
    vol->k.voxel = p->voxel;
    vol->k.inv_voxel = 1.0f / p->voxel;
    memcpy(vol->k.origin, p->origin, sizeof vol->k.origin);
    vol->k.mu = p->mu;
    vol->k.max_weight = p->max_weight;
done:
    if (rc != OSLAM_OK) {
        if (vol->k.words) (void)hipFree(vol->k.words);
        free(vol);
        return rc;
    }
    *out = vol;
    return OSLAM_OK;
}

int oslam_volume_destroy(oslam_volume *vol)
{
    if (!vol) return fail(OSLAM_E_INVALID, "volume is NULL");
    /* every call that touched the volume ended with a synchronisation of its stream */
    pthread_mutex_lock(&g_vol_mu);
    if (hipSetDevice(vol->dev) == hipSuccess) {
        (void)hipFree(vol->k.words);
        if (vol->spare) (void)hipFree(vol->spare);
        if (vol->colour.words) (void)hipFree(vol->colour.words);
        if (vol->colour_spare) (void)hipFree(vol->colour_spare);
    }
    pthread_mutex_unlock(&g_vol_mu);
    free(vol);
    return OSLAM_OK;
}

int oslam_volume_reset(oslam_volume *vol)
{
    int rc = OSLAM_OK;
    if (!vol) return fail(OSLAM_E_INVALID, "volume is NULL");
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    pthread_mutex_lock(&g_vol_mu);
    HIPCHK(hipMemsetAsync(vol->k.words, 0, oslam_volume_bytes(&vol->p), (hipStream_t)oslam_stream()));
    if (vol->colour.words) HIPCHK(hipMemsetAsync(vol->colour.words, 0, oslam_volume_bytes(&vol->p), (hipStream_t)oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    memset(vol->off, 0, sizeof vol->off);
    oslam_window_origin(vol->p.origin, vol->p.voxel, vol->off, vol->k.origin);
done:
    pthread_mutex_unlock(&g_vol_mu);
    return rc;
}

int oslam_volume_integrate(oslam_volume *vol, const oslam_view *v, const float T_vol_cam[16], oslam_integrate_result *res)
{
    int rc;
    if (!vol || !v || !T_vol_cam) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_refine_check_rigid(T_vol_cam);
    if (rc != OSLAM_OK) return rc;
    if (vol->dev != v->dev) return fail(OSLAM_E_INVALID, "volume and view live on different devices");
    return oslam_volume_integrate_views(vol, v, NULL, T_vol_cam, res, NULL);
}

int oslam_volume_integrate_views(oslam_volume *vol, const oslam_view *v, const oslam_view *c, const float T_vol_cam[16],
                                 oslam_integrate_result *res, uint32_t *coloured)
{
    int rc = OSLAM_OK, a;
    const double t0 = now_ms();
    double inv_d[12];
    float inv[12];
    uint32_t *d_cnt = NULL, cnt[2] = {0, 0};
    void *stream = oslam_stream();
    if (res) memset(res, 0, sizeof *res);
    oslam_rigid_inverse(T_vol_cam, inv_d);
    for (a = 0; a < 12; a++) inv[a] = (float)inv_d[a];
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    pthread_mutex_lock(&g_vol_mu);
    KCHK(oslam_counters_open(&d_cnt, 0, stream));
    KCHK(oslamk_tsdf_integrate(&vol->k, &v->k, inv, d_cnt, stream));
    if (c) KCHK(oslamk_tsdf_colour(&vol->k, &vol->colour, &v->k, c->d_colour, inv, d_cnt + 1, stream));
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof(uint32_t) * (c ? 2 : 1), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    pthread_mutex_unlock(&g_vol_mu);
    if (d_cnt) oslam_dev_free(d_cnt);
    if (rc == OSLAM_OK && res) {
        res->updated = cnt[0];
        res->launches = c ? 2 : 1;
        res->ms_total = (float)(now_ms() - t0);
    }
    if (rc == OSLAM_OK && coloured) *coloured = cnt[1];
    return rc;
}

static int check_raycast(const oslam_volume *vol, const float *T, const oslam_camera *cam, int width, int height)
{
    if (!vol || !T || !cam) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!oslam_view_camera_ok(cam, width, height, 0, 1)) return fail(OSLAM_E_INVALID, "bad ray cast camera or size");
    return oslam_refine_check_rigid(T);
}

/* the ray cast proper, with g_vol_mu held and the volume's device bound */
static int raycast(oslam_volume *vol, const float T[16], const oslam_camera *cam, int width, int height, oslam_view **out,
                   uint32_t cnt[2])
{
    int rc;
    const size_t n_pix = (size_t)width * (size_t)height;
    uint32_t *d_cnt = NULL;
    void *stream = oslam_stream();
    oslam_view *v;
    rc = oslam_view_new(vol->dev, width, height, cam, &v);
    if (rc != OSLAM_OK) return rc;
    KCHK(oslam_dev_alloc((void **)&v->d_maps, sizeof(float) * 8 * n_pix));
    KCHK(oslam_counters_open(&d_cnt, 0, stream));
    KCHK(oslamk_tsdf_raycast(&vol->k, &v->k, T, v->d_z, v->d_maps, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(cnt, d_cnt, sizeof(uint32_t) * 2, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    if (d_cnt) oslam_dev_free(d_cnt);
    if (rc != OSLAM_OK) {
        oslam_view_destroy(v);
        return rc;
    }
    *out = v;
    return OSLAM_OK;
}

int oslam_volume_raycast(oslam_volume *vol, const float T_vol_cam[16], const oslam_camera *cam, int width, int height,
                         oslam_view **view_out, oslam_raycast_result *res)
{
    int rc;
    const double t0 = now_ms();
    uint32_t cnt[2] = {0, 0};
    if (view_out) *view_out = NULL;
    if (!view_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_raycast(vol, T_vol_cam, cam, width, height);
    if (rc != OSLAM_OK) return rc;
    if (res) memset(res, 0, sizeof *res);
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    pthread_mutex_lock(&g_vol_mu);
    rc = raycast(vol, T_vol_cam, cam, width, height, view_out, cnt);
    pthread_mutex_unlock(&g_vol_mu);
    if (rc == OSLAM_OK && res) {
        res->hits = cnt[0];
        res->normals = cnt[1];
        res->launches = 1;
        res->ms_total = (float)(now_ms() - t0);
    }
    return rc;
}

/* The body of oslam_volume_track (frame and q both NULL: v against the ray cast from T_prev) and of
 * oslam_volume_track_pyramid (frame and q both given, v = the base of frame: frame against a pyramid of the ray cast
 * made with q), after their argument checks; p and q are the parameters in force, t0 the start of the call.  frame is
 * NULL exactly when q is: q is read only under frame. */
static int track_from_raycast(oslam_volume *vol, oslam_view *v, oslam_pyramid *frame, const oslam_pyramid_params *q,
                              const float T_prev[16], const oslam_egomotion_params *p, double t0, float T_out[16],
                              oslam_egomotion_result *ego_res)
{
    int rc;
    oslam_egomotion_result er;
    oslam_camera cam;
    oslam_view *model = NULL;
    oslam_pyramid *model_pyr = NULL;
    uint32_t cnt[2];
    float T[16];
    oslam_view_camera(v, &cam);
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    pthread_mutex_lock(&g_vol_mu);
    rc = raycast(vol, T_prev, &cam, v->k.w, v->k.h, &model, cnt);
    if (rc == OSLAM_OK && frame) rc = oslam_pyramid_create(model, q, &model_pyr);
    if (rc == OSLAM_OK)
        rc = frame ? oslam_pyramid_egomotion(frame, model_pyr, NULL, p, T, &er)
                   : oslam_view_egomotion(v, model, NULL, p, T, &er);
    pthread_mutex_unlock(&g_vol_mu);
    if (model_pyr) oslam_pyramid_destroy(model_pyr);
    if (model) oslam_view_destroy(model);
    if (rc != OSLAM_OK) return rc;
    oslam_rigid_product_f(T_prev, T, T_out);      /* the element order of oslam_tracker_step_cam */
    T_out[12] = T_out[13] = T_out[14] = 0.0f;
    T_out[15] = 1.0f;
    if (ego_res) {
        *ego_res = er;
        ego_res->launches += 1 + (frame ? q->n_levels - 1 : 0);     /* the ray cast and the down-sampling launches */
        ego_res->ms_total = (float)(now_ms() - t0);
    }
    return OSLAM_OK;
}

int oslam_volume_track(oslam_volume *vol, oslam_view *v, const float T_prev[16], const oslam_egomotion_params *ep,
                       float T_out[16], oslam_egomotion_result *ego_res)
{
    int rc;
    const double t0 = now_ms();
    oslam_egomotion_params p;
    if (!vol || !v || !T_prev || !T_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_ego_check_params(ep, &p);
    if (rc == OSLAM_OK) rc = oslam_refine_check_rigid(T_prev);
    if (rc != OSLAM_OK) return rc;
    if (vol->dev != v->dev) return fail(OSLAM_E_INVALID, "volume and view live on different devices");
    return track_from_raycast(vol, v, NULL, NULL, T_prev, &p, t0, T_out, ego_res);
}

int oslam_volume_track_pyramid(oslam_volume *vol, oslam_pyramid *frame, const float T_prev[16], const oslam_pyramid_params *pp,
                               const oslam_egomotion_params *ep, float T_out[16], oslam_egomotion_result *ego_res)
{
    int rc;
    const double t0 = now_ms();
    oslam_egomotion_params p;
    oslam_pyramid_params q;
    if (!vol || !frame || !T_prev || !T_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_ego_check_params(ep, &p);
    if (rc == OSLAM_OK) rc = oslam_pyramid_check_params(pp, &q);
    if (rc == OSLAM_OK) rc = oslam_refine_check_rigid(T_prev);
    if (rc == OSLAM_OK)
        rc = oslam_ego_check_pyramid_schedule(&p, q.n_levels < frame->n_levels ? q.n_levels : frame->n_levels);
    if (rc != OSLAM_OK) return rc;
    if (vol->dev != frame->dev) return fail(OSLAM_E_INVALID, "volume and pyramid live on different devices");
    return track_from_raycast(vol, frame->level[0], frame, &q, T_prev, &p, t0, T_out, ego_res);
}

int oslam_view_to_cloud(oslam_view *v, float *xyz_out, float *nrm_out, size_t cap, size_t *n_out)
{
    int rc, built = 0, k;
    float *d_out = NULL, *h_out = NULL;
    uint32_t np = 0;
    size_t n_pix;
    if (!v || !xyz_out || !nrm_out || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = 0;
    n_pix = (size_t)v->k.w * (size_t)v->k.h;
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    /* takes its turn with the calls on volumes: the shared stream and the kept scratch blocks */
    pthread_mutex_lock(&g_vol_mu);
    rc = oslam_track_view_maps(v, &built);
    if (rc != OSLAM_OK) goto done;
    KCHK(oslam_dev_alloc((void **)&d_out, sizeof(float) * 6 * n_pix));
    k = oslamk_maps_to_cloud(v->d_maps, n_pix, d_out, &np, oslam_stream());
    if (k != 0) { rc = fail(OSLAM_E_DEVICE, hipGetErrorString((hipError_t)k)); goto done; }
    *n_out = np;
    if (np > cap) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    h_out = (float *)malloc(sizeof(float) * 6 * (np ? np : 1));
    if (!h_out) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    if (np) HIPCHK(hipMemcpy(h_out, d_out, sizeof(float) * 6 * np, hipMemcpyDeviceToHost));
    split_points(h_out, np, xyz_out, nrm_out);
done:
    pthread_mutex_unlock(&g_vol_mu);
    free(h_out);
    if (d_out) oslam_dev_free(d_out);
    return rc;
}

int oslam_volume_voxels(oslam_volume *vol, int16_t *tsdf_q_out, uint16_t *weight_out)
{
    int rc = OSLAM_OK;
    size_t i, n;
    uint32_t *h = NULL;
    if (!vol || !tsdf_q_out || !weight_out) return fail(OSLAM_E_INVALID, "NULL argument");
    n = (size_t)vol->p.nx * (size_t)vol->p.ny * (size_t)vol->p.nz;
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    h = (uint32_t *)malloc(n * sizeof *h);
    if (!h) return fail(OSLAM_E_NOMEM, "host allocation failed");
    pthread_mutex_lock(&g_vol_mu);
    HIPCHK(hipMemcpy(h, vol->k.words, n * sizeof *h, hipMemcpyDeviceToHost));
    for (i = 0; i < n; i++) {
        tsdf_q_out[i] = (int16_t)(h[i] & 0xffffu);
        weight_out[i] = (uint16_t)(h[i] >> 16);
    }
done:
    pthread_mutex_unlock(&g_vol_mu);
    free(h);
    return rc;
}

int oslam_view_maps(oslam_view *v, float *maps_out, float *z_out)
{
    int rc, built = 0;
    size_t n_pix;
    if (!v || !maps_out) return fail(OSLAM_E_INVALID, "NULL argument");
    n_pix = (size_t)v->k.w * (size_t)v->k.h;
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    pthread_mutex_lock(&g_vol_mu);
    rc = oslam_track_view_maps(v, &built);
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipMemcpyAsync(maps_out, v->d_maps, sizeof(float) * 8 * n_pix, hipMemcpyDeviceToHost, (hipStream_t)oslam_stream()));
    if (z_out) HIPCHK(hipMemcpyAsync(z_out, v->d_z, sizeof(float) * n_pix, hipMemcpyDeviceToHost, (hipStream_t)oslam_stream()));
done:
    if (hipStreamSynchronize((hipStream_t)oslam_stream()) != hipSuccess && rc == OSLAM_OK) rc = fail(OSLAM_E_DEVICE, "synchronisation failed");
    pthread_mutex_unlock(&g_vol_mu);
    return rc;
}

int oslam_volume_set_voxels(oslam_volume *vol, const int16_t *tsdf_q, const uint16_t *weight)
{
    int rc = OSLAM_OK;
    size_t i, n;
    uint32_t *h = NULL;
    if (!vol || !tsdf_q || !weight) return fail(OSLAM_E_INVALID, "NULL argument");
    n = (size_t)vol->p.nx * (size_t)vol->p.ny * (size_t)vol->p.nz;
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    h = (uint32_t *)malloc(n * sizeof *h);
    if (!h) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (i = 0; i < n; i++) h[i] = (uint32_t)(uint16_t)tsdf_q[i] | (uint32_t)weight[i] << 16;
    pthread_mutex_lock(&g_vol_mu);
    HIPCHK(hipMemcpy(vol->k.words, h, n * sizeof *h, hipMemcpyHostToDevice));
done:
    pthread_mutex_unlock(&g_vol_mu);
    free(h);
    return rc;
}
