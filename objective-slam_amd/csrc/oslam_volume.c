/*
 * oslam_volume.c -- fusion of depth views into a TSDF volume and the ray cast back into a view (include/oslam.h at
 * oslam_volume_integrate): the host side of the kernels in oslam_volume.hip.  A call checks its arguments, zeroes a
 * counter block, runs one kernel and reads the counters back with one host wait.  oslam_volume_track is glue over the
 * ray cast and oslam_view_egomotion, oslam_volume_track_pyramid over the ray cast, a pyramid of it and
 * oslam_pyramid_egomotion (one body, track_from_raycast); oslam_view_to_cloud runs the depth front end's compaction
 * over a view's maps.  oslam_volume_shift moves the window of voxels the volume holds (k_tsdf_shift of oslam_shift.hip
 * into a second buffer, then a swap of the two), oslam_volume_follow decides such a move on the host,
 * oslam_volume_shift_world makes it through a voxel store that keeps what leaves and gives back what returns (the store:
 * oslam_world.c; kernels: oslam_reload.hip).  The extraction of
 * the fused volume, or of what a shift loses, as a cloud or a triangle list is oslam_surface.c (kernels: oslam_surface.hip
 * and oslam_mesh.hip).  The limits of a volume's sides and of a shift are oslam_kernels.h's.  A volume with colour
 * (oslam_colour.c) gets its colour pass from the integration's body here, in the same call, and its colour buffer moves
 * with every shift.
 */
#include <math.h>
#include <pthread.h>

#include "oslam_internal.h"
#include "oslam_world.h"

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

/* the origin of the window at vol->off, derived from the created origin and never accumulated (include/oslam.h at
 * oslam_volume_shift): one float multiply, then one float add */
static void window_origin(const oslam_volume *vol, const int off[3], float origin[3])
{
    int a;
    for (a = 0; a < 3; a++) {
        origin[a] = vol->p.origin[a];
        if (off[a] != 0) {
            const float step = (float)off[a] * vol->p.voxel;
            origin[a] = vol->p.origin[a] + step;
        }
    }
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
    window_origin(vol, vol->off, vol->k.origin);
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

/* ---- the shifting window (include/oslam.h at oslam_volume_shift; kernel: oslam_shift.hip) ---- */
/* the second buffers a shift needs, with g_vol_mu held and the volume's device bound: the TSDF's and, on a coloured
 * volume, the colours'.  Both exist afterwards or the call fails before anything moved */
static int shift_spares(oslam_volume *vol)
{
    uint32_t **want[2] = {&vol->spare, vol->colour.words ? &vol->colour_spare : NULL};
    int b;
    for (b = 0; b < 2; b++) {
        if (!want[b] || *want[b]) continue;
        if (hipMalloc((void **)want[b], oslam_volume_bytes(&vol->p)) != hipSuccess) {
            (void)hipGetLastError();
            *want[b] = NULL;
            return fail(OSLAM_E_NOMEM, "no device memory for the second buffer of the shift");
        }
    }
    return OSLAM_OK;
}

/* the colours of a coloured volume moved as k_tsdf_shift moves words, into colour_spare: launched behind the TSDF's shift;
 * scratch = a zeroed counter for the kernel's count, which nobody reads.  The caller swaps after its wait */
static int shift_colours(const oslam_volume *vol, const int shift[3], uint32_t *scratch, void *stream)
{
    oslamk_volume k = vol->k;
    k.words = vol->colour.words;
    return oslamk_tsdf_shift(&k, vol->colour_spare, shift, scratch, stream);
}

static void swap_colours(oslam_volume *vol)
{
    uint32_t *t = vol->colour.words;
    vol->colour.words = vol->colour_spare;
    vol->colour_spare = t;
}

int oslam_volume_shift(oslam_volume *vol, const int shift[3], oslam_shift_result *res)
{
    int rc = OSLAM_OK, a, off[3];
    const double t0 = now_ms();
    uint32_t *d_cnt = NULL, *spare = NULL, kept = 0;
    void *stream = oslam_stream();
    if (!vol || !shift) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!oslamk_shift_ok(shift)) return fail(OSLAM_E_INVALID, "a shift is at most 2^20 voxels");
    pthread_mutex_lock(&g_vol_mu);
    for (a = 0; a < 3; a++) off[a] = vol->off[a] + shift[a];
    if (!oslamk_shift_ok(off)) { rc = fail(OSLAM_E_INVALID, "the window's offset is at most 2^20 voxels"); goto done; }
    if (res) memset(res, 0, sizeof *res);
    if (!(shift[0] | shift[1] | shift[2])) {
        if (res) memcpy(res->offset, off, sizeof off);
        goto done;
    }
    if (hipSetDevice(vol->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    rc = shift_spares(vol);
    if (rc != OSLAM_OK) goto done;
    spare = vol->spare;
    KCHK(oslam_counters_open(&d_cnt, 0, stream));
    KCHK(oslamk_tsdf_shift(&vol->k, spare, shift, d_cnt, stream));
    if (vol->colour.words) KCHK(shift_colours(vol, shift, d_cnt + 1, stream));
    HIPCHK(hipMemcpyAsync(&kept, d_cnt, sizeof kept, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    vol->spare = vol->k.words;
    vol->k.words = spare;
    if (vol->colour.words) swap_colours(vol);
    memcpy(vol->off, off, sizeof off);
    window_origin(vol, vol->off, vol->k.origin);
    if (res) {
        memcpy(res->offset, off, sizeof off);
        res->kept = kept;
        res->launches = vol->colour.words ? 2 : 1;
    }
done:
    if (rc != OSLAM_OK && d_cnt) (void)hipStreamSynchronize((hipStream_t)stream);
    pthread_mutex_unlock(&g_vol_mu);
    if (d_cnt) oslam_dev_free(d_cnt);
    if (rc == OSLAM_OK && res) res->ms_total = (float)(now_ms() - t0);
    return rc;
}

/* ---- the shift through the voxel store (include/oslam.h at oslam_volume_shift_world; kernels: oslam_reload.hip; the
 * store: oslam_world.c) ---- */
int oslam_world_params_of(const oslam_volume *vol, oslam_world_params *p)
{
    if (!vol || !p) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(p, 0, sizeof *p);
    p->voxel = vol->p.voxel;
    memcpy(p->origin0, vol->p.origin, sizeof p->origin0);
    return OSLAM_OK;
}

/* The two passes of the pack, with g_vol_mu held and the volume's device bound: *n_rec = the seen voxels that leave
 * under shift; at most cap of them are packed, into *d_rec = device [n_rec][2] (NULL otherwise).  One host wait, for the
 * total; the second pass is only launched.  With colours (the volume's colour buffer, or NULL) *d_rec is [n_rec][2]
 * followed by [n_rec] colour words, gathered behind the second pass: one buffer, so one copy takes both down.  The caller
 * frees *d_cnt and *d_rec after its own wait */
static int pack_leaving(oslam_volume *vol, const int shift[3], size_t cap, const uint32_t *colours, uint32_t **d_cnt, uint32_t **d_rec,
                        uint32_t *n_rec, uint32_t *launches)
{
    int rc = OSLAM_OK;
    const uint32_t n_groups = oslamk_pack_groups(&vol->k);
    void *stream = oslam_stream();
    *n_rec = 0;
    KCHK(oslam_counters_open(d_cnt, n_groups, stream));            /* the total in the first 256 bytes, then one counter per workgroup */
    KCHK(oslamk_tsdf_pack_count(&vol->k, shift, n_groups, *d_cnt + 64, *d_cnt, stream));
    *launches += 2;
    HIPCHK(hipMemcpyAsync(n_rec, *d_cnt, sizeof *n_rec, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (*n_rec > 0 && (size_t)*n_rec <= cap) {
        KCHK(oslam_dev_alloc((void **)d_rec, sizeof(uint32_t) * (colours ? 3 : 2) * (size_t)*n_rec));
        KCHK(oslamk_tsdf_pack_emit(&vol->k, shift, n_groups, *d_cnt + 64, *n_rec, *d_rec, stream));
        *launches += 1;
        if (colours) {
            KCHK(oslamk_pack_colours(colours, vol->k.nx, vol->k.ny, vol->k.nz, *d_rec, *n_rec, *d_rec + 2 * (size_t)*n_rec, stream));
            *launches += 1;
        }
    }
done:
    return rc;
}

static void stage_release(void *p) { (void)hipHostFree(p); }

/* a pinned staging buffer of the store with room for bytes: grown by half as much again, so a stream of similar shifts
 * allocates once (oslam_world_surface.c stages the store's bricks through it too) */
int oslam_world_stage_fit(oslam_world_stage *st, size_t bytes)
{
    void *p = NULL;
    const size_t want = bytes + bytes / 2;
    if (st->bytes >= bytes) return OSLAM_OK;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OSLAM_E_NOMEM, "no pinned host memory for the records of the shift");
    }
    if (st->p) st->release(st->p);
    st->p = p;
    st->bytes = want;
    st->release = stage_release;
    return OSLAM_OK;
}

/* The entering region, the window at off_new minus the window at off_old in global coordinates, as at most 7 disjoint
 * boxes lo <= g < hi: axis by axis, the slabs of what remains that lie outside the old window, then the rest restricted
 * to the overlap; all of what remains as soon as an axis has no overlap.  -> the number of boxes */
static int entering_boxes(const int off_old[3], const int off_new[3], const unsigned n[3], int32_t lo[7][3], int32_t hi[7][3])
{
    int a, nb = 0;
    int32_t cl[3], ch[3];
    for (a = 0; a < 3; a++) {
        cl[a] = off_new[a];
        ch[a] = off_new[a] + (int)n[a];
    }
    for (a = 0; a < 3; a++) {
        const int32_t ol = cl[a] > off_old[a] ? cl[a] : off_old[a];
        const int32_t oh = ch[a] < off_old[a] + (int)n[a] ? ch[a] : off_old[a] + (int)n[a];
        if (ol >= oh) {
            memcpy(lo[nb], cl, sizeof cl);
            memcpy(hi[nb], ch, sizeof ch);
            return nb + 1;
        }
        if (cl[a] < ol) {
            memcpy(lo[nb], cl, sizeof cl);
            memcpy(hi[nb], ch, sizeof ch);
            hi[nb++][a] = ol;
        }
        if (oh < ch[a]) {
            memcpy(lo[nb], cl, sizeof cl);
            memcpy(hi[nb], ch, sizeof ch);
            lo[nb++][a] = oh;
        }
        cl[a] = ol;
        ch[a] = oh;
    }
    return nb;                                                      /* what remains is the overlap: it does not enter */
}

/* the global coordinate of the old window's voxel lin */
static void global_of(const oslam_volume *vol, uint32_t lin, int32_t g[3])
{
    const uint32_t row = lin / vol->p.nx;
    g[0] = (int32_t)(lin - row * vol->p.nx) + vol->off[0];
    g[1] = (int32_t)(row % vol->p.ny) + vol->off[1];
    g[2] = (int32_t)(row / vol->p.ny) + vol->off[2];
}

typedef struct enter_ctx {
    uint32_t *rec;                                                  /* [n][2]: lin in the new window, word */
    uint32_t *col;                                                  /* [n]: the colour stored with it, or NULL */
    size_t n;
    int off[3];
    size_t nx, ny;
} enter_ctx;

static void enter_record(void *ctx, const int32_t g[3], uint32_t word, uint32_t colour)
{
    enter_ctx *e = (enter_ctx *)ctx;
    e->rec[2 * e->n] = (uint32_t)(((size_t)(g[2] - e->off[2]) * e->ny + (size_t)(g[1] - e->off[1])) * e->nx + (size_t)(g[0] - e->off[0]));
    e->rec[2 * e->n + 1] = word;
    if (e->col) e->col[e->n] = colour;
    e->n++;
}

int oslam_volume_shift_world(oslam_volume *vol, oslam_world *w, const int shift[3], oslam_reload_result *res)
{
    int rc = OSLAM_OK, a, b, nb = 0, off[3], locked = 0, reserved = 0, cs = 0;
    const double t0 = now_ms();
    uint32_t *d_cnt = NULL, *d_out = NULL, *d_in = NULL, *d_kept = NULL, *spare = NULL;
    uint32_t n_out = 0, kept = 0, launches = 0, r;
    size_t n_in = 0, mark = 0, rec_words = 2;
    int32_t lo[7][3], hi[7][3], g[3];
    const uint32_t *rec_out = NULL, *col_out = NULL;
    oslam_world_stage *st = NULL;
    void *stream = oslam_stream();
    if (!vol || !w || !shift) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!oslamk_shift_ok(shift)) return fail(OSLAM_E_INVALID, "a shift is at most 2^20 voxels");
    pthread_mutex_lock(&g_vol_mu);
    for (a = 0; a < 3; a++) off[a] = vol->off[a] + shift[a];
    if (!oslamk_shift_ok(off)) { rc = fail(OSLAM_E_INVALID, "the window's offset is at most 2^20 voxels"); goto done; }
    if (!oslam_world_compatible(w, vol->p.voxel, vol->p.origin)) {
        rc = fail(OSLAM_E_INVALID, "the voxel store was made for another voxel size or origin");
        goto done;
    }
    cs = oslam_world_coloured(w);                                   /* fixed when the store was created */
    if (cs && !vol->colour.words) {
        rc = fail(OSLAM_E_INVALID, "a colour store needs a volume with colour");
        goto done;
    }
    rec_words = cs ? 3 : 2;                                         /* a record crosses the host link as 12 bytes or as 8 */
    if (res) memset(res, 0, sizeof *res);
    if (!(shift[0] | shift[1] | shift[2])) {
        if (res) memcpy(res->offset, off, sizeof off);
        goto done;
    }
    if (hipSetDevice(vol->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    rc = shift_spares(vol);
    if (rc != OSLAM_OK) goto done;
    spare = vol->spare;
    /* 1. pack what leaves, with its colours for a colour store, and copy it down */
    rc = pack_leaving(vol, shift, (size_t)-1, cs ? vol->colour.words : NULL, &d_cnt, &d_out, &n_out, &launches);
    if (rc != OSLAM_OK) goto done;
    oslam_world_lock(w);
    locked = 1;
    st = oslam_world_stages(w);
    if (n_out) {
        rc = oslam_world_stage_fit(&st[0], sizeof(uint32_t) * rec_words * (size_t)n_out);
        if (rc != OSLAM_OK) goto done;
        HIPCHK(hipMemcpyAsync(st[0].p, d_out, sizeof(uint32_t) * rec_words * (size_t)n_out, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        rec_out = (const uint32_t *)st[0].p;
        if (cs) col_out = rec_out + 2 * (size_t)n_out;
    }
    /* 2. the bricks the leaving records need, still empty */
    mark = oslam_world_mark(w);
    reserved = 1;
    for (r = 0; r < n_out; r++) {
        global_of(vol, rec_out[2 * r], g);
        rc = oslam_world_reserve(w, g);
        if (rc != OSLAM_OK) goto done;
    }
    /* 3. the entering records: counted, then read; the store does not change */
    {
        const unsigned n[3] = {vol->p.nx, vol->p.ny, vol->p.nz};
        nb = entering_boxes(vol->off, off, n, lo, hi);
    }
    for (b = 0; b < nb; b++) n_in += oslam_world_visit(w, lo[b], hi[b], 0, NULL, NULL);
    if (n_in) {
        enter_ctx e;
        rc = oslam_world_stage_fit(&st[1], sizeof(uint32_t) * rec_words * n_in);
        if (rc != OSLAM_OK) goto done;
        e.rec = (uint32_t *)st[1].p;
        e.col = cs ? e.rec + 2 * n_in : NULL;
        e.n = 0;
        memcpy(e.off, off, sizeof off);
        e.nx = vol->p.nx;
        e.ny = vol->p.ny;
        for (b = 0; b < nb; b++) (void)oslam_world_visit_colour(w, lo[b], hi[b], 0, enter_record, &e);
        /* 4. copy up; shift and unpack in stream order */
        KCHK(oslam_dev_alloc((void **)&d_in, sizeof(uint32_t) * rec_words * n_in));
        HIPCHK(hipMemcpyAsync(d_in, st[1].p, sizeof(uint32_t) * rec_words * n_in, hipMemcpyHostToDevice, (hipStream_t)stream));
    }
    KCHK(oslam_counters_open(&d_kept, 0, stream));
    KCHK(oslamk_tsdf_shift(&vol->k, spare, shift, d_kept, stream));
    launches++;
    if (vol->colour.words) {                                            /* a plain store keeps no colour: what it reloads has wc = 0 */
        KCHK(shift_colours(vol, shift, d_kept + 1, stream));
        launches++;
        if (cs && n_in) {                                               /* a colour store's colours, into the buffer that shift wrote */
            KCHK(oslamk_unpack_colours(vol->colour_spare, vol->k.nx, vol->k.ny, vol->k.nz, d_in, d_in + 2 * n_in, (uint32_t)n_in, stream));
            launches++;
        }
    }
    if (n_in) {
        KCHK(oslamk_tsdf_unpack(spare, vol->k.nx, vol->k.ny, vol->k.nz, d_in, (uint32_t)n_in, stream));
        launches++;
    }
    HIPCHK(hipMemcpyAsync(&kept, d_kept, sizeof kept, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    /* 5. commit: nothing below can fail */
    for (r = 0; r < n_out; r++) {
        global_of(vol, rec_out[2 * r], g);
        oslam_world_store_colour(w, g, rec_out[2 * r + 1], col_out ? col_out[r] : 0u);
    }
    for (b = 0; b < nb; b++) (void)oslam_world_visit(w, lo[b], hi[b], 1, NULL, NULL);
    reserved = 0;
    vol->spare = vol->k.words;
    vol->k.words = spare;
    if (vol->colour.words) swap_colours(vol);
    memcpy(vol->off, off, sizeof off);
    window_origin(vol, vol->off, vol->k.origin);
    if (res) {
        memcpy(res->offset, off, sizeof off);
        res->kept = kept + (uint32_t)n_in;                          /* the reloaded words are seen and their voxels were 0 */
        res->stored = n_out;
        res->reloaded = (uint32_t)n_in;
        res->launches = launches;
    }
done:
    if (rc != OSLAM_OK && d_cnt) (void)hipStreamSynchronize((hipStream_t)stream);
    if (reserved) oslam_world_rollback(w, mark);
    if (locked) oslam_world_unlock(w);
    pthread_mutex_unlock(&g_vol_mu);
    if (d_kept) oslam_dev_free(d_kept);
    if (d_in) oslam_dev_free(d_in);
    if (d_out) oslam_dev_free(d_out);
    if (d_cnt) oslam_dev_free(d_cnt);
    if (rc == OSLAM_OK && res) res->ms_total = (float)(now_ms() - t0);
    return rc;
}

/* the tap of the pack, without colours (colour_out == NULL, want_colour == 0) or with them */
static int pack_tap(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, uint32_t *colour_out, int want_colour,
                    size_t cap, size_t *n_out)
{
    int rc = OSLAM_OK;
    uint32_t *d_cnt = NULL, *d_rec = NULL, *h = NULL, n = 0, launches = 0, r;
    const size_t rec_words = want_colour ? 3 : 2;
    if (!vol || !shift || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (cap != 0 && (!lin_out || !word_out || (want_colour && !colour_out)))
        return fail(OSLAM_E_INVALID, "the outputs must be given with cap != 0");
    if (want_colour && !vol->colour.words) return fail(OSLAM_E_INVALID, "the volume has no colour");
    if (!oslamk_shift_ok(shift)) return fail(OSLAM_E_INVALID, "a shift is at most 2^20 voxels");
    *n_out = 0;
    if (!(shift[0] | shift[1] | shift[2])) return OSLAM_OK;
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    pthread_mutex_lock(&g_vol_mu);
    rc = pack_leaving(vol, shift, cap, want_colour ? vol->colour.words : NULL, &d_cnt, &d_rec, &n, &launches);
    if (rc != OSLAM_OK) goto done;
    *n_out = n;
    if (cap != 0 && (size_t)n > cap) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    if (d_rec) {
        h = (uint32_t *)malloc(sizeof(uint32_t) * rec_words * (size_t)n);
        if (!h) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        HIPCHK(hipMemcpy(h, d_rec, sizeof(uint32_t) * rec_words * (size_t)n, hipMemcpyDeviceToHost));
        for (r = 0; r < n; r++) {
            lin_out[r] = h[2 * r];
            word_out[r] = h[2 * r + 1];
            if (want_colour) colour_out[r] = h[2 * (size_t)n + r];
        }
    }
done:
    if (d_cnt) (void)hipStreamSynchronize((hipStream_t)oslam_stream());
    pthread_mutex_unlock(&g_vol_mu);
    free(h);
    if (d_rec) oslam_dev_free(d_rec);
    if (d_cnt) oslam_dev_free(d_cnt);
    return rc;
}

int oslam_volume_pack(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, size_t cap, size_t *n_out)
{
    return pack_tap(vol, shift, lin_out, word_out, NULL, 0, cap, n_out);
}

int oslam_volume_pack_colour(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, uint32_t *colour_out,
                             size_t cap, size_t *n_out)
{
    return pack_tap(vol, shift, lin_out, word_out, colour_out, 1, cap, n_out);
}

int oslam_volume_window(oslam_volume *vol, int offset_out[3], float origin_out[3])
{
    if (!vol || !offset_out || !origin_out) return fail(OSLAM_E_INVALID, "NULL argument");
    pthread_mutex_lock(&g_vol_mu);
    memcpy(offset_out, vol->off, sizeof vol->off);
    memcpy(origin_out, vol->k.origin, sizeof vol->k.origin);
    pthread_mutex_unlock(&g_vol_mu);
    return OSLAM_OK;
}

int oslam_follow_params_default(const oslam_volume *vol, oslam_follow_params *fp)
{
    unsigned n_min;
    if (!vol || !fp) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(fp, 0, sizeof *fp);
    n_min = vol->p.nx < vol->p.ny ? vol->p.nx : vol->p.ny;
    if (vol->p.nz < n_min) n_min = vol->p.nz;
    fp->lookahead = (float)(0.5 * (double)vol->p.nz * (double)vol->p.voxel);
    fp->threshold = (float)n_min / 4.0f;
    fp->granule = 8;
    return OSLAM_OK;
}

int oslam_volume_follow(oslam_volume *vol, const float T_vol_cam[16], const oslam_follow_params *fp, int shift_out[3])
{
    int rc, a, moved = 0;
    oslam_follow_params p;
    float origin[3];
    double d[3];
    if (!vol || !T_vol_cam || !shift_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (fp && (!isfinite(fp->lookahead) || !isfinite(fp->threshold) || !(fp->lookahead >= 0.0f) || !(fp->threshold >= 0.0f)))
        return fail(OSLAM_E_INVALID, "lookahead and threshold must be finite and not negative");
    if (fp && (fp->granule < 1 || fp->granule > 64)) return fail(OSLAM_E_INVALID, "granule must lie in 1..64");
    rc = oslam_refine_check_rigid(T_vol_cam);
    if (rc != OSLAM_OK) return rc;
    if (fp) p = *fp;
    else oslam_follow_params_default(vol, &p);
    pthread_mutex_lock(&g_vol_mu);
    memcpy(origin, vol->k.origin, sizeof origin);
    pthread_mutex_unlock(&g_vol_mu);
    {
        const unsigned n[3] = {vol->p.nx, vol->p.ny, vol->p.nz};
        const double h = (double)vol->p.voxel;
        for (a = 0; a < 3; a++) {
            const double c = (double)T_vol_cam[4 * a + 3] + (double)p.lookahead * (double)T_vol_cam[4 * a + 2];
            const double centre = (double)origin[a] + 0.5 * (double)n[a] * h;
            d[a] = (c - centre) / h;
            if (!(fabs(d[a]) <= (double)p.threshold)) moved = 1;
        }
        for (a = 0; a < 3; a++) {
            double s = moved ? (double)p.granule * rint(d[a] / (double)p.granule) : 0.0;
            if (s > (double)n[a]) s = (double)n[a];
            if (s < -(double)n[a]) s = -(double)n[a];
            shift_out[a] = (int)s;
        }
    }
    return OSLAM_OK;
}
