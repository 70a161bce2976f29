/*
 * oslam_track.c -- tracking across depth frames by projective ICP (include/oslam.h at oslam_track): the host side of the
 * kernels in oslam_track.hip.  A call checks its arguments, builds the view's vertex and normal map when it does not
 * exist yet, uploads one descriptor per hypothesis, runs k_track once for all of them and reads one record per
 * hypothesis back into pinned memory with one host wait.
 */
#include <math.h>
#include <pthread.h>

#include "oslam_internal.h"

/* the pinned records of a call, [OSLAMK_ARB_MAX_HYP]: one for the process, so tracking calls take turns; the same lock
 * guards the lazy build of a view's maps */
static oslamk_track_rec *g_rec;
static pthread_mutex_t g_track_mu = PTHREAD_MUTEX_INITIALIZER;

void oslam_track_release(void)
{
    pthread_mutex_lock(&g_track_mu);
    if (g_rec) (void)hipHostFree(g_rec);
    g_rec = NULL;
    pthread_mutex_unlock(&g_track_mu);
}

void oslam_track_release_maps(oslam_view *v)
{
    /* every call that read the maps ended with a synchronisation of its stream */
    oslam_dev_free(v->d_maps);
    v->d_maps = NULL;
}

int oslam_track_params_default(oslam_track_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->max_iterations = 10;
    p->max_corr_dist = 2.0f;
    p->min_normal_dot = 0.8f;
    p->stop_rot = 1e-5f;
    p->stop_trans = 1e-4f;
    oslam_verify_params_default(&p->verify);
    return OSLAM_OK;
}

int oslam_track_check_params(const oslam_track_params *tp, oslam_track_params *out)
{
    oslam_verify_params vp;
    if (tp) *out = *tp;
    else oslam_track_params_default(out);
    if (!isfinite(out->max_corr_dist) || !isfinite(out->min_normal_dot) || !isfinite(out->stop_rot) ||
        !isfinite(out->stop_trans))
        return fail(OSLAM_E_INVALID, "track parameters must be finite");
    if (!(out->max_corr_dist > 0.0f)) return fail(OSLAM_E_INVALID, "max_corr_dist must be > 0");
    if (out->max_iterations > 1000) return fail(OSLAM_E_INVALID, "max_iterations above 1000");
    if (out->stop_rot < 0.0f || out->stop_trans < 0.0f) return fail(OSLAM_E_INVALID, "negative stop criterion");
    return oslam_verify_check_params(&out->verify, &vp);
}

/* The view's maps, built on first use (enqueued on the stream; *built = 1).  Called with g_track_mu held and the view's
 * device bound.  The block lives as long as the view and goes back to the kept blocks of the scene path with it: the
 * next frame's view takes it again without a hipMalloc / hipFree pair. */
static int view_maps(oslam_view *v, int *built)
{
    int rc = OSLAM_OK;
    const size_t n_pix = (size_t)v->k.w * (size_t)v->k.h;
    *built = 0;
    if (v->d_maps) return OSLAM_OK;
    KCHK(oslam_dev_alloc((void **)&v->d_maps, sizeof(float) * 8 * n_pix));
    KCHK(oslamk_view_normals(&v->k, v->max_jump, v->d_maps, oslam_stream()));
    *built = 1;
done:
    if (rc != OSLAM_OK && v->d_maps) {
        (void)hipStreamSynchronize((hipStream_t)oslam_stream());
        oslam_dev_free(v->d_maps);
        v->d_maps = NULL;
    }
    return rc;
}

int oslam_track_view_maps(oslam_view *v, int *built)
{
    int rc;
    pthread_mutex_lock(&g_track_mu);
    rc = view_maps(v, built);
    pthread_mutex_unlock(&g_track_mu);
    return rc;
}

/* the descriptor of one hypothesis: the pose bookkeeping of oslam_refine (oslam_refine.c, set_pose) */
static void set_member(oslamk_track_member *d, const oslam_model *m, const float T[16], const oslam_track_params *p)
{
    const float rc_ = p->max_corr_dist * m->d_dist;
    double c[3];
    int a;
    memcpy(d->cm, m->cm, sizeof d->cm);
    for (a = 0; a < 12; a++) d->T[a] = (double)T[a];
    oslam_rigid_apply(d->T, d->cm, c);
    for (a = 0; a < 3; a++) d->c[a] = (float)c[a];
    d->m = m->c.k;
    d->r2_corr = rc_ * rc_;
    d->min_dot = p->min_normal_dot;
    d->stop_rot = p->stop_rot;
    d->stop_trans = p->stop_trans * m->d_dist;
    d->tol = (float)((double)p->verify.depth_tol * (double)m->d_dist);
    d->max_iter = p->max_iterations;
    d->n_blocks = (uint32_t)(((size_t)m->c.n + OSLAMK_TRACK_THREADS - 1) / OSLAMK_TRACK_THREADS);
}

/* hypotheses ms[0 .. H) with T_prev [H][16] (all-zero = skipped) against v: the whole stage */
static int track_members(oslam_model *const *ms, size_t H, const oslam_view *v, const float *T_prev,
                         const oslam_track_params *p, float *T_out, oslam_track_result *res)
{
    int rc = OSLAM_OK, locked = 0, built = 0, any = 0;
    const double t0 = now_ms();
    size_t h, off_rec;
    oslamk_track_member *hm = NULL;
    uint32_t launches = 0;
    char *dev = NULL;
    void *stream = oslam_stream();

    memset(T_out, 0, sizeof(float) * 16 * H);
    if (res) memset(res, 0, sizeof *res * H);
    hm = (oslamk_track_member *)calloc(H, sizeof *hm);
    if (!hm) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (h = 0; h < H; h++)
        if (!oslam_is_zero_pose(T_prev + 16 * h)) {
            set_member(&hm[h], ms[h], T_prev + 16 * h, p);
            any = 1;
        }
    if (!any) goto done;                        /* every hypothesis skipped: no device work */
    if (hipSetDevice(v->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    pthread_mutex_lock(&g_track_mu);
    locked = 1;
    if (!g_rec) HIPCHK(hipHostMalloc((void **)&g_rec, sizeof *g_rec * OSLAMK_ARB_MAX_HYP, hipHostMallocPortable));
    off_rec = align256(sizeof *hm * H);
    KCHK(oslam_dev_alloc((void **)&dev, off_rec + sizeof(oslamk_track_rec) * H));
    HIPCHK(hipMemcpyAsync(dev, hm, sizeof *hm * H, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = view_maps((oslam_view *)v, &built);    /* the maps are a cache of the view: building them does not change it */
    if (rc != OSLAM_OK) goto done;
    if (built) launches++;
    KCHK(oslamk_track(&v->k, v->d_maps, (const oslamk_track_member *)dev, (uint32_t)H, (int)p->verify.window,
                      (oslamk_track_rec *)(dev + off_rec), stream));
    launches++;
    HIPCHK(hipMemcpyAsync(g_rec, dev + off_rec, sizeof *g_rec * H, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (h = 0; h < H; h++) {
        const oslamk_track_rec *k = &g_rec[h];
        float *T = T_out + 16 * h;
        int a;
        if (hm[h].n_blocks == 0) continue;
        for (a = 0; a < 12; a++) T[a] = k->T[a];
        T[15] = 1.0f;
        if (res) {
            oslam_track_result *r = &res[h];
            oslam_verify_fill_result(&r->verify, k->counts, &p->verify);
            r->iterations = k->iterations;
            r->correspondences = k->n_corr;
            r->converged = k->converged;
            r->found = r->verify.found;
        }
    }
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);    /* nothing may still use the block */
    if (locked) pthread_mutex_unlock(&g_track_mu);
    if (dev) oslam_dev_free(dev);
    if (rc == OSLAM_OK && res) {
        const float ms_total = (float)(now_ms() - t0);
        for (h = 0; h < H; h++) {
            res[h].launches = launches;
            res[h].ms_total = ms_total;
            if (hm[h].n_blocks) {
                res[h].verify.launches = launches;
                res[h].verify.ms_total = ms_total;
            }
        }
    }
    free(hm);
    return rc;
}

int oslam_track(oslam_model *const *models, const float *T_prev, size_t H, const oslam_view *v, const oslam_track_params *tp,
                float *T_out, oslam_track_result *res)
{
    oslam_track_params p;
    int rc;
    if (!models || !T_prev || !v || !T_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_track_check_params(tp, &p);
    if (rc == OSLAM_OK) rc = oslam_check_poses(models, T_prev, H, 1);
    if (rc == OSLAM_OK) rc = oslam_check_handles(models, T_prev, H, v);
    if (rc != OSLAM_OK) return rc;
    return track_members(models, H, v, T_prev, &p, T_out, res);
}

int oslam_db_track(oslam_db *db, const uint32_t *member, const float *T_prev, size_t H, const oslam_view *v,
                   const oslam_track_params *tp, float *T_out, oslam_track_result *res)
{
    oslam_track_params p;
    oslam_model **ms;
    size_t h;
    int rc;
    if (!db || !member || !T_prev || !v || !T_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_track_check_params(tp, &p);
    if (rc == OSLAM_OK) rc = oslam_check_poses(NULL, T_prev, H, 1);    /* the members' models are not looked up yet */
    if (rc != OSLAM_OK) return rc;
    for (h = 0; h < H; h++)
        if (member[h] >= db->n) return fail(OSLAM_E_INVALID, "member index outside the database");
    ms = (oslam_model **)malloc(sizeof *ms * H);
    if (!ms) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (h = 0; h < H; h++) ms[h] = db->models[member[h]];
    rc = oslam_check_handles(ms, T_prev, H, v);
    if (rc == OSLAM_OK) rc = track_members(ms, H, v, T_prev, &p, T_out, res);
    free(ms);
    return rc;
}

/* the maps of the view on the host: what both taps read */
static int maps_to_host(oslam_view *v, float **maps_out)
{
    int rc = OSLAM_OK, built = 0;
    const size_t n_pix = (size_t)v->k.w * (size_t)v->k.h;
    float *hmaps = (float *)malloc(sizeof(float) * 8 * n_pix);
    *maps_out = NULL;
    if (!hmaps) return fail(OSLAM_E_NOMEM, "host allocation failed");
    if (hipSetDevice(v->dev) != hipSuccess) { free(hmaps); return fail(OSLAM_E_DEVICE, "hipSetDevice failed"); }
    pthread_mutex_lock(&g_track_mu);
    rc = view_maps(v, &built);
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipMemcpyAsync(hmaps, v->d_maps, sizeof(float) * 8 * n_pix, hipMemcpyDeviceToHost, (hipStream_t)oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)oslam_stream());
    pthread_mutex_unlock(&g_track_mu);
    if (rc != OSLAM_OK) free(hmaps);
    else *maps_out = hmaps;
    return rc;
}

int oslam_view_normals(oslam_view *v, float *nrm_out, uint8_t *has_normal_out)
{
    float *hmaps;
    size_t i, n_pix;
    int rc;
    if (!v || !nrm_out || !has_normal_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = maps_to_host(v, &hmaps);
    if (rc != OSLAM_OK) return rc;
    n_pix = (size_t)v->k.w * (size_t)v->k.h;
    for (i = 0; i < n_pix; i++) {
        memcpy(nrm_out + 3 * i, hmaps + 8 * i + 4, 3 * sizeof(float));
        has_normal_out[i] = hmaps[8 * i + 3] != 0.0f;
    }
    free(hmaps);
    return OSLAM_OK;
}

int oslam_view_vertices(oslam_view *v, float *vtx_out)
{
    float *hmaps;
    size_t i, n_pix;
    int rc;
    if (!v || !vtx_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = maps_to_host(v, &hmaps);
    if (rc != OSLAM_OK) return rc;
    n_pix = (size_t)v->k.w * (size_t)v->k.h;
    for (i = 0; i < n_pix; i++) memcpy(vtx_out + 3 * i, hmaps + 8 * i, 3 * sizeof(float));
    free(hmaps);
    return OSLAM_OK;
}

int oslam_track_correspondences(oslam_model *m, const oslam_view *v, const float T[16], float max_corr_dist,
                                float min_normal_dot, int32_t *pixel_out)
{
    oslam_track_params p;
    oslamk_track_member h;
    char *dev = NULL;
    void *stream = oslam_stream();
    size_t M, off_pix;
    int rc, built = 0, locked = 0;
    if (!m || !v || !T || !pixel_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!(max_corr_dist > 0.0f) || !isfinite(max_corr_dist) || !isfinite(min_normal_dot))
        return fail(OSLAM_E_INVALID, "bad max_corr_dist or normal gate");
    rc = oslam_refine_check_rigid(T);
    if (rc == OSLAM_OK) rc = oslam_view_check_pair(m, v);
    if (rc != OSLAM_OK) return rc;
    if (hipSetDevice(v->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_track_params_default(&p);
    p.max_corr_dist = max_corr_dist;
    p.min_normal_dot = min_normal_dot;
    M = (size_t)m->c.n;
    memset(&h, 0, sizeof h);
    set_member(&h, m, T, &p);
    off_pix = align256(sizeof h);
    pthread_mutex_lock(&g_track_mu);
    locked = 1;
    KCHK(oslam_dev_alloc((void **)&dev, off_pix + sizeof(int32_t) * M));
    HIPCHK(hipMemcpyAsync(dev, &h, sizeof h, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = view_maps((oslam_view *)v, &built);
    if (rc != OSLAM_OK) goto done;
    KCHK(oslamk_track_corr(&v->k, v->d_maps, (const oslamk_track_member *)dev, h.n_blocks, (int32_t *)(dev + off_pix), stream));
    HIPCHK(hipMemcpyAsync(pixel_out, dev + off_pix, sizeof(int32_t) * M, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    if (locked) pthread_mutex_unlock(&g_track_mu);
    if (dev) oslam_dev_free(dev);
    return rc;
}
