/*
 * oslam_ego.c -- camera motion between two depth views by dense projective ICP (include/oslam.h at
 * oslam_view_egomotion): the host side of the kernels in oslam_ego.hip.  A call checks its arguments, builds the maps of
 * its views when they do not exist yet, uploads the state, zeroes the arrival counters, enqueues one k_ego_step per
 * scheduled iteration back to back and reads the state back into pinned memory with one host wait.  Every level of the
 * schedule has its own source and destination view: oslam_view_egomotion runs all of them on one pair,
 * oslam_pyramid_egomotion on the matching levels of two pyramids (oslam_pyramid.c).
 */
#include <math.h>
#include <pthread.h>

#include "oslam_internal.h"

/* the pinned state of a call: one for the process, so egomotion calls take turns (on every device; the lock is held
 * across the host wait).  Lock order: g_ego_mu, then the lock of the views' maps inside oslam_track_view_maps. */
static oslamk_ego_state *g_state;
static pthread_mutex_t g_ego_mu = PTHREAD_MUTEX_INITIALIZER;

void oslam_ego_release(void)
{
    pthread_mutex_lock(&g_ego_mu);
    if (g_state) (void)hipHostFree(g_state);
    g_state = NULL;
    pthread_mutex_unlock(&g_ego_mu);
}

int oslam_egomotion_params_default(oslam_egomotion_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->n_levels = 3;
    p->level[0].stride = 4;
    p->level[0].max_iterations = 4;
    p->level[1].stride = 2;
    p->level[1].max_iterations = 5;
    p->level[2].stride = 1;
    p->level[2].max_iterations = 10;
    p->max_corr_dist = 0.30f;
    p->min_normal_dot = 0.93969262f;
    p->stop_rot = 1e-5f;
    p->stop_trans = 1e-5f;
    p->min_overlap = 0.75f;
    return OSLAM_OK;
}

static int check_params(const oslam_egomotion_params *ep, oslam_egomotion_params *out)
{
    unsigned l;
    if (ep) *out = *ep;
    else oslam_egomotion_params_default(out);
    if (!isfinite(out->max_corr_dist) || !isfinite(out->min_normal_dot) || !isfinite(out->stop_rot) ||
        !isfinite(out->stop_trans) || !isfinite(out->min_overlap))
        return fail(OSLAM_E_INVALID, "egomotion parameters must be finite");
    if (out->n_levels < 1 || out->n_levels > OSLAM_EGOMOTION_MAX_LEVELS)
        return fail(OSLAM_E_INVALID, "n_levels must lie in 1..OSLAM_EGOMOTION_MAX_LEVELS");
    for (l = 0; l < out->n_levels; l++) {
        if (out->level[l].stride < 1 || out->level[l].stride > 16) return fail(OSLAM_E_INVALID, "a stride outside 1..16");
        if (out->level[l].max_iterations > 1000) return fail(OSLAM_E_INVALID, "max_iterations above 1000");
    }
    if (!(out->max_corr_dist > 0.0f)) return fail(OSLAM_E_INVALID, "max_corr_dist must be > 0");
    if (out->stop_rot < 0.0f || out->stop_trans < 0.0f) return fail(OSLAM_E_INVALID, "negative stop criterion");
    if (out->min_overlap < 0.0f || out->min_overlap > 1.0f) return fail(OSLAM_E_INVALID, "min_overlap must lie in [0, 1]");
    return OSLAM_OK;
}

int oslam_ego_check_params(const oslam_egomotion_params *ep, oslam_egomotion_params *out) { return check_params(ep, out); }

static const float k_identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

/* the lattice of level l of p over its source image, every stride-th pixel (include/oslam.h, "Levels" and "Step") */
static void set_level(oslamk_ego_level *lv, const oslam_egomotion_params *p, unsigned l, const oslamk_view *src, unsigned stride)
{
    const int s = (int)stride;
    unsigned q;
    lv->stride = s;
    lv->lw = (src->w + s - 1) / s;
    lv->n = (uint32_t)lv->lw * (uint32_t)((src->h + s - 1) / s);
    lv->n_blocks = (lv->n + OSLAMK_EGO_THREADS - 1) / OSLAMK_EGO_THREADS;
    lv->chunk = (lv->n_blocks + OSLAMK_EGO_MAX_SLOTS - 1) / OSLAMK_EGO_MAX_SLOTS;
    lv->n_slots = (lv->n_blocks + lv->chunk - 1) / lv->chunk;
    lv->max_iter = p->level[l].max_iterations;
    lv->level = (int32_t)l;
    for (q = l + 1; q < p->n_levels && p->level[q].max_iterations == 0; q++) {}
    lv->next_level = (int32_t)q;
}

int oslam_ego_run(const oslam_ego_pair *pair, const float T0[16], const oslam_egomotion_params *p, float T_out[16],
                  oslam_egomotion_result *res)
{
    int rc = OSLAM_OK, locked = 0, built = 0, a, finest = -1;
    const double t0 = now_ms();
    oslamk_ego_state st;
    oslamk_ego_level lv[OSLAMK_EGO_MAX_LEVELS];
    uint32_t launches = 0, scheduled = 0, it, k = 0;
    unsigned l, first;
    size_t off_cnt, off_slots;
    char *dev = NULL;
    void *stream = oslam_stream();

    memcpy(T_out, T0, 16 * sizeof(float));
    if (res) memset(res, 0, sizeof *res);
    for (l = 0; l < p->n_levels; l++) {
        set_level(&lv[l], p, l, &pair[l].src->k, pair[l].lattice);
        scheduled += lv[l].max_iter;
    }
    if (scheduled == 0) goto done;              /* nothing to run: the pose as given, overlap 0 */
    for (first = 0; p->level[first].max_iterations == 0; first++) {}
    memset(&st, 0, sizeof st);
    for (a = 0; a < 12; a++) {
        st.T[a] = (double)T0[a];
        st.Tf[a] = T0[a];
    }
    for (a = 0; a < 3; a++) st.c[a] = T0[4 * a + 3];
    st.r2_corr = p->max_corr_dist * p->max_corr_dist;
    st.min_dot = p->min_normal_dot;
    st.stop_rot = p->stop_rot;
    st.stop_trans = p->stop_trans;
    st.level = (int32_t)first;
    st.n_levels = (int32_t)p->n_levels;

    if (hipSetDevice(pair[first].src->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    pthread_mutex_lock(&g_ego_mu);
    locked = 1;
    if (!g_state) HIPCHK(hipHostMalloc((void **)&g_state, sizeof *g_state, hipHostMallocPortable));
    off_cnt = align256(sizeof st);
    off_slots = off_cnt + align256(sizeof(uint32_t) * scheduled);
    KCHK(oslam_dev_alloc((void **)&dev, off_slots + sizeof(double) * OSLAMK_EGO_SLOT * OSLAMK_EGO_MAX_SLOTS));
    HIPCHK(hipMemcpyAsync(dev, &st, sizeof st, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(dev + off_cnt, 0, sizeof(uint32_t) * scheduled, (hipStream_t)stream));
    for (l = first; l < p->n_levels; l++) {     /* the maps of every view a level runs on; a view that has them builds nothing */
        if (lv[l].max_iter == 0) continue;
        rc = oslam_track_view_maps(pair[l].src, &built);
        if (rc != OSLAM_OK) goto done;
        launches += (uint32_t)built;
        rc = oslam_track_view_maps(pair[l].dst, &built);
        if (rc != OSLAM_OK) goto done;
        launches += (uint32_t)built;
    }
    for (l = 0; l < p->n_levels; l++)
        for (it = 0; it < lv[l].max_iter; it++, k++) {
            oslam_view *src = pair[l].src, *dst = pair[l].dst;
            KCHK(oslamk_ego_step(&src->k, src->d_maps, &dst->k, dst->d_maps, &lv[l], (oslamk_ego_state *)dev,
                                 (double *)(dev + off_slots), (uint32_t *)(dev + off_cnt) + k, stream));
            launches++;
        }
    HIPCHK(hipMemcpyAsync(g_state, dev, sizeof *g_state, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (a = 0; a < 12; a++) T_out[a] = g_state->Tf[a];
    if (res) {
        for (l = 0; l < p->n_levels; l++) {
            res->iterations[l] = g_state->iterations[l];
            /* the level with the smallest stride that evaluated a step, the later of equal strides */
            if ((g_state->iterations[l] > 0 || (int32_t)l == g_state->level) &&
                (finest < 0 || p->level[l].stride <= p->level[finest].stride))
                finest = (int)l;
        }
        res->correspondences = g_state->last_corr;
        res->rmse = g_state->rmse;
        if (finest >= 0 && g_state->n_src[finest] > 0)
            res->overlap = (float)g_state->corr[finest] / (float)g_state->n_src[finest];
        res->converged = g_state->converged;
    }
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);    /* nothing may still use the block */
    if (locked) pthread_mutex_unlock(&g_ego_mu);
    if (dev) oslam_dev_free(dev);
    if (rc == OSLAM_OK && res) {
        res->ok = res->overlap >= p->min_overlap;
        res->launches = launches;
        res->ms_total = (float)(now_ms() - t0);
    }
    return rc;
}

/* everything that can be said without reading a handle */
static int check_call(const void *src, const void *dst, const float *T, const oslam_egomotion_params *ep,
                      oslam_egomotion_params *p)
{
    int rc;
    if (!src || !dst) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_params(ep, p);
    if (rc == OSLAM_OK && T) rc = oslam_refine_check_rigid(T);
    return rc;
}

/* src == dst: the identity at once, without a device */
static void same_handle(const oslam_egomotion_params *p, float T_out[16], oslam_egomotion_result *res)
{
    memcpy(T_out, k_identity, sizeof k_identity);
    if (res) {
        memset(res, 0, sizeof *res);
        res->converged = 1;
        res->overlap = 1.0f;
        res->ok = 1.0f >= p->min_overlap;
    }
}

int oslam_ego_check_pyramid_schedule(const oslam_egomotion_params *p, unsigned n_levels)
{
    unsigned l;
    for (l = 0; l < p->n_levels; l++) {
        const unsigned s = p->level[l].stride;
        if (s != 1 && s != 2 && s != 4) return fail(OSLAM_E_INVALID, "a stride of a pyramid schedule must be 1, 2 or 4");
        if ((s >> 1) >= n_levels)               /* s >> 1: log2 of 1, 2, 4 */
            return fail(OSLAM_E_INVALID, "a stride names a level the pyramid does not have");
    }
    return OSLAM_OK;
}

int oslam_view_egomotion(oslam_view *src, oslam_view *dst, const float T_init[16], const oslam_egomotion_params *ep,
                         float T_out[16], oslam_egomotion_result *res)
{
    oslam_egomotion_params p;
    oslam_ego_pair pair[OSLAM_EGOMOTION_MAX_LEVELS];
    unsigned l;
    int rc;
    if (!T_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_call(src, dst, T_init, ep, &p);
    if (rc != OSLAM_OK) return rc;
    if (src == dst) {
        same_handle(&p, T_out, res);
        return OSLAM_OK;
    }
    if (src->dev != dst->dev) return fail(OSLAM_E_INVALID, "the two views live on different devices");
    for (l = 0; l < p.n_levels; l++) {          /* every level on the one pair, its stride over the source */
        pair[l].src = src;
        pair[l].dst = dst;
        pair[l].lattice = p.level[l].stride;
    }
    return oslam_ego_run(pair, T_init ? T_init : k_identity, &p, T_out, res);
}

int oslam_pyramid_egomotion(oslam_pyramid *src, oslam_pyramid *dst, const float T_init[16], const oslam_egomotion_params *ep,
                            float T_out[16], oslam_egomotion_result *res)
{
    oslam_egomotion_params p;
    oslam_ego_pair pair[OSLAM_EGOMOTION_MAX_LEVELS];
    unsigned l;
    int rc;
    if (!T_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_call(src, dst, T_init, ep, &p);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_ego_check_pyramid_schedule(&p, UINT_MAX);     /* the strides alone, before a handle is read */
    if (rc != OSLAM_OK) return rc;
    if (src == dst) {
        same_handle(&p, T_out, res);
        return OSLAM_OK;
    }
    if (src->dev != dst->dev) return fail(OSLAM_E_INVALID, "the two pyramids live on different devices");
    rc = oslam_ego_check_pyramid_schedule(&p, src->n_levels < dst->n_levels ? src->n_levels : dst->n_levels);
    if (rc != OSLAM_OK) return rc;
    for (l = 0; l < p.n_levels; l++) {          /* level log2(stride) of both pyramids, every pixel of its source */
        pair[l].src = src->level[p.level[l].stride >> 1];
        pair[l].dst = dst->level[p.level[l].stride >> 1];
        pair[l].lattice = 1;
    }
    return oslam_ego_run(pair, T_init ? T_init : k_identity, &p, T_out, res);
}

int oslam_view_egomotion_correspondences(oslam_view *src, oslam_view *dst, const float T[16],
                                         const oslam_egomotion_params *ep, int32_t *pixel_out)
{
    oslam_egomotion_params p;
    int rc, built = 0;
    int32_t *d_pix = NULL;
    size_t n;
    void *stream = oslam_stream();
    if (!T || !pixel_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_call(src, dst, T, ep, &p);
    if (rc != OSLAM_OK) return rc;
    if (src->dev != dst->dev) return fail(OSLAM_E_INVALID, "the two views live on different devices");
    if (hipSetDevice(src->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    n = (size_t)src->k.w * (size_t)src->k.h;
    pthread_mutex_lock(&g_ego_mu);
    KCHK(oslam_dev_alloc((void **)&d_pix, sizeof(int32_t) * n));
    rc = oslam_track_view_maps(src, &built);
    if (rc == OSLAM_OK) rc = oslam_track_view_maps(dst, &built);
    if (rc != OSLAM_OK) goto done;
    KCHK(oslamk_ego_corr(&src->k, src->d_maps, &dst->k, dst->d_maps, T, p.max_corr_dist * p.max_corr_dist, p.min_normal_dot,
                         d_pix, stream));
    HIPCHK(hipMemcpyAsync(pixel_out, d_pix, sizeof(int32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    pthread_mutex_unlock(&g_ego_mu);
    if (d_pix) oslam_dev_free(d_pix);
    return rc;
}
