/*
 * oslam_refine.c -- pose refinement and presence score (include/oslam.h at oslam_refine): the host side of the
 * kernels in oslam_refine.hip.  The host checks the arguments, finds or builds the scene grid, uploads one
 * descriptor per member and enqueues score -> (correspond, solve) x iterations -> score; it reads an "all members
 * done" word after every 4th iteration and the results once at the end.  The pose lives in double on the device
 * between iterations; the host only rounds the final one.
 */
#include <math.h>
#include <pthread.h>

#include "oslam_internal.h"

#define GRID_SLOTS 4
#define CHECK_EVERY 4                 /* iterations between two reads of the "all done" word */

/* one cached grid of a scene (oslam_scene.grids[GRID_SLOTS]) */
struct oslam_scene_grid {
    float radius;                     /* radius it was built for; 0 = empty slot */
    double edge;
    uint64_t used;                    /* call counter of its last use (the least recently used slot is rebuilt) */
    void *block;                      /* one device block holding every array of g */
    oslamk_grid g;
};

/* one refinement call at a time per process: the grid caches of the scenes are shared state */
static pthread_mutex_t g_refine_mu = PTHREAD_MUTEX_INITIALIZER;
static uint64_t g_calls;

int oslam_refine_params_default(oslam_refine_params *p)
{
    if (!p) return oslam_fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->max_iterations = 30;
    p->max_corr_dist = 2.0f;
    p->min_normal_dot = 0.8f;
    p->inlier_dist = 0.5f;
    p->min_fitness = 0.3f;
    p->stop_rot = 1e-5f;
    p->stop_trans = 1e-4f;
    return OSLAM_OK;
}

int oslam_refine_check_params(const oslam_refine_params *rp, oslam_refine_params *out)
{
    if (rp) *out = *rp;
    else oslam_refine_params_default(out);
    if (!isfinite(out->max_corr_dist) || !isfinite(out->inlier_dist) || !isfinite(out->min_normal_dot) ||
        !isfinite(out->min_fitness) || !isfinite(out->stop_rot) || !isfinite(out->stop_trans))
        return oslam_fail(OSLAM_E_INVALID, "refine parameters must be finite");
    if (!(out->max_corr_dist > 0.0f) || !(out->inlier_dist > 0.0f))
        return oslam_fail(OSLAM_E_INVALID, "max_corr_dist and inlier_dist must be > 0");
    if (out->inlier_dist > out->max_corr_dist) return oslam_fail(OSLAM_E_INVALID, "inlier_dist larger than max_corr_dist");
    if (out->max_iterations > 1000) return oslam_fail(OSLAM_E_INVALID, "max_iterations above 1000");
    if (out->stop_rot < 0.0f || out->stop_trans < 0.0f) return oslam_fail(OSLAM_E_INVALID, "negative stop criterion");
    return OSLAM_OK;
}

/* finite, rotation orthonormal to 1e-3 with determinant > 0, last row 0 0 0 1 */
int oslam_refine_check_rigid(const float T[16])
{
    int a, b, k;
    double det;
    for (k = 0; k < 16; k++)
        if (!isfinite(T[k])) return oslam_fail(OSLAM_E_INVALID, "T_in is not finite");
    if (T[12] != 0.0f || T[13] != 0.0f || T[14] != 0.0f || T[15] != 1.0f)
        return oslam_fail(OSLAM_E_INVALID, "T_in: last row is not 0 0 0 1");
    for (a = 0; a < 3; a++)
        for (b = 0; b < 3; b++) {
            double dot = 0.0;
            for (k = 0; k < 3; k++) dot += (double)T[4 * k + a] * (double)T[4 * k + b];
            if (fabs(dot - (a == b ? 1.0 : 0.0)) > 1e-3) return oslam_fail(OSLAM_E_INVALID, "T_in: rotation not orthonormal");
        }
    det = (double)T[0] * ((double)T[5] * T[10] - (double)T[6] * T[9]) - (double)T[1] * ((double)T[4] * T[10] - (double)T[6] * T[8]) +
          (double)T[2] * ((double)T[4] * T[9] - (double)T[5] * T[8]);
    if (!(det > 0.0)) return oslam_fail(OSLAM_E_INVALID, "T_in: rotation is a reflection");
    return OSLAM_OK;
}

static int check_model(const oslam_model *m, const oslam_scene *s)
{
    if (m->unusable) return oslam_fail(OSLAM_E_INVALID, "this model lost its key tables with its database: it can only be destroyed");
    if (m->dev != s->dev) return oslam_fail(OSLAM_E_INVALID, "model and scene live on different devices");
    return OSLAM_OK;
}

void oslam_refine_release_grids(oslam_scene *s)
{
    int k;
    if (!s || !s->grids) return;
    /* every refinement call ends with a synchronisation of its stream: no kernel still reads these blocks */
    for (k = 0; k < GRID_SLOTS; k++)
        if (s->grids[k].block) oslam_dev_free(s->grids[k].block);
    free(s->grids);
    s->grids = NULL;
}

/* A grid of the scene whose cells serve `radius`: a cached one with an edge in [radius, 2 radius] (the smallest such
 * edge), else the one that was built for exactly this radius (a grid enlarged to stay within OSLAMK_GRID_MAX_CELLS has an
 * edge above 2 radius: no other grid of this radius would be finer), else a new one (enqueued on the stream; *built = 1). */
static int scene_grid(oslam_scene *s, float radius, oslamk_grid *out, int *built)
{
    int rc = OSLAM_OK, k, slot = -1, a;
    struct oslam_scene_grid *e;
    double lo[3], hi[3], edge, cells;
    size_t n = (size_t)s->c.n, n_items, nb, off;
    char *base;
    *built = 0;
    if (!s->grids) {
        s->grids = (struct oslam_scene_grid *)calloc(GRID_SLOTS, sizeof *s->grids);
        if (!s->grids) return oslam_fail(OSLAM_E_NOMEM, "host allocation failed");
    }
    for (k = 0; k < GRID_SLOTS; k++) {
        e = &s->grids[k];
        if (e->radius > 0.0f && e->edge >= (double)radius && e->edge <= 2.0 * (double)radius &&
            (slot < 0 || e->edge < s->grids[slot].edge))
            slot = k;
    }
    for (k = 0; k < GRID_SLOTS && slot < 0; k++)
        if (s->grids[k].radius == radius) slot = k;
    if (slot >= 0) {
        s->grids[slot].used = g_calls;
        *out = s->grids[slot].g;
        return OSLAM_OK;
    }
    for (k = 0; k < GRID_SLOTS && slot < 0; k++)          /* an empty slot, or the least recently used one */
        if (s->grids[k].radius == 0.0f) slot = k;
    if (slot < 0)
        for (slot = 0, k = 1; k < GRID_SLOTS; k++)
            if (s->grids[k].used < s->grids[slot].used) slot = k;
    e = &s->grids[slot];
    if (e->block) oslam_dev_free(e->block);     /* the last call that used it synchronised its stream */
    memset(e, 0, sizeof *e);

    for (a = 0; a < 3; a++) lo[a] = hi[a] = s->c.h_xyz[a];
    for (k = 1; k < (int)n; k++)
        for (a = 0; a < 3; a++) {
            const double x = s->c.h_xyz[3 * (size_t)k + a];
            if (x < lo[a]) lo[a] = x;
            if (x > hi[a]) hi[a] = x;
        }
    /* an edge a little above the radius: a point within the radius is at most one cell away in every axis */
    edge = (double)radius * (1.0 + 1e-4);
    for (;;) {
        cells = 1.0;
        for (a = 0; a < 3; a++) cells *= floor((hi[a] - lo[a]) / edge) + 1.0;
        if (cells <= (double)OSLAMK_GRID_MAX_CELLS) break;
        edge *= cbrt(cells / (double)OSLAMK_GRID_MAX_CELLS) * 1.01;
    }
    e->g.inv_edge = 1.0 / edge;
    for (a = 0; a < 3; a++) {
        e->g.lo[a] = lo[a];
        e->g.dim[a] = (int)floor((hi[a] - lo[a]) * e->g.inv_edge) + 1;
    }
    /* the device computes a point's cell as floor((x - lo) * inv_edge): the last cell must hold the largest point */
    e->g.n_cells = (uint32_t)e->g.dim[0] * (uint32_t)e->g.dim[1] * (uint32_t)e->g.dim[2];
    if (e->g.n_cells > OSLAMK_GRID_MAX_CELLS) { rc = oslam_fail(OSLAM_E_LIMIT, "scene grid too large"); goto done; }
    e->g.n = (int)n;
    n_items = (size_t)e->g.n_cells + 1;
    nb = (n_items + OSLAMK_SCAN_ITEMS - 1) / OSLAMK_SCAN_ITEMS;
    off = 2 * align256(4 * n_items) + align256(4 * nb) + 2 * align256(4 * n) + align256(32 * n);
    KCHK(oslam_dev_alloc(&e->block, off));
    base = (char *)e->block;
    e->g.start = (uint32_t *)base;   base += align256(4 * n_items);
    e->g.local = (uint32_t *)base;   base += align256(4 * n_items);
    e->g.bsum = (uint32_t *)base;    base += align256(4 * nb);
    e->g.cell_of = (uint32_t *)base; base += align256(4 * n);
    e->g.rank = (uint32_t *)base;    base += align256(4 * n);
    e->g.pts = (float *)base;
    KCHK(oslamk_refine_grid_build(&e->g, s->c.k, oslam_stream()));
    e->edge = edge;
    e->radius = radius;
    e->used = g_calls;
    *built = 1;
    *out = e->g;
done:
    if (rc != OSLAM_OK) {
        (void)hipStreamSynchronize((hipStream_t)oslam_stream());
        if (e->block) oslam_dev_free(e->block);
        memset(e, 0, sizeof *e);
    }
    return rc;
}

/* the pose bookkeeping of a descriptor: the model's centroid, the pose in double and in float, the centroid under it */
static void set_pose(oslamk_refine_member *d, const oslam_model *m, const float T[16])
{
    double c[3];
    int a;
    memcpy(d->cm, m->cm, sizeof d->cm);
    for (a = 0; a < 12; a++) {
        d->T[a] = (double)T[a];
        d->Tf[a] = T[a];
    }
    oslam_rigid_apply(d->T, d->cm, c);
    for (a = 0; a < 3; a++) d->c[a] = (float)c[a];
}

/* The members ms[0 .. n) (T_in[j*16], all-zero = skipped) against scene s: the whole stage. */
int oslam_refine_members(oslam_model *const *ms, size_t n, oslam_scene *s, const float *T_in, const oslam_refine_params *p,
                         float *T_out, oslam_refine_result *res)
{
    int rc = OSLAM_OK, built = 0;
    const double t0 = now_ms();
    size_t j, n_act = 0, b, max_blocks = 1, off_slab, off_in, off_out, off_done, bytes;
    size_t *act = NULL;
    float rmax = 0.0f;
    oslamk_grid g;
    oslamk_refine_member *h = NULL;
    float *h_in = NULL, *h_out = NULL;
    char *dev = NULL;
    uint32_t launches = 0, it, n_done = 0;
    void *stream = oslam_stream();

    memset(T_out, 0, sizeof(float) * 16 * n);
    if (res) memset(res, 0, sizeof *res * n);
    act = (size_t *)malloc(sizeof *act * (n ? n : 1));
    if (!act) return oslam_fail(OSLAM_E_NOMEM, "host allocation failed");
    for (j = 0; j < n; j++)
        if (!oslam_is_zero_pose(T_in + 16 * j)) {
            const float r = p->max_corr_dist * ms[j]->d_dist;
            const size_t nb = ((size_t)ms[j]->c.n + OSLAMK_REFINE_THREADS - 1) / OSLAMK_REFINE_THREADS;
            act[n_act++] = j;
            if (r > rmax) rmax = r;
            if (nb > max_blocks) max_blocks = nb;
        }
    if (n_act == 0) { free(act); return OSLAM_OK; }
    if (n_act > 65535) { free(act); return oslam_fail(OSLAM_E_LIMIT, "more than 65535 members in one refinement"); }
    if (hipSetDevice(s->dev) != hipSuccess) { free(act); return oslam_fail(OSLAM_E_DEVICE, "hipSetDevice failed"); }

    /* device block: descriptors | all-done word | step slab | score slabs (input pose, output pose) */
    off_done = align256(sizeof *h * n_act);
    off_slab = off_done + 256;
    off_in = off_slab + align256(sizeof(float) * OSLAMK_REFINE_STRIDE * max_blocks * n_act);
    off_out = off_in + align256(sizeof(float) * 2 * max_blocks * n_act);
    bytes = off_out + align256(sizeof(float) * 2 * max_blocks * n_act);
    h = (oslamk_refine_member *)calloc(1, off_slab);
    h_in = (float *)malloc(sizeof(float) * 2 * max_blocks * n_act);
    h_out = (float *)malloc(sizeof(float) * 2 * max_blocks * n_act);
    if (!h || !h_in || !h_out) { free(act); free(h); free(h_in); free(h_out); return oslam_fail(OSLAM_E_NOMEM, "host allocation failed"); }
    for (b = 0; b < n_act; b++) {
        const oslam_model *m = ms[act[b]];
        oslamk_refine_member *d = &h[b];
        const float rc_ = p->max_corr_dist * m->d_dist, rs = p->inlier_dist * m->d_dist;
        set_pose(d, m, T_in + 16 * act[b]);
        d->m = m->c.k;
        d->r2_corr = rc_ * rc_;
        d->r2_score = rs * rs;
        d->min_dot = p->min_normal_dot;
        d->stop_rot = p->stop_rot;
        d->stop_trans = p->stop_trans * m->d_dist;
        d->max_iter = p->max_iterations;
        d->n_blocks = (uint32_t)(((size_t)m->c.n + OSLAMK_REFINE_THREADS - 1) / OSLAMK_REFINE_THREADS);
        d->active = 1;
        d->done = p->max_iterations == 0;
    }
    if (p->max_iterations == 0) *(uint32_t *)((char *)h + off_done) = (uint32_t)n_act;

    pthread_mutex_lock(&g_refine_mu);
    g_calls++;
    KCHK(oslam_dev_alloc((void **)&dev, bytes));
    /* the descriptors (and the zeroed all-done word behind them) first: the copy does not wait for the grid */
    HIPCHK(hipMemcpyAsync(dev, h, off_slab, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = scene_grid(s, rmax, &g, &built);
    if (rc != OSLAM_OK) goto done;
    if (built) launches += 5;
    KCHK(oslamk_refine_corr(OSLAMK_REFINE_SCORE, &g, (oslamk_refine_member *)dev, (uint32_t)n_act, (uint32_t)max_blocks,
                            (float *)(dev + off_in), NULL, stream));
    launches++;
    for (it = 0; it < p->max_iterations; it++) {
        KCHK(oslamk_refine_corr(OSLAMK_REFINE_STEP, &g, (oslamk_refine_member *)dev, (uint32_t)n_act, (uint32_t)max_blocks,
                                (float *)(dev + off_slab), NULL, stream));
        KCHK(oslamk_refine_solve((oslamk_refine_member *)dev, (uint32_t)n_act, (uint32_t)max_blocks, (const float *)(dev + off_slab),
                                 (uint32_t *)(dev + off_done), stream));
        launches += 2;
        if ((it + 1) % CHECK_EVERY == 0 && it + 1 < p->max_iterations) {
            HIPCHK(hipMemcpyAsync(&n_done, dev + off_done, sizeof n_done, hipMemcpyDeviceToHost, (hipStream_t)stream));
            HIPCHK(hipStreamSynchronize((hipStream_t)stream));
            if (n_done >= n_act) break;
        }
    }
    KCHK(oslamk_refine_corr(OSLAMK_REFINE_SCORE, &g, (oslamk_refine_member *)dev, (uint32_t)n_act, (uint32_t)max_blocks,
                            (float *)(dev + off_out), NULL, stream));
    launches++;
    HIPCHK(hipMemcpyAsync(h, dev, sizeof *h * n_act, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(h_in, dev + off_in, sizeof(float) * 2 * max_blocks * n_act, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(h_out, dev + off_out, sizeof(float) * 2 * max_blocks * n_act, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));

    for (b = 0; b < n_act; b++) {
        const oslamk_refine_member *d = &h[b];
        const size_t jj = act[b];
        const double M = (double)ms[jj]->c.n;
        double in_n = 0.0, out_n = 0.0, out_d2 = 0.0;
        size_t w;
        int a;
        float *T = T_out + 16 * jj;
        for (w = 0; w < d->n_blocks; w++) {              /* workgroup order, in double: reproducible */
            in_n += (double)h_in[(b * max_blocks + w) * 2];
            out_n += (double)h_out[(b * max_blocks + w) * 2];
            out_d2 += (double)h_out[(b * max_blocks + w) * 2 + 1];
        }
        for (a = 0; a < 12; a++) T[a] = d->Tf[a];
        T[15] = 1.0f;
        if (res) {
            oslam_refine_result *r = &res[jj];
            r->fitness_in = (float)(in_n / M);
            r->fitness = (float)(out_n / M);
            r->rmse = out_n > 0.0 ? (float)sqrt(out_d2 / out_n) : 0.0f;
            r->inliers = (uint32_t)out_n;
            r->correspondences = (uint32_t)d->n_corr;
            r->iterations = (uint32_t)d->iterations;
            r->converged = d->converged;
            r->found = r->fitness >= p->min_fitness;
        }
    }
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);    /* nothing may still use the block we give back */
    if (dev) oslam_dev_free(dev);
    pthread_mutex_unlock(&g_refine_mu);
    if (res && rc == OSLAM_OK) {
        const float ms_total = (float)(now_ms() - t0);
        for (j = 0; j < n; j++) {
            res[j].launches = launches;
            res[j].ms_total = ms_total;
        }
    }
    free(act);
    free(h);
    free(h_in);
    free(h_out);
    return rc;
}

int oslam_refine(oslam_model *m, oslam_scene *s, const float T_in[16], const oslam_refine_params *rp, float T_out[16],
                 oslam_refine_result *res)
{
    oslam_refine_params p;
    int rc;
    if (!m || !s || !T_in || !T_out) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_refine_check_params(rp, &p);
    if (rc == OSLAM_OK) rc = oslam_refine_check_rigid(T_in);
    if (rc == OSLAM_OK) rc = check_model(m, s);
    if (rc != OSLAM_OK) return rc;
    return oslam_refine_members(&m, 1, s, T_in, &p, T_out, res);
}

int oslam_db_refine(oslam_db *db, oslam_scene *s, const float *T_in, const oslam_refine_params *rp, float *T_out,
                    oslam_refine_result *res)
{
    oslam_refine_params p;
    size_t j;
    int rc;
    if (!db || !s || !T_in || !T_out) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_refine_check_params(rp, &p);
    if (rc == OSLAM_OK) rc = oslam_check_poses(NULL, T_in, db->n, 0);
    for (j = 0; rc == OSLAM_OK && j < db->n; j++)     /* the handles: against a scene, not a view */
        if (!oslam_is_zero_pose(T_in + 16 * j)) rc = check_model(db->models[j], s);
    if (rc != OSLAM_OK) return rc;
    return oslam_refine_members(db->models, db->n, s, T_in, &p, T_out, res);
}

int oslam_refine_correspondences(oslam_model *m, oslam_scene *s, const float T[16], float radius, float min_normal_dot,
                                 int32_t *idx_out)
{
    int rc, built = 0;
    oslamk_refine_member h;
    oslamk_grid g;
    char *dev = NULL;
    void *stream = oslam_stream();
    size_t M, off_idx;
    if (!m || !s || !T || !idx_out) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    if (!(radius > 0.0f) || !isfinite(radius) || !isfinite(min_normal_dot)) return oslam_fail(OSLAM_E_INVALID, "bad radius or normal gate");
    rc = oslam_refine_check_rigid(T);
    if (rc == OSLAM_OK) rc = check_model(m, s);
    if (rc != OSLAM_OK) return rc;
    if (hipSetDevice(s->dev) != hipSuccess) return oslam_fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    M = (size_t)m->c.n;
    memset(&h, 0, sizeof h);
    set_pose(&h, m, T);
    h.m = m->c.k;
    h.r2_corr = radius * radius;
    h.min_dot = min_normal_dot;
    h.n_blocks = (uint32_t)((M + OSLAMK_REFINE_THREADS - 1) / OSLAMK_REFINE_THREADS);
    h.active = 1;
    off_idx = align256(sizeof h);
    pthread_mutex_lock(&g_refine_mu);
    g_calls++;
    KCHK(oslam_dev_alloc((void **)&dev, off_idx + sizeof(int32_t) * M));
    HIPCHK(hipMemcpyAsync(dev, &h, sizeof h, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = scene_grid(s, radius, &g, &built);
    if (rc != OSLAM_OK) goto done;
    KCHK(oslamk_refine_corr(OSLAMK_REFINE_TAP, &g, (oslamk_refine_member *)dev, 1, h.n_blocks, NULL,
                            (int32_t *)(dev + off_idx), stream));
    HIPCHK(hipMemcpyAsync(idx_out, dev + off_idx, sizeof(int32_t) * M, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    if (dev) oslam_dev_free(dev);
    pthread_mutex_unlock(&g_refine_mu);
    return rc;
}
