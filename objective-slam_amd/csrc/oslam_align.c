/*
 * oslam_align.c -- one registration after its votes (the pose tail, on the device or the host), the single-GPU
 * align entry points, and the multi-GPU exchange (exchange_peaks, oslam_align_multi).
 */
#include <pthread.h>

#include "oslam_comm.h"
#include "oslam_internal.h"
#include "oslam_pose.h"

/* ---- pose tail on the device (oslam_posegpu.hip) for large peak sets ---- */

/* 0: the tail may run on the device; the host-only variants keep the host path */
size_t oslam_pose_gpu_from(const oslam_model *m)
{
    if (m->params.cpu_clustering || m->params.use_averaged_clusters) return 0;
    return m->params.pose_gpu_min ? (size_t)m->params.pose_gpu_min : 4096;      /* tests force either tail through the parameter */
}

void oslam_drop_last(oslam_model *m)
{
    free(m->last_cells);
    free(m->last_poses);
    m->last_cells = NULL;
    m->last_poses = NULL;
    m->n_last = 0;
    m->last_on_device = 0;
}

/* frames and weights the device tail reads; built on first use */
int oslam_pose_tables(oslam_model *m, oslam_scene *s)
{
    int rc = OSLAM_OK;
    float *h = NULL, *d_T = NULL, *d_w = NULL, *d_S = NULL;
    if (!m->d_Tm16) {
        const size_t M = (size_t)m->c.n;
        h = (float *)malloc(sizeof(float) * 16 * M);
        if (!h) return fail(OSLAM_E_NOMEM, "host allocation failed");
        oslam_T_g_full(m->c.h_xyz, m->c.h_nrm, 0, 1, M, h);
        HIPCHK(hipMalloc((void **)&d_T, sizeof(float) * 16 * M));
        HIPCHK(hipMemcpy(d_T, h, sizeof(float) * 16 * M, hipMemcpyHostToDevice));
        HIPCHK(hipMalloc((void **)&d_w, sizeof(float) * M));
        HIPCHK(hipMemcpy(d_w, m->weights, sizeof(float) * M, hipMemcpyHostToDevice));
        m->d_Tm16 = d_T;                 /* the model owns them only when both are complete */
        m->d_weights = d_w;
        d_T = d_w = NULL;
        free(h);
        h = NULL;
    }
    if (!s->d_Ts16) {
        const size_t n_all = ((size_t)s->c.n + s->df - 1) / s->df;
        h = (float *)malloc(sizeof(float) * 16 * n_all);
        if (!h) return fail(OSLAM_E_NOMEM, "host allocation failed");
        oslam_T_g_full(s->c.h_xyz, s->c.h_nrm, 0, s->df, n_all, h);
        HIPCHK((hipError_t)oslam_dev_alloc((void **)&d_S, sizeof(float) * 16 * n_all));
        HIPCHK(hipMemcpy(d_S, h, sizeof(float) * 16 * n_all, hipMemcpyHostToDevice));
        s->d_Ts16 = d_S;
        d_S = NULL;
    }
done:
    free(h);
    if (d_T) (void)hipFree(d_T);
    if (d_w) (void)hipFree(d_w);
    oslam_dev_free(d_S);
    return rc;
}

/* the 64 rotations about x of the pose tail (host libm), made once per process */
static float g_rotx[128];
static pthread_once_t g_rotx_once = PTHREAD_ONCE_INIT;
static void rotx_init(void) { oslam_rotx_table(g_rotx); }
const float *oslam_rotx(void) { pthread_once(&g_rotx_once, rotx_init); return g_rotx; }

/* device buffers for the kept cells and their poses of up to n records */
int oslam_ensure_pose_buffers(oslam_model *m, size_t n)
{
    int rc = OSLAM_OK;
    if (m->pose_cap < n) {
        /* with head room: the number of peak records changes from frame to frame, and freeing device memory waits
         * for the device (0.2 ms a time on the 50-model depth stream) */
        const size_t cap = n + n / 2 > 8192 ? n + n / 2 : 8192;
        if (m->d_pose_cells) (void)hipFree(m->d_pose_cells);
        if (m->d_pose_T) (void)hipFree(m->d_pose_T);
        m->d_pose_cells = NULL;
        m->d_pose_T = NULL;
        m->pose_cap = 0;
        HIPCHK(hipMalloc((void **)&m->d_pose_cells, sizeof(oslamk_cell) * cap));
        HIPCHK(hipMalloc((void **)&m->d_pose_T, sizeof(float) * 16 * cap));
        m->pose_cap = cap;
    }
done:
    return rc;
}

/* Pose tail on the device over the n records in m->d_out.  Returns OSLAM_OK with *done = 1 when it
 * produced the pose; *done = 0 when fewer than two cells survive (the host path handles those). */
static int finish_on_device(oslam_model *m, oslam_scene *s, size_t n, uint32_t gmax, float T[16], oslam_stats *st,
                            const oslam_inst_req *req, oslamk_inst_out *sel, int *done)
{
    int rc = OSLAM_OK, k;
    uint32_t n_kept = 0, best = 0;
    const float min_votecount = m->params.vote_count_threshold * gmax;      /* model.cu:164 */
    *done = 0;
    rc = oslam_pose_tables(m, s);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_ensure_pose_buffers(m, n);
    if (rc != OSLAM_OK) return rc;
    k = oslamk_pose_stage(m->d_out, (uint32_t)n, min_votecount, m->d_Tm16, s->d_Ts16, s->df, m->d_weights, oslam_rotx(), m->d_dist,
                          m->params.use_l1_norm, m->d_pose_cells, m->d_pose_T, gmax, (uint32_t)m->c.n, (uint32_t)s->c.n, m->params.pose_two_sorts,
                          req ? &req->a : NULL, &n_kept, &best, T, sel, oslam_stream());
    if (k == -2) return fail(OSLAM_E_NOMEM, "host allocation failed");
    if (k != 0) return fail(OSLAM_E_DEVICE, hipGetErrorString((hipError_t)k));
    if (n_kept < 2) return OSLAM_OK;
    oslam_drop_last(m);
    m->n_last = n_kept;
    m->last_on_device = 1;
    if (st) { st->num_top = n_kept; st->max_count = gmax; }
    *done = 1;
    return rc;
}

/* the instance selection on the host over the candidates of the clustering stage */
static int select_on_host(const oslam_inst_req *req, const oslam_pose_cands *c, oslamk_inst_out *sel)
{
    uint32_t idx[OSLAMK_MAX_INSTANCES];
    size_t k, n = 0;
    const int rc = oslam_select_instances(c->T, c->score, c->n, req->a.c, req->extent, req->ip, idx, OSLAMK_MAX_INSTANCES, &n);
    sel->n = 0;
    if (rc != OSLAM_OK) return fail(rc, rc == OSLAM_E_NOMEM ? "host allocation failed" : "instance selection failed");
    for (k = 0; k < n; k++) {
        sel->idx[k] = c->index[idx[k]];
        sel->score[k] = c->score[idx[k]];
        memcpy(sel->T[k], c->T + 16 * (size_t)idx[k], 16 * sizeof(float));
    }
    sel->n = (uint32_t)n;
    return OSLAM_OK;
}

static int finish_cells(oslam_model *m, oslam_scene *s, oslam_cell *cells, size_t n, uint32_t gmax,
                        float T[16], oslam_stats *st, const oslam_inst_req *req, oslamk_inst_out *sel)
{
    int rc;
    oslam_pose_cands cands;
    memset(&cands, 0, sizeof cands);
    if (sel) sel->n = 0;
    n = oslam_filter_cells(cells, n, m->params.vote_count_threshold, gmax);
    oslam_sort_cells(cells, n);
    oslam_drop_last(m);
    m->last_cells = (oslam_cell *)malloc(sizeof(oslam_cell) * (n ? n : 1));
    m->last_poses = (float *)calloc(16 * (n ? n : 1), sizeof(float));
    m->n_last = 0;
    if (!m->last_cells || !m->last_poses) return fail(OSLAM_E_NOMEM, "host allocation failed");
    memcpy(m->last_cells, cells, sizeof(oslam_cell) * n);
    m->n_last = n;
    if (st) { st->num_top = n; st->max_count = gmax; }
    oslam_pose_set_cluster_hook(oslam_cluster_scores_on_device);
    if (req)
        rc = oslam_pose_stage_cands(cells, n, m->c.h_xyz, m->c.h_nrm, (size_t)m->c.n, s->c.h_xyz, s->c.h_nrm,
                                    (size_t)s->c.n, m->d_dist, m->params.cpu_clustering, m->params.use_l1_norm,
                                    m->params.use_averaged_clusters, m->weights, T, m->last_poses, &cands);
    else
        rc = oslam_pose_stage(cells, n, m->c.h_xyz, m->c.h_nrm, (size_t)m->c.n, s->c.h_xyz, s->c.h_nrm,
                              (size_t)s->c.n, m->d_dist, m->params.cpu_clustering, m->params.use_l1_norm,
                              m->params.use_averaged_clusters, m->weights, T, m->last_poses);
    oslam_pose_set_cluster_hook(NULL);
    if (rc == OSLAM_E_NO_VOTES) return fail(rc, "no scene pair matched the model");
    if (rc != OSLAM_OK) return fail(rc, "pose stage failed");
    if (req) {
        rc = select_on_host(req, &cands, sel);
        oslam_pose_cands_free(&cands);
    }
    return rc;
}

int oslam_align_prepare(oslam_model *m, oslam_scene *s)
{
    int rc;
    scratch_pool *pool;
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_pool_reserve_counts(pool, (size_t)(s->n_ref > 0 ? s->n_ref : 1));
    if (rc == OSLAM_OK && oslam_pose_gpu_from(m)) rc = oslam_pose_tables(m, s);
    oslam_pool_unlock(pool);
    return rc;
}

/* Everything after the votes of one registration on one device, over the n records in m->d_out: the pose tail on
 * the device when the set is large enough, else (or when fewer than two cells survive there) on the host.  try_device
 * 0: the caller ran the device tail already. */
int oslam_finish_after_votes(oslam_model *m, oslam_scene *s, size_t n, uint32_t gmax, int try_device, float T[16],
                             oslam_stats *stats, const oslam_inst_req *req, oslamk_inst_out *sel)
{
    int rc = OSLAM_OK;
    if (sel) sel->n = 0;
    if (try_device && oslam_pose_gpu_from(m) && n >= oslam_pose_gpu_from(m)) {
        int done = 0;
        rc = finish_on_device(m, s, n, gmax, T, stats, req, sel, &done);
        if (rc != OSLAM_OK || done) return rc;
    }
    if (n) HIPCHK(hipMemcpy(m->h_out, m->d_out, sizeof(oslam_cell) * n, hipMemcpyDeviceToHost));
    rc = finish_cells(m, s, m->h_out, n, gmax, T, stats, req, sel);
done:
    return rc;
}

int oslam_align(oslam_model *m, oslam_scene *s, float T[16], oslam_stats *stats)
{
    int rc;
    oslamk_counters cnt;
    size_t n = 0;
    oslam_stats local;
    scratch_pool *pool;
    double t0 = now_ms();
    if (!T) return fail(OSLAM_E_INVALID, "T is NULL");
    memset(T, 0, 16 * sizeof(float));
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc != OSLAM_OK) return rc;
    rc = oslam_vote_records(pool, m, s, &cnt, &n, stats, 0);
    if (rc == OSLAM_OK) rc = oslam_finish_after_votes(m, s, n, cnt.gmax, 1, T, stats, NULL, NULL);
    oslam_pool_unlock(pool);
    stats->ms_total = (float)(now_ms() - t0);
    return rc;
}

/* ---- multi-GPU, host-buffer form ------------------------------------------------------------- */
int oslam_align_local(oslam_model *m, oslam_scene *s, oslam_cell *cells_out, size_t cap,
                      size_t *n_out, uint32_t *local_max_out, oslam_stats *stats)
{
    int rc;
    oslamk_counters cnt;
    size_t n = 0;
    oslam_stats local;
    scratch_pool *pool;
    double t0 = now_ms();
    if (!n_out || !local_max_out || (!cells_out && cap)) return fail(OSLAM_E_INVALID, "NULL output");
    *n_out = 0;
    *local_max_out = 0;
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc != OSLAM_OK) return rc;
    m->n_local = 0;
    rc = oslam_vote_records(pool, m, s, &cnt, &n, stats, 1);
    oslam_pool_unlock(pool);
    if (rc != OSLAM_OK) return rc;
    /* peaks above the local threshold: a superset of what survives the global one; they stay with the
     * model (oslam_local_peaks hands them out again, filtered with the global maximum) */
    n = oslam_filter_cells(m->h_out, n, m->params.vote_count_threshold, cnt.gmax);
    m->n_local = n;
    m->local_max = cnt.gmax;
    *n_out = n;
    *local_max_out = cnt.gmax;
    stats->ms_total = (float)(now_ms() - t0);
    if (n > cap) {
        /* nothing is dropped silently: the caller learns the count and either passes a larger buffer to
         * oslam_local_peaks or exchanges the maxima first and asks for the (fewer) survivors */
        if (cap) {
            oslam_sort_cells(m->h_out, n);
            memcpy(cells_out, m->h_out, sizeof(oslam_cell) * cap);
        }
        return cap ? fail(OSLAM_E_LIMIT, "more local peaks than the buffer holds: *n_out is the number; fetch them with oslam_local_peaks")
                   : OSLAM_OK;
    }
    memcpy(cells_out, m->h_out, sizeof(oslam_cell) * n);
    return OSLAM_OK;
}

int oslam_local_peaks(oslam_model *m, uint32_t global_max, oslam_cell *cells_out, size_t cap, size_t *n_out)
{
    size_t i, n = 0;
    float bound;
    if (!m || !n_out || (!cells_out && cap)) return fail(OSLAM_E_INVALID, "NULL argument");
    if (global_max < m->local_max) return fail(OSLAM_E_INVALID, "the global maximum is below this rank's own");
    bound = m->params.vote_count_threshold * (float)global_max;      /* model.cu:164 */
    for (i = 0; i < m->n_local; i++)
        if ((float)m->h_out[i].count > bound) {
            if (n < cap) cells_out[n] = m->h_out[i];
            n++;
        }
    *n_out = n;
    if (n > cap) return fail(OSLAM_E_LIMIT, "more peaks above the global threshold than the buffer holds: *n_out is the number");
    return OSLAM_OK;
}

int oslam_align_finish(oslam_model *m, oslam_scene *s, const oslam_cell *cells, size_t n,
                       uint32_t global_max, float T[16], oslam_stats *stats)
{
    int rc;
    oslam_cell *tmp = NULL;
    oslam_stats local;
    scratch_pool *pool;
    if (!T || (!cells && n)) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(T, 0, 16 * sizeof(float));
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc != OSLAM_OK) return rc;
    if (oslam_pose_gpu_from(m) && n >= oslam_pose_gpu_from(m) && n <= m->out_cap) {
        /* the gathered union goes back to HBM; codes that do not name a reference point of this scene
         * and a point of this model are left to the host path, which reports them */
        size_t i;
        int ok = 1, done = 0;
        for (i = 0; i < n && ok; i++) {
            const uint32_t sr = (uint32_t)(cells[i].code >> 32), mr = ((uint32_t)cells[i].code) >> 6;
            ok = sr < (uint32_t)s->c.n && sr % s->df == 0 && mr < (uint32_t)m->c.n;
        }
        if (ok) {
            HIPCHK(hipMemcpy(m->d_out, cells, sizeof(oslam_cell) * n, hipMemcpyHostToDevice));
            rc = finish_on_device(m, s, n, global_max, T, stats, NULL, NULL, &done);
            if (rc != OSLAM_OK || done) goto done;
        }
    }
    tmp = (oslam_cell *)malloc(sizeof(oslam_cell) * (n ? n : 1));
    if (!tmp) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    memcpy(tmp, cells, sizeof(oslam_cell) * n);
    rc = finish_cells(m, s, tmp, n, global_max, T, stats, NULL, NULL);
done:
    free(tmp);
    oslam_pool_unlock(pool);
    return rc;
}

/* ---- multi-GPU: one call per rank does everything (ppf.h:9-15 is one call too) -----------------
 * The exchange stays in HBM: all-reduce(MAX) of the vote maxima, the local records filtered with the
 * global threshold where they lie, an all-gather of the survivor counts, an all-gather with exact
 * sizes of the survivors straight into the union buffer, and the pose tail on the union -- on the
 * device when it is large.  The collectives go through the communicator's table of operations
 * (oslam_comm.h): RCCL over xGMI, or the in-process loopback that lets the same function run with
 * N emulated ranks on one device.  Latency-bound: a few KiB to a few hundred KiB per rank.
 *
 * Failure is collective: whatever goes wrong on ONE rank between two collectives (no memory for the
 * union, more peaks than the buffers can hold, a failed kernel) travels as an error word beside the
 * payload of the next collective, so that every rank leaves at the same point -- none is left
 * waiting in a collective its peer will never enter.  A collective that fails itself aborts the
 * communicator (ncclCommAbort) and marks it broken. */

static int ensure_union(oslam_model *m, size_t n)
{
    if (m->union_cap >= n) return OSLAM_OK;
    if (m->d_union) { (void)hipFree(m->d_union); m->d_union = NULL; m->union_cap = 0; }
    if (hipMalloc((void **)&m->d_union, sizeof(oslamk_cell) * (n + n / 4)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OSLAM_E_NOMEM, "no device memory for the accumulator peaks");
    }
    m->union_cap = n + n / 4;
    return OSLAM_OK;
}

/* this rank's n_local records in m->d_out (local maximum lmax, rc_local = what the vote stage returned) ->
 * the union of every rank's records above the global threshold in m->d_out, *total of them */
static int exchange_peaks(oslam_model *m, oslam_comm *c, size_t n_local, uint32_t lmax, int rc_local,
                          uint32_t *gmax_out, size_t *total_out)
{
    int rc = OSLAM_OK, own = OSLAM_OK, r, any = 0, grow_any = 0, together = 0;   /* together: every rank leaves at this point */
    uint32_t n_mine = 0, gmax;
    size_t total = 0, bytes[64];
    size_t *by = bytes;
    hipStream_t st = (hipStream_t)oslam_stream();
    uint32_t *h = c->h_small, *d = c->d_small;
    *gmax_out = 0;
    *total_out = 0;
    if (c->world > 64) {
        by = (size_t *)malloc(sizeof(size_t) * (size_t)c->world);
        if (!by) { by = bytes; rc_local = rc_local != OSLAM_OK ? rc_local : fail(OSLAM_E_NOMEM, "host allocation failed"); }
    }
    /* 1. the threshold is global (model.cu:164-170): maximum over ranks, with the error word */
    h[0] = lmax;
    h[1] = (rc_local != OSLAM_OK || c->inject_stage == OSLAM_STAGE_VOTE) ? 1u : 0u;
    HIPCHK(hipMemcpyAsync(d, h, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    rc = oslam_comm_all_reduce_max(c, d, 2, oslam_stream());
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipMemcpyAsync(h, d, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[1]) {
        together = 1;
        rc = oslam_comm_error(c, rc_local, OSLAM_STAGE_VOTE);
        goto done;
    }
    gmax = h[0];
    /* 2. survivors of this rank, compacted into the second record buffer */
    {
        scratch_pool *pool;                                    /* the selection shares the device's work space */
        int k = 1;
        if (oslam_pool_enter(m->dev, &pool) == OSLAM_OK && ensure_union(m, n_local > 0 ? n_local : 1) == OSLAM_OK)
            k = n_local ? oslamk_select_cells(m->d_out, (uint32_t)n_local, m->params.vote_count_threshold * (float)gmax,
                                              m->d_union, &n_mine, oslam_stream()) : 0;
        oslam_pool_unlock(pool);
        if (k != 0) own = fail(OSLAM_E_NOMEM, "no device memory for this rank's survivors");
    }
    h[0] = n_mine;
    h[1] = own != OSLAM_OK || c->inject_stage == OSLAM_STAGE_SELECT;
    h[2] = m->out_cap;
    HIPCHK(hipMemcpyAsync(d, h, 3 * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    rc = oslam_comm_all_gather(c, d, d + 4, 3, oslam_stream());
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipMemcpyAsync(h + 4, d + 4, 3 * sizeof(uint32_t) * (size_t)c->world, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (r = 0; r < c->world; r++) {
        total += h[4 + 3 * r];
        any |= h[4 + 3 * r + 1] != 0;
        by[r] = (size_t)h[4 + 3 * r] * sizeof(oslamk_cell);
    }
    if (any) {
        together = 1;
        rc = oslam_comm_error(c, own, OSLAM_STAGE_SELECT);
        goto done;
    }
    if (total > ((size_t)1 << 28)) {                       /* the same on every rank */
        together = 1;
        rc = fail(OSLAM_E_LIMIT, "more than 2^28 accumulator peaks above the threshold");
        goto done;
    }
    /* 3. room for the union, rank after rank, in m->d_out (this rank's survivors are safe in d_union).  Buffers
     * differ per rank; whether ANY rank has to grow is known to all from the gathered capacities, and only
     * then does everybody meet once more to learn whether the growing worked */
    for (r = 0; r < c->world; r++) grow_any |= total > h[4 + 3 * r + 2];
    if (grow_any) {
        if (total > m->out_cap && oslam_grow_records(m, total + total / 8 + 1024) != OSLAM_OK)
            own = fail(OSLAM_E_NOMEM, "no memory for the union of the accumulator peaks");
        h[0] = own != OSLAM_OK || c->inject_stage == OSLAM_STAGE_GROW;
        HIPCHK(hipMemcpyAsync(d, h, sizeof(uint32_t), hipMemcpyHostToDevice, st));
        rc = oslam_comm_all_reduce_max(c, d, 1, oslam_stream());
        if (rc != OSLAM_OK) goto done;
        HIPCHK(hipMemcpyAsync(h, d, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h[0]) {
            together = 1;
            rc = oslam_comm_error(c, own, OSLAM_STAGE_GROW);
            goto done;
        }
    }
    /* 4. the union */
    if (total) {
        rc = oslam_comm_all_gather_v(c, m->d_union, m->d_out, by, oslam_stream());
        if (rc != OSLAM_OK) goto done;
        HIPCHK(hipStreamSynchronize(st));
    }
    *gmax_out = gmax;
    *total_out = total;
done:
    if (rc != OSLAM_OK && !together)
        /* a HIP call of this rank failed between collectives: the peers cannot be told through a device buffer any
         * more; give the communicator up so that nothing of it is used again */
        (void)oslam_comm_abort(c);
    c->inject_stage = OSLAM_STAGE_NONE;
    if (by != bytes) free(by);
    return rc;
}

int oslam_align_multi(oslam_model *m, oslam_scene *s, oslam_comm *c, float T[16], oslam_stats *stats)
{
    int rc, vrc;
    oslamk_counters cnt;
    size_t n = 0, total = 0;
    uint32_t gmax = 0;
    oslam_stats local;
    scratch_pool *pool = NULL;
    double t0 = now_ms();
    if (!T || !c) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(T, 0, 16 * sizeof(float));
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (c->dev != m->dev) return fail(OSLAM_E_INVALID, "communicator and model live on different devices");
    if (s->world != c->world || s->rank != c->rank) return fail(OSLAM_E_INVALID, "the scene's shard differs from the communicator's rank");
    if (c->broken) return fail(OSLAM_E_DEVICE, "the communicator was aborted after a failed collective: make a new one");
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    /* this rank's votes; the records stay in m->d_out.  The device's pool is held for the votes and for the pose
     * tail, not across the collectives: emulated ranks share a device (and a pool).  A failure here travels to the
     * peers with the first collective */
    memset(&cnt, 0, sizeof cnt);
    vrc = oslam_pool_enter(m->dev, &pool);
    if (vrc == OSLAM_OK) vrc = oslam_vote_records(pool, m, s, &cnt, &n, stats, 0);
    oslam_pool_unlock(pool);
    if (vrc != OSLAM_OK) { n = 0; cnt.gmax = 0; }
    rc = exchange_peaks(m, c, n, cnt.gmax, vrc, &gmax, &total);
    if (rc != OSLAM_OK) goto done;
    stats->num_emitted = (uint32_t)total;
    /* every rank finishes on the same union: same pose everywhere, no second exchange */
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc == OSLAM_OK) rc = oslam_finish_after_votes(m, s, total, gmax, 1, T, stats, NULL, NULL);
    oslam_pool_unlock(pool);
done:
    stats->ms_total = (float)(now_ms() - t0);
    return rc;
}
