/*
 * oslam_db.c -- the model database: groups of models that share one union table, their registration against
 * one scene, the database split by model over a communicator, and oslam_ppf_registration.
 */

#include "oslam_comm.h"
#include "oslam_internal.h"

/* ------------------------------------------------------------------------
 * Model database (src/cuda/ppf.cu:57-100: the reference loops scenes x models and rebuilds
 * both every time).  Models that share d_dist (and device and vote mode) form a group with ONE union table:
 * the scene pass -- count, pair keys, probe, hit sort -- then runs once per group and frame instead of once
 * per model, every model votes from the same hit lists with its own buckets (table.uinfo under the group's
 * slots), and nothing waits on the host between the models of a group.  Models with a d_dist of their own
 * are groups of one and take the single-model path.
 * ---------------------------------------------------------------------- */
static int same_group(const oslam_model *a, const oslam_model *b)
{
    return a->dev == b->dev && a->d_dist == b->d_dist && a->params.vote_mode == b->params.vote_mode;
}

static void db_destroy(oslam_db *db, int give_back)
{
    int g, k;
    uint32_t *d_small = NULL;
    if (!db) return;
    (void)hipSetDevice(db->dev);
    if (give_back) (void)hipMalloc((void **)&d_small, 2 * sizeof(uint32_t));
    for (g = 0; g < db->n_groups; g++) {
        db_group *gr = &db->groups[g];
        if (gr->n > 1) {
            /* the members get a union table of their own back; one that cannot (or is not asked to) is left
             * without key tables and refuses every call but oslam_model_destroy */
            for (k = 0; k < gr->n; k++) {
                oslam_model *m = db->models[gr->members[k]];
                int ok = 0;
                if (!m->shared_union) continue;         /* never switched to the group's tables (a failed oslam_db_create) */
                if (d_small && oslam_build_union(m, (uint32_t)(m->num_model_keys ? m->num_model_keys - 1 : 0), d_small, d_small + 1) == OSLAM_OK)
                    ok = oslam_build_uinfo(m) == OSLAM_OK;
                if (!ok) {
                    if (m->shared_union) {               /* still pointing at the group's tables, which are freed below */
                        m->table.ukeys = NULL;
                        m->table.reach = NULL;
                        m->table.kmap = NULL;
                        m->table.uids = NULL;
                        m->shared_union = 0;
                    }
                    m->unusable = 1;
                }
            }
            (void)hipStreamSynchronize((hipStream_t)oslam_stream());
            if (gr->ukeys) (void)hipFree(gr->ukeys);
            if (gr->reach) (void)hipFree(gr->reach);
            if (gr->kmap) (void)hipFree(gr->kmap);
            if (gr->uids) (void)hipFree(gr->uids);
        }
        free(gr->members);
    }
    if (d_small) (void)hipFree(d_small);
    free(db->groups);
    free(db->models);
    free(db);
}

void oslam_db_destroy(oslam_db *db) { db_destroy(db, 1); }

void oslam_db_destroy_with_models(oslam_db *db) { db_destroy(db, 0); }

int oslam_db_create(oslam_model *const *models, size_t n, oslam_db **out)
{
    int rc = OSLAM_OK, g, k;
    size_t j;
    oslam_db *db;
    oslamk_table *parts = NULL;
    uint32_t *d_small = NULL, h_small[2];
    if (!out) return fail(OSLAM_E_INVALID, "out is NULL");
    *out = NULL;
    if (!models || n == 0) return fail(OSLAM_E_INVALID, "empty database");
    for (j = 0; j < n; j++) {
        if (!models[j]) return fail(OSLAM_E_INVALID, "NULL model");
        if (models[j]->shared_union) return fail(OSLAM_E_INVALID, "a model can be in one database at a time");
        if (models[j]->unusable) return fail(OSLAM_E_INVALID, "a model without key tables cannot join a database");
        if (models[j]->dev != models[0]->dev) return fail(OSLAM_E_INVALID, "the models of a database live on one device");
        for (k = 0; k < (int)j; k++)
            if (models[k] == models[j]) return fail(OSLAM_E_INVALID, "the same model handle twice in one database");
    }
    db = (oslam_db *)calloc(1, sizeof *db);
    if (!db) return fail(OSLAM_E_NOMEM, "host allocation failed");
    db->dev = models[0]->dev;
    db->n = n;
    db->models = (oslam_model **)malloc(sizeof *db->models * n);
    db->groups = (db_group *)calloc(n, sizeof *db->groups);
    if (!db->models || !db->groups) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    memcpy(db->models, models, sizeof *db->models * n);
    if (hipSetDevice(db->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    for (j = 0; j < n; j++) {
        for (g = 0; g < db->n_groups; g++)
            if (same_group(models[db->groups[g].members[0]], models[j])) break;
        if (g == db->n_groups) {
            db->groups[g].members = (size_t *)malloc(sizeof(size_t) * n);
            if (!db->groups[g].members) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
            db->n_groups++;
        }
        db->groups[g].members[db->groups[g].n++] = j;
    }
    HIPCHK(hipMalloc((void **)&d_small, 2 * sizeof(uint32_t)));
    parts = (oslamk_table *)malloc(sizeof *parts * n);
    if (!parts) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    for (g = 0; g < db->n_groups; g++) {
        db_group *gr = &db->groups[g];
        oslamk_table t;
        uint64_t distinct = 0;
        uint32_t lg = 16;
        if (gr->n < 2) continue;
        for (k = 0; k < gr->n; k++) distinct += models[gr->members[k]]->num_model_keys;
        while (((uint64_t)1 << lg) < 4u * distinct && lg < OSLAMK_RUN_SHIFT) lg++;
        if (((uint64_t)1 << lg) < 2u * distinct) { rc = fail(OSLAM_E_LIMIT, "more distinct pair keys in the group than a union table can index"); goto done; }
        HIPCHK(hipMalloc((void **)&gr->ukeys, sizeof(uint32_t) << lg));
        HIPCHK(hipMalloc((void **)&gr->reach, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32)));
        HIPCHK(hipMemsetAsync(gr->ukeys, 0, sizeof(uint32_t) << lg, (hipStream_t)oslam_stream()));
        HIPCHK(hipMemsetAsync(gr->reach, 0, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32), (hipStream_t)oslam_stream()));
        HIPCHK(hipMemsetAsync(d_small, 0, 2 * sizeof(uint32_t), (hipStream_t)oslam_stream()));
        /* every member's keys into the group's table */
        for (k = 0; k < gr->n; k++) {
            t = models[gr->members[k]]->table;
            t.ukeys = gr->ukeys;
            t.ucap = 1u << lg;
            t.ushift = 32 - lg;
            KCHK(oslamk_union_build(t, d_small, d_small + 1, oslam_stream()));
        }
        t.reach = gr->reach;
        KCHK(oslamk_reach_build(t, models[gr->members[0]]->d_dist, oslam_stream()));
        /* the key numbers of the group: by the entries of all its members under each key */
        for (k = 0; k < gr->n; k++) parts[k] = models[gr->members[k]]->table;
        rc = oslam_build_kmap(&t, models[gr->members[0]]->d_dist, parts, gr->n, models[gr->members[0]]->params.vote_order);
        gr->kmap = t.kmap;
        gr->uids = t.uids;
        if (rc != OSLAM_OK) goto done;
        HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
        HIPCHK(hipMemcpy(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost));
        if (h_small[1]) { rc = fail(OSLAM_E_LIMIT, "union key table overflow"); goto done; }
        /* the members look their buckets up under the group's slots from now on */
        for (k = 0; k < gr->n; k++) {
            oslam_model *m = models[gr->members[k]];
            (void)hipFree(m->table.ukeys);
            (void)hipFree(m->table.reach);
            if (m->table.kmap) (void)hipFree(m->table.kmap);
            if (m->table.uids) (void)hipFree(m->table.uids);
            m->table.ukeys = gr->ukeys;
            m->table.reach = gr->reach;
            m->table.kmap = gr->kmap;
            m->table.uids = gr->uids;
            m->table.kmap_bins = t.kmap_bins;
            m->table.reach_words = t.reach_words;
            m->table.n_ids = t.n_ids;
            m->table.id_bits = t.id_bits;
            m->table.uinfo_stride = t.uinfo_stride;
            m->table.ucap = 1u << lg;
            m->table.ushift = 32 - lg;
            m->shared_union = 1;
            rc = oslam_build_uinfo(m);
            if (rc != OSLAM_OK) goto done;
        }
        HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    }
done:
    free(parts);
    if (d_small) (void)hipFree(d_small);
    if (rc != OSLAM_OK) { oslam_db_destroy(db); return rc; }
    *out = db;
    return OSLAM_OK;
}

int oslam_db_align(oslam_db *db, oslam_scene *s, float *T_out, oslam_stats *stats)
{
    return oslam_db_align_frame(db, s, T_out, stats, NULL, NULL);
}

int oslam_db_align_frame(oslam_db *db, oslam_scene *s, float *T_out, oslam_stats *stats, const oslam_inst_req *reqs,
                         oslamk_inst_out *sels)
{
    int rc = OSLAM_OK, g, k, first_err = OSLAM_OK;
    scratch_pool *pool = NULL;
    oslamk_counters *cnt = NULL;
    oslam_model **ms = NULL;
    int *on_dev = NULL;               /* per member of the current group: 0, or the number of cells its device tail kept */
    double t0 = now_ms();
    if (!db || !s || !T_out) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(T_out, 0, sizeof(float) * 16 * db->n);
    if (stats) memset(stats, 0, sizeof *stats * db->n);
    if (sels)
        for (k = 0; k < (int)db->n; k++) sels[k].n = 0;
    for (k = 0; k < (int)db->n; k++) {
        rc = oslam_check_pair(db->models[k], s);
        if (rc != OSLAM_OK) return rc;
    }
    cnt = (oslamk_counters *)malloc(sizeof *cnt * db->n);
    ms = (oslam_model **)malloc(sizeof *ms * db->n);
    on_dev = (int *)malloc(sizeof *on_dev * (db->n ? db->n : 1));
    if (!cnt || !ms || !on_dev) rc = fail(OSLAM_E_NOMEM, "host allocation failed");
    else rc = oslam_pool_enter(db->dev, &pool);
    for (g = 0; g < db->n_groups && rc == OSLAM_OK; g++) {
        db_group *gr = &db->groups[g];
        oslam_vote_times share;      /* of one member in the group's pass */
        memset(&share, 0, sizeof share);
        for (k = 0; k < gr->n; k++) ms[k] = db->models[gr->members[k]];
        if (gr->n > 1) {
            /* one scene pass, every member's votes behind it */
            rc = oslam_run_votes_group(pool, ms, gr->n, s, s->d_ref_idx, s->d_tsg, s->n_ref, 0, NULL, cnt, &share);
            if (rc != OSLAM_OK) break;
            /* num_hits is the group pass's (pairs whose key is in some member); its times are shared out evenly */
            share.ms /= (float)gr->n;
            share.ms_vote_kernel /= (float)gr->n;
            share.ms_key_kernel /= (float)gr->n;
        }
        /* The pose tails of the group's members, in flight together: every member's selection of its peak records is
         * enqueued, one wait, then every member's chain (order, poses, clustering scores, winner), one wait -- two
         * waits per group instead of two per model, and the kernels of one model run while the next one's are being
         * launched (50 models on a depth frame: 36 -> 32.6 ms together with the single packed sort).  A member whose records did not fit its buffer, whose
         * tail belongs to the host (few records, or a host-only variant), or with fewer than two records above the
         * threshold goes through the single-model path afterwards. */
        memset(on_dev, 0, sizeof *on_dev * (size_t)gr->n);
        if (gr->n > 1) {
            uint32_t n_max = 0;
            for (k = 0; k < gr->n; k++) {
                oslam_model *m = ms[k];
                if (cnt[k].out_count <= m->out_cap && oslam_pose_gpu_from(m) && cnt[k].out_count >= oslam_pose_gpu_from(m)) {
                    on_dev[k] = 1;
                    if (cnt[k].out_count > n_max) n_max = (uint32_t)cnt[k].out_count;
                }
            }
            if (n_max) {
                int kk;
                for (k = 0; k < gr->n && rc == OSLAM_OK; k++)
                    if (on_dev[k]) {
                        rc = oslam_pose_tables(ms[k], s);
                        if (rc == OSLAM_OK) rc = oslam_ensure_pose_buffers(ms[k], (size_t)cnt[k].out_count);
                    }
                if (rc != OSLAM_OK) break;
                kk = oslamk_pose_reserve(n_max, (uint32_t)gr->n, oslam_rotx(), oslam_stream());
                for (k = 0; k < gr->n && kk == 0; k++)
                    if (on_dev[k])
                        kk = oslamk_pose_select_async(ms[k]->d_out, (uint32_t)cnt[k].out_count,
                                                      ms[k]->params.vote_count_threshold * cnt[k].gmax, ms[k]->d_pose_cells,
                                                      (uint32_t)k, oslam_stream());
                if (kk == 0) kk = (int)hipStreamSynchronize((hipStream_t)oslam_stream());
                for (k = 0; k < gr->n && kk == 0; k++)
                    if (on_dev[k]) {
                        const uint32_t n_sel = oslamk_pose_selected((uint32_t)k);
                        if (n_sel < 2) { on_dev[k] = 0; continue; }
                        on_dev[k] = (int)n_sel;
                        kk = oslamk_pose_finish_async(n_sel, ms[k]->d_pose_cells, ms[k]->d_Tm16, s->d_Ts16, s->df, ms[k]->d_weights,
                                                      ms[k]->d_dist, ms[k]->params.use_l1_norm, ms[k]->d_pose_cells,
                                                      ms[k]->d_pose_T, cnt[k].gmax, (uint32_t)ms[k]->c.n, (uint32_t)s->c.n,
                                                      ms[k]->params.pose_two_sorts, reqs ? &reqs[gr->members[k]].a : NULL,
                                                      (uint32_t)k, oslam_stream());
                    }
                if (kk == 0) kk = (int)hipStreamSynchronize((hipStream_t)oslam_stream());
                if (kk != 0) { rc = fail(OSLAM_E_DEVICE, hipGetErrorString((hipError_t)kk)); break; }
            }
        }
        for (k = 0; k < gr->n && rc == OSLAM_OK; k++) {
            oslam_model *m = ms[k];
            oslam_stats local, *st = stats ? &stats[gr->members[k]] : &local;
            float *T = T_out + 16 * gr->members[k];
            size_t n = 0;
            int arc;
            memset(st, 0, sizeof *st);
            if (gr->n > 1 && cnt[k].out_count <= m->out_cap) {
                oslam_vote_stats(st, pool, m, s, &cnt[k], &share);
                if (on_dev[k]) {                            /* its chain has run: the winner is in its slot */
                    uint32_t best = 0;
                    oslamk_pose_result((uint32_t)k, &best, T);
                    if (sels) oslamk_pose_instances((uint32_t)k, &sels[gr->members[k]]);
                    oslam_drop_last(m);
                    m->n_last = (size_t)on_dev[k];
                    m->last_on_device = 1;
                    st->num_top = (uint64_t)on_dev[k];
                    st->ms_total = (float)(now_ms() - t0);
                    continue;
                }
                /* the device tail has had its chance above */
                arc = oslam_finish_after_votes(m, s, cnt[k].out_count, cnt[k].gmax, 0, T, st, reqs ? &reqs[gr->members[k]] : NULL,
                                               sels ? &sels[gr->members[k]] : NULL);
            } else {
                /* a group of one -- or a member whose peak records did not fit its buffer: the single-model path */
                arc = oslam_vote_records(pool, m, s, &cnt[k], &n, st, 0);
                if (arc == OSLAM_OK)
                    arc = oslam_finish_after_votes(m, s, n, cnt[k].gmax, 1, T, st, reqs ? &reqs[gr->members[k]] : NULL,
                                                   sels ? &sels[gr->members[k]] : NULL);
            }
            if (arc != OSLAM_OK && arc != OSLAM_E_NO_VOTES) rc = arc;
            else if (arc == OSLAM_E_NO_VOTES && first_err == OSLAM_OK) first_err = arc;
            st->ms_total = (float)(now_ms() - t0);
        }
    }
    oslam_pool_unlock(pool);
    free(cnt);
    free(ms);
    free(on_dev);
    (void)first_err;                  /* a model without votes leaves its T zero, as oslam_ppf_registration does */
    return rc;
}

int oslam_db_size(const oslam_db *db, size_t *n_models, size_t *n_groups)
{
    if (!db) return fail(OSLAM_E_INVALID, "NULL handle");
    if (n_models) *n_models = db->n;
    if (n_groups) *n_groups = (size_t)db->n_groups;
    return OSLAM_OK;
}

/* The database split by model (see oslam.h): this rank's models against the whole scene, then every pose to every
 * rank in one all-gather of {found, error, 16 floats} per model slot.  A rank without the exchange buffers gives the
 * communicator up; any later error on one rank travels in its slots' error word (OSLAM_E_PEER on the others). */
int oslam_db_align_multi(oslam_db *db, oslam_scene *s, oslam_comm *c, size_t n_total, float *T_out, int *found_out,
                         oslam_stats *stats_local)
{
    int rc = OSLAM_OK, lrc = OSLAM_OK, any = 0, r, together = 0;   /* together: every rank leaves at this point */
    size_t n_mine, block, k, words;
    uint32_t *h_send = NULL, *h_recv = NULL, *d_buf = NULL;
    float *T_loc = NULL;
    hipStream_t st = (hipStream_t)oslam_stream();
    if (!s || !c || !T_out || n_total == 0) return fail(OSLAM_E_INVALID, "NULL argument");
    if (c->broken) return fail(OSLAM_E_DEVICE, "the communicator was aborted after a failed collective: make a new one");
    if (s->world != 1) return fail(OSLAM_E_INVALID, "a database split by model takes the whole scene on every rank (shard_world 1)");
    n_mine = (n_total + (size_t)c->world - 1 - (size_t)c->rank) / (size_t)c->world;     /* models rank, rank + world, ... */
    block = (n_total + (size_t)c->world - 1) / (size_t)c->world;
    if ((db ? db->n : 0) != n_mine) return fail(OSLAM_E_INVALID, "this rank's database does not hold models rank, rank + world, ... of n_total");
    memset(T_out, 0, sizeof(float) * 16 * n_total);
    if (found_out) memset(found_out, 0, sizeof(int) * n_total);
    words = 18 * block;
    h_send = (uint32_t *)calloc(words ? words : 1, sizeof(uint32_t));
    h_recv = (uint32_t *)malloc(sizeof(uint32_t) * (words ? words : 1) * (size_t)c->world);
    T_loc = (float *)calloc(16 * (n_mine ? n_mine : 1), sizeof(float));
    if (!h_send || !h_recv || !T_loc) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    HIPCHK(hipSetDevice(c->dev));
    if (hipMalloc((void **)&d_buf, sizeof(uint32_t) * words * (size_t)(c->world + 1)) != hipSuccess) {
        d_buf = NULL;
        rc = fail(OSLAM_E_NOMEM, "no device memory for the pose exchange");
        goto done;
    }
    if (n_mine) lrc = oslam_db_align(db, s, T_loc, stats_local);
    for (k = 0; k < block; k++) {
        uint32_t *slot = h_send + 18 * k;
        slot[1] = lrc != OSLAM_OK || c->inject_stage == OSLAM_STAGE_VOTE;
        if (k < n_mine && lrc == OSLAM_OK) {
            int nz = 0, q;
            for (q = 0; q < 16; q++) nz |= T_loc[16 * k + q] != 0.0f;
            slot[0] = (uint32_t)nz;             /* a model without votes leaves its pose all zeros */
            memcpy(slot + 2, T_loc + 16 * k, 16 * sizeof(float));
        }
    }
    HIPCHK(hipMemcpyAsync(d_buf, h_send, sizeof(uint32_t) * words, hipMemcpyHostToDevice, st));
    rc = oslam_comm_all_gather(c, d_buf, d_buf + words, words, oslam_stream());
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipMemcpyAsync(h_recv, d_buf + words, sizeof(uint32_t) * words * (size_t)c->world, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    together = 1;
    for (r = 0; r < c->world; r++)
        for (k = 0; k < block; k++) any |= h_recv[((size_t)r * block + k) * 18 + 1] != 0;
    if (any) { rc = oslam_comm_error(c, lrc, OSLAM_STAGE_VOTE); goto done; }
    for (r = 0; r < c->world; r++)
        for (k = 0; k < block; k++) {
            const size_t j = k * (size_t)c->world + (size_t)r;
            const uint32_t *slot = h_recv + ((size_t)r * block + k) * 18;
            if (j >= n_total) continue;
            memcpy(T_out + 16 * j, slot + 2, 16 * sizeof(float));
            if (found_out) found_out[j] = (int)slot[0];
        }
done:
    /* this rank left before the exchange, or a HIP call failed around it: its peers cannot be told any more */
    if (rc != OSLAM_OK && !together) (void)oslam_comm_abort(c);
    c->inject_stage = OSLAM_STAGE_NONE;
    free(h_send);
    free(h_recv);
    free(T_loc);
    if (d_buf) (void)hipFree(d_buf);
    return rc;
}

int oslam_ppf_registration(const float *const *scene_xyz, const float *const *scene_nrm,
                           const size_t *scene_n, size_t n_scenes, const float *const *model_xyz,
                           const float *const *model_nrm, const size_t *model_n, size_t n_models,
                           size_t stride_bytes, const float *model_d_dists, unsigned df,
                           float vote_count_threshold, int cpu_clustering, int use_l1_norm,
                           int use_averaged_clusters, int devUse, const float *model_weights,
                           float *T_out)
{
    oslam_params p;
    oslam_model **models = NULL;
    oslam_db *db = NULL;
    size_t i, j;
    int rc = OSLAM_OK;
    (void)model_weights;                       /* ignored by the reference too: ppf.cu:35 */
    if (!scene_xyz || !scene_nrm || !scene_n || !model_xyz || !model_nrm || !model_n || !model_d_dists || !T_out)
        return fail(OSLAM_E_INVALID, "NULL argument");
    oslam_params_default(&p);
    p.ref_point_df = df;
    p.vote_count_threshold = vote_count_threshold;
    p.cpu_clustering = cpu_clustering;
    p.use_l1_norm = use_l1_norm;
    p.use_averaged_clusters = use_averaged_clusters;
    p.dev = devUse;
    memset(T_out, 0, sizeof(float) * 16 * n_scenes * n_models);
    models = (oslam_model **)calloc(n_models ? n_models : 1, sizeof *models);
    if (!models) return fail(OSLAM_E_NOMEM, "host allocation failed");
    /* models are built once and stay resident (the reference rebuilds per pair) */
    for (j = 0; j < n_models && rc == OSLAM_OK; j++)
        rc = oslam_model_create(model_xyz[j], model_nrm[j], model_n[j], stride_bytes, model_d_dists[j], &p, &models[j]);
    if (rc == OSLAM_OK && n_models) rc = oslam_db_create(models, n_models, &db);
    for (i = 0; i < n_scenes && rc == OSLAM_OK && n_models; i++) {
        /* one scene object for all models: the reference prepares the scene per model because its
         * pair keys depend on the model's d_dist (ppf.cu:64-67); here they are made inside the align,
         * once per group of models that share a d_dist */
        oslam_scene *sc = NULL;
        rc = oslam_scene_create(scene_xyz[i], scene_nrm[i], scene_n[i], stride_bytes, 0.0f, df, &p, &sc);
        if (rc == OSLAM_OK) rc = oslam_db_align(db, sc, T_out + 16 * (i * n_models), NULL);
        oslam_scene_destroy(sc);
    }
    oslam_db_destroy_with_models(db);         /* the models go next: no key tables are rebuilt for them */
    for (j = 0; j < n_models; j++) oslam_model_destroy(models[j]);
    free(models);
    return rc;
}
