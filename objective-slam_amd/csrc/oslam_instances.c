/*
 * oslam_instances.c -- every instance of a model in a scene (include/oslam.h at oslam_align_instances): the vote path
 * and pose tail of oslam_align / oslam_db_align with the instance selection asked of the tail (k_pose_instances on the
 * device, oslam_select_instances on the host), then one refinement over every accepted instance, deduplication of
 * the refined poses and the presence filter.
 */
#include <math.h>

#include "oslam_internal.h"
#include "oslam_pose.h"

static int check_args(const oslam_instance_params *ip, const oslam_refine_params *rp, size_t cap, oslam_refine_params *rpc)
{
    if (oslam_instance_params_check(ip, cap) != OSLAM_OK)
        return oslam_fail(OSLAM_E_INVALID, "instance parameters out of range (max_instances 1..64 and <= cap, min_separation "
                                           ">= 0, max_angle in [0, pi], min_score_ratio in [0, 1])");
    return rp ? oslam_refine_check_params(rp, rpc) : OSLAM_OK;
}

/* the rule resolved for m: its centroid and extent are the model's shape (oslam_model.c) */
static void make_req(const oslam_model *m, const oslam_instance_params *ip, oslam_inst_req *req)
{
    int rot_on = 0;
    memset(req, 0, sizeof *req);
    req->ip = ip;
    req->extent = m->inst_extent;
    req->a.max_instances = ip->max_instances;
    req->a.ratio = ip->min_score_ratio;
    oslam_instance_thresholds(ip, m->inst_extent, &req->a.sep2, &req->a.cos_thr, &rot_on);
    req->a.rot_on = rot_on;
    memcpy(req->a.c, m->inst_c, sizeof req->a.c);
}

/* the winners of the tail -> out[]; an all-zero instance 0 (oslam_align's all-zero T) gives none */
static size_t fill_out(const oslamk_inst_out *sel, oslam_instance *out)
{
    size_t k;
    if (sel->n == 0 || oslam_is_zero_pose(sel->T[0])) return 0;
    for (k = 0; k < sel->n; k++) {
        oslam_instance *o = &out[k];
        memset(o, 0, sizeof *o);
        memcpy(o->T_vote, sel->T[k], sizeof o->T_vote);
        memcpy(o->T, sel->T[k], sizeof o->T);
        o->score = sel->score[k];
        o->candidate = sel->idx[k];
    }
    return sel->n;
}

/* One refinement over the instances of every list j (out + j*cap, n_out[j] of them, model models[j]), then per list:
 * drop an instance that is the same instance as an earlier kept one (refined poses), then the ones not found. */
static int refine_lists(oslam_model *const *models, const oslam_inst_req *reqs, size_t nm, oslam_scene *s,
                        const oslam_refine_params *p, int keep_not_found, oslam_instance *out, size_t cap, size_t *n_out)
{
    size_t j, k, q, total = 0, at = 0;
    oslam_model **ms = NULL;
    float *T_in = NULL, *T_out = NULL, *pc = NULL;
    oslam_refine_result *res = NULL;
    int rc = OSLAM_OK;
    for (j = 0; j < nm; j++) total += n_out[j];
    if (total == 0) return OSLAM_OK;
    ms = (oslam_model **)malloc(sizeof *ms * total);
    T_in = (float *)malloc(sizeof(float) * 16 * total);
    T_out = (float *)malloc(sizeof(float) * 16 * total);
    res = (oslam_refine_result *)malloc(sizeof *res * total);
    pc = (float *)malloc(sizeof(float) * 3 * cap);
    if (!ms || !T_in || !T_out || !res || !pc) { rc = oslam_fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    for (j = 0; j < nm; j++)
        for (k = 0; k < n_out[j]; k++) {
            const float *T = out[j * cap + k].T_vote;
            rc = oslam_refine_check_rigid(T);
            if (rc != OSLAM_OK) goto done;
            ms[at] = models[j];
            memcpy(T_in + 16 * at, T, 16 * sizeof(float));
            at++;
        }
    rc = oslam_refine_members(ms, total, s, T_in, p, T_out, res);
    if (rc != OSLAM_OK) goto done;
    at = 0;
    for (j = 0; j < nm; j++) {
        oslam_instance *o = out + j * cap;
        const oslam_inst_req *r = &reqs[j];
        size_t kept = 0;
        for (k = 0; k < n_out[j]; k++, at++) {
            memcpy(o[k].T, T_out + 16 * at, 16 * sizeof(float));
            o[k].refine = res[at];
        }
        /* deduplicate in acceptance order (not-found ones count as kept here), then the presence filter */
        for (k = 0; k < n_out[j]; k++) {
            int same = 0;
            float pk[3];
            oslam_instance_centroid(o[k].T, r->a.c, pk);
            for (q = 0; q < kept && !same; q++)
                same = oslam_same_instance(pk, o[k].T, pc + 3 * q, o[q].T, r->a.sep2, r->a.cos_thr, r->a.rot_on);
            if (same) continue;
            memcpy(pc + 3 * kept, pk, sizeof pk);
            if (kept != k) o[kept] = o[k];
            kept++;
        }
        n_out[j] = kept;
        kept = 0;
        for (k = 0; k < n_out[j]; k++) {
            if (!keep_not_found && !o[k].refine.found) continue;
            if (kept != k) o[kept] = o[k];
            kept++;
        }
        for (k = kept; k < n_out[j]; k++) memset(&o[k], 0, sizeof o[k]);
        n_out[j] = kept;
    }
done:
    free(ms);
    free(T_in);
    free(T_out);
    free(res);
    free(pc);
    return rc;
}

int oslam_align_instances(oslam_model *m, oslam_scene *s, const oslam_instance_params *ip, const oslam_refine_params *rp,
                          oslam_instance *out, size_t cap, size_t *n_out, oslam_stats *stats)
{
    int rc;
    oslamk_counters cnt;
    oslam_refine_params rpc;
    oslam_inst_req req;
    oslamk_inst_out *sel = NULL;
    oslam_stats local;
    scratch_pool *pool;
    size_t n = 0, n_inst = 0;
    float T[16];
    double t0 = now_ms();
    if (!m || !s || !ip || !out || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = 0;
    rc = check_args(ip, rp, cap, &rpc);
    if (rc != OSLAM_OK) return rc;
    memset(out, 0, sizeof *out * ip->max_instances);
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    sel = (oslamk_inst_out *)malloc(sizeof *sel);
    if (!sel) return fail(OSLAM_E_NOMEM, "host allocation failed");
    make_req(m, ip, &req);
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc == OSLAM_OK) {
        rc = oslam_vote_records(pool, m, s, &cnt, &n, stats, 0);
        if (rc == OSLAM_OK) rc = oslam_finish_after_votes(m, s, n, cnt.gmax, 1, T, stats, &req, sel);
        oslam_pool_unlock(pool);
    }
    if (rc == OSLAM_OK) {
        n_inst = fill_out(sel, out);
        if (rp) rc = refine_lists(&m, &req, 1, s, &rpc, ip->keep_not_found, out, cap, &n_inst);
    }
    free(sel);
    if (rc == OSLAM_OK) *n_out = n_inst;
    stats->ms_total = (float)(now_ms() - t0);
    return rc;
}

int oslam_db_align_instances(oslam_db *db, oslam_scene *s, const oslam_instance_params *ip, const oslam_refine_params *rp,
                             oslam_instance *out, size_t cap, size_t *n_out, oslam_stats *stats)
{
    int rc;
    oslam_refine_params rpc;
    oslam_inst_req *reqs = NULL;
    oslamk_inst_out *sels = NULL;
    float *T = NULL;
    size_t j;
    if (!db || !s || !ip || !out || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_args(ip, rp, cap, &rpc);
    if (rc != OSLAM_OK) return rc;
    memset(n_out, 0, sizeof *n_out * db->n);
    for (j = 0; j < db->n; j++) memset(out + j * cap, 0, sizeof *out * ip->max_instances);
    reqs = (oslam_inst_req *)malloc(sizeof *reqs * (db->n ? db->n : 1));
    sels = (oslamk_inst_out *)malloc(sizeof *sels * (db->n ? db->n : 1));
    T = (float *)malloc(sizeof(float) * 16 * (db->n ? db->n : 1));
    if (!reqs || !sels || !T) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    for (j = 0; j < db->n; j++) make_req(db->models[j], ip, &reqs[j]);
    rc = oslam_db_align_frame(db, s, T, stats, reqs, sels);
    if (rc != OSLAM_OK) goto done;
    for (j = 0; j < db->n; j++) n_out[j] = fill_out(&sels[j], out + j * cap);
    if (rp) rc = refine_lists(db->models, reqs, db->n, s, &rpc, ip->keep_not_found, out, cap, n_out);
    if (rc != OSLAM_OK) memset(n_out, 0, sizeof *n_out * db->n);
done:
    free(reqs);
    free(sels);
    free(T);
    return rc;
}
