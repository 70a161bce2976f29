/*
 * oslam_tracker.c -- identity across depth frames (include/oslam.h at oslam_tracker_step): a host-side object over the
 * stages, with no kernel of its own.  A step tracks every live track from its last pose (oslam_db_track), arbitrates
 * the ones that were found, ages and deletes, and now and then runs the search (oslam_db_detect) and folds its
 * detections into the tracks (oslam_tracker_update: association by the same-instance test, birth).  Under a moving
 * camera oslam_tracker_step_cam first moves every live pose by the camera's motion (predict) and accumulates the camera.
 */
#include <math.h>

#include "oslam_internal.h"
#include "oslam_pose.h"

struct oslam_tracker {
    oslam_db *db;                     /* borrowed; NULL for a tracker made from shapes */
    size_t n_models;
    float *centroid, *extent;         /* [n_models][3], [n_models]: the instance rule's shape of every member */
    oslam_tracker_params p;
    oslam_track_state *tracks;        /* live, ordered by id (births append the largest id) */
    size_t n, cap;
    uint32_t next_id;
    uint64_t frame;
    double T_world_cam[16];           /* the camera in the frame of the first step's camera (oslam_tracker_predict) */
};

int oslam_tracker_params_default(oslam_tracker_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    oslam_track_params_default(&p->track);
    oslam_detect_params_default(&p->detect);
    oslam_arbitrate_params_default(&p->arbitrate);
    p->max_misses = 2;
    p->detect_every = 10;
    p->assoc_min_separation = 0.5f;
    p->assoc_max_angle = 3.14159265358979323846f;
    return OSLAM_OK;
}

static int check_params(const oslam_tracker_params *in, oslam_tracker_params *out)
{
    oslam_track_params tp;
    oslam_refine_params rp;
    oslam_verify_params vp;
    oslam_arbitrate_params ap;
    oslam_instance_params ip;
    int rc;
    if (in) *out = *in;
    else oslam_tracker_params_default(out);
    rc = oslam_track_check_params(&out->track, &tp);
    if (rc == OSLAM_OK) rc = oslam_arbitrate_check_params(&out->arbitrate, &ap);
    if (rc == OSLAM_OK) rc = oslam_refine_check_params(&out->detect.refine, &rp);
    if (rc == OSLAM_OK) rc = oslam_verify_check_params(&out->detect.verify, &vp);
    if (rc == OSLAM_OK) rc = oslam_arbitrate_check_params(&out->detect.arbitrate, &ap);
    if (rc != OSLAM_OK) return rc;
    if (oslam_instance_params_check(&out->detect.instances, out->detect.instances.max_instances) != OSLAM_OK)
        return fail(OSLAM_E_INVALID, "instance parameters out of range");
    if (out->detect_every == 0) return fail(OSLAM_E_INVALID, "detect_every must be >= 1");
    /* the association thresholds are an instance rule's: the same ranges */
    oslam_instance_params_default(&ip);
    ip.min_separation = out->assoc_min_separation;
    ip.max_angle = out->assoc_max_angle;
    if (oslam_instance_params_check(&ip, ip.max_instances) != OSLAM_OK)
        return fail(OSLAM_E_INVALID, "assoc_min_separation must be >= 0 and assoc_max_angle lie in [0, pi]");
    return OSLAM_OK;
}

static int tracker_new(size_t n, const oslam_tracker_params *p, oslam_tracker **out)
{
    oslam_tracker *t = (oslam_tracker *)calloc(1, sizeof *t);
    if (!t) return fail(OSLAM_E_NOMEM, "host allocation failed");
    t->centroid = (float *)calloc(n ? n : 1, 3 * sizeof(float));
    t->extent = (float *)calloc(n ? n : 1, sizeof(float));
    if (!t->centroid || !t->extent) {
        oslam_tracker_destroy(t);
        return fail(OSLAM_E_NOMEM, "host allocation failed");
    }
    t->n_models = n;
    t->p = *p;
    t->T_world_cam[0] = t->T_world_cam[5] = t->T_world_cam[10] = t->T_world_cam[15] = 1.0;
    *out = t;
    return OSLAM_OK;
}

int oslam_tracker_create(oslam_db *db, const oslam_tracker_params *p, oslam_tracker **out)
{
    oslam_tracker_params q;
    size_t j;
    int rc;
    if (out) *out = NULL;
    if (!db || !out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = check_params(p, &q);
    if (rc != OSLAM_OK) return rc;
    rc = tracker_new(db->n, &q, out);
    if (rc != OSLAM_OK) return rc;
    (*out)->db = db;
    for (j = 0; j < db->n; j++) {
        memcpy((*out)->centroid + 3 * j, db->models[j]->inst_c, 3 * sizeof(float));
        (*out)->extent[j] = db->models[j]->inst_extent;
    }
    return OSLAM_OK;
}

int oslam_tracker_create_shapes(const float *centroid, const float *extent, size_t n, const oslam_tracker_params *p,
                                oslam_tracker **out)
{
    oslam_tracker_params q;
    size_t j;
    int rc;
    if (out) *out = NULL;
    if (!centroid || !extent || !out || n == 0) return fail(OSLAM_E_INVALID, "NULL argument or no models");
    for (j = 0; j < n; j++)
        if (!isfinite(centroid[3 * j]) || !isfinite(centroid[3 * j + 1]) || !isfinite(centroid[3 * j + 2]) ||
            !isfinite(extent[j]) || extent[j] < 0.0f)
            return fail(OSLAM_E_INVALID, "a centroid or an extent is not finite");
    rc = check_params(p, &q);
    if (rc != OSLAM_OK) return rc;
    rc = tracker_new(n, &q, out);
    if (rc != OSLAM_OK) return rc;
    memcpy((*out)->centroid, centroid, 3 * n * sizeof(float));
    memcpy((*out)->extent, extent, n * sizeof(float));
    return OSLAM_OK;
}

void oslam_tracker_destroy(oslam_tracker *t)
{
    if (!t) return;
    free(t->centroid);
    free(t->extent);
    free(t->tracks);
    free(t);
}

static int reserve(oslam_tracker *t, size_t need)
{
    oslam_track_state *q;
    size_t cap = t->cap ? t->cap : 16;
    if (need <= t->cap) return OSLAM_OK;
    while (cap < need) cap *= 2;
    q = (oslam_track_state *)realloc(t->tracks, sizeof *q * cap);
    if (!q) return fail(OSLAM_E_NOMEM, "host allocation failed");
    t->tracks = q;
    t->cap = cap;
    return OSLAM_OK;
}

int oslam_tracker_update(oslam_tracker *t, const oslam_detection *det, size_t n)
{
    oslam_instance_params ip;
    size_t k, q;
    if (!t || (n && !det)) return fail(OSLAM_E_INVALID, "NULL argument");
    for (k = 0; k < n; k++) {
        if (det[k].model >= t->n_models) return fail(OSLAM_E_INVALID, "a detection names a model outside the database");
        if (oslam_refine_check_rigid(det[k].T) != OSLAM_OK) return OSLAM_E_INVALID;
    }
    oslam_instance_params_default(&ip);
    ip.min_separation = t->p.assoc_min_separation;
    ip.max_angle = t->p.assoc_max_angle;
    for (k = 0; k < n; k++) {
        const oslam_detection *d = &det[k];
        const float *c = t->centroid + 3 * d->model;
        float sep2, cos_thr, pd[3], best = 0.0f;
        int rot_on, have = 0;
        oslam_instance_thresholds(&ip, t->extent[d->model], &sep2, &cos_thr, &rot_on);
        oslam_instance_centroid(d->T, c, pd);
        for (q = 0; q < t->n; q++) {            /* id ascending: < keeps the lower id of a tie */
            const oslam_track_state *s = &t->tracks[q];
            float pt[3], dx, dy, dz, d2;
            if (s->model != d->model) continue;
            oslam_instance_centroid(s->T, c, pt);
            if (!oslam_same_instance(pd, d->T, pt, s->T, sep2, cos_thr, rot_on)) continue;
            dx = pd[0] - pt[0];
            dy = pd[1] - pt[1];
            dz = pd[2] - pt[2];
            d2 = (dx * dx + dy * dy) + dz * dz;
            if (!have || d2 < best) {
                best = d2;
                have = 1;
            }
        }
        if (have) continue;                     /* matched: the tracked pose is the fresher one */
        if (reserve(t, t->n + 1) != OSLAM_OK) return OSLAM_E_NOMEM;
        {
            oslam_track_state *s = &t->tracks[t->n++];
            memset(s, 0, sizeof *s);
            s->id = t->next_id++;
            s->model = d->model;
            memcpy(s->T, d->T, sizeof s->T);
            s->hits = 1;
            s->found = 1;
        }
    }
    return OSLAM_OK;
}

int oslam_tracker_tracks(const oslam_tracker *t, oslam_track_state *out, size_t cap, size_t *n_out)
{
    if (!t || !n_out || (cap && !out)) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = t->n;
    if (t->n > cap) return fail(OSLAM_E_LIMIT, "more live tracks than out holds");
    if (t->n) memcpy(out, t->tracks, sizeof *out * t->n);
    return OSLAM_OK;
}

/* step 0 of oslam_tracker_step_cam: T <- float32(T_cam * T) of every live track, T_world_cam <- T_world_cam * T_cam^-1 */
static void predict(oslam_tracker *t, const float C[16])
{
    double W[12], inv[12];
    size_t k;
    int a;
    for (k = 0; k < t->n; k++) {
        float *T = t->tracks[k].T, N[12];
        oslam_rigid_product_f(C, T, N);
        for (a = 0; a < 12; a++)
            if (N[a] != T[a]) T[a] = N[a];      /* an element whose value does not change keeps its bits */
    }
    oslam_rigid_inverse(C, inv);
    memcpy(W, t->T_world_cam, sizeof W);
    oslam_rigid_product(W, inv, t->T_world_cam);
}

int oslam_tracker_predict(oslam_tracker *t, const float T_cam[16])
{
    if (!t || !T_cam) return fail(OSLAM_E_INVALID, "NULL argument");
    if (oslam_refine_check_rigid(T_cam) != OSLAM_OK) return OSLAM_E_INVALID;
    predict(t, T_cam);
    return OSLAM_OK;
}

int oslam_tracker_camera(const oslam_tracker *t, float T_world_cam[16])
{
    int a;
    if (!t || !T_world_cam) return fail(OSLAM_E_INVALID, "NULL argument");
    for (a = 0; a < 16; a++) T_world_cam[a] = (float)t->T_world_cam[a];
    return OSLAM_OK;
}

int oslam_tracker_step(oslam_tracker *t, oslam_scene *scene, const oslam_view *v, oslam_track_state *out, size_t cap,
                       size_t *n_out, int *searched)
{
    return oslam_tracker_step_cam(t, scene, v, NULL, out, cap, n_out, searched);
}

int oslam_tracker_step_cam(oslam_tracker *t, oslam_scene *scene, const oslam_view *v, const float T_cam[16],
                           oslam_track_state *out, size_t cap, size_t *n_out, int *searched)
{
    int rc = OSLAM_OK, any = 0;
    size_t k, H, kept = 0;
    uint32_t *member = NULL;
    oslam_model **ms = NULL;
    float *T = NULL, *T_new = NULL, *Tz = NULL;
    oslam_track_result *res = NULL;
    oslam_arbitrate_result *ares = NULL;
    oslam_detection *det = NULL;
    if (searched) *searched = 0;
    if (!t || !v || !n_out || (cap && !out)) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = 0;
    if (T_cam && oslam_refine_check_rigid(T_cam) != OSLAM_OK) return OSLAM_E_INVALID;
    if (!t->db) return fail(OSLAM_E_INVALID, "a tracker made from shapes has no database to step with");
    H = t->n;
    if (H > OSLAM_ARBITRATE_MAX_HYPOTHESES) return fail(OSLAM_E_LIMIT, "more live tracks than one tracking call takes");
    if (T_cam) predict(t, T_cam);
    if (H) {
        member = (uint32_t *)malloc(sizeof *member * H);
        ms = (oslam_model **)malloc(sizeof *ms * H);
        T = (float *)malloc(sizeof(float) * 16 * H);
        T_new = (float *)malloc(sizeof(float) * 16 * H);
        Tz = (float *)calloc(16 * H, sizeof(float));
        res = (oslam_track_result *)malloc(sizeof *res * H);
        ares = (oslam_arbitrate_result *)calloc(H, sizeof *ares);
        if (!member || !ms || !T || !T_new || !Tz || !res || !ares) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        for (k = 0; k < H; k++) {
            member[k] = t->tracks[k].model;
            ms[k] = t->db->models[member[k]];
            memcpy(T + 16 * k, t->tracks[k].T, 16 * sizeof(float));
        }
        rc = oslam_db_track(t->db, member, T, H, v, &t->p.track, T_new, res);
        if (rc != OSLAM_OK) goto done;
        for (k = 0; k < H; k++)
            if (res[k].found) {
                memcpy(Tz + 16 * k, T_new + 16 * k, 16 * sizeof(float));
                any = 1;
            }
        if (any) {
            rc = oslam_arbitrate(ms, Tz, H, v, &t->p.arbitrate, ares);
            if (rc != OSLAM_OK) goto done;
        }
        for (k = 0; k < H; k++) {
            oslam_track_state *s = &t->tracks[k];
            const int found = res[k].found && ares[k].kept;
            s->age++;
            s->track = res[k];
            s->found = found;
            if (found) {
                memcpy(s->T, T_new + 16 * k, sizeof s->T);
                s->hits++;
                s->misses = 0;
            } else {
                s->misses++;
                if (s->misses > t->p.max_misses) continue;      /* deleted */
            }
            if (kept != k) t->tracks[kept] = *s;
            kept++;
        }
        t->n = kept;
    }
    if (scene && (t->n == 0 || t->frame % t->p.detect_every == 0)) {
        const size_t dcap = t->db->n * (size_t)t->p.detect.instances.max_instances;
        size_t nd = 0;
        det = (oslam_detection *)malloc(sizeof *det * (dcap ? dcap : 1));
        if (!det) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        rc = oslam_db_detect(t->db, scene, v, &t->p.detect, det, dcap ? dcap : 1, &nd);
        if (rc != OSLAM_OK) goto done;
        if (searched) *searched = 1;
        rc = oslam_tracker_update(t, det, nd);
        if (rc != OSLAM_OK) goto done;
    }
    t->frame++;
    rc = oslam_tracker_tracks(t, out, cap, n_out);
done:
    free(member);
    free(ms);
    free(T);
    free(T_new);
    free(Tz);
    free(res);
    free(ares);
    free(det);
    return rc;
}
