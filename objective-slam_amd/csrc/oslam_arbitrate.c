/*
 * oslam_arbitrate.c -- arbitration between hypotheses that claim the same pixels of a depth image (include/oslam.h at
 * oslam_arbitrate): the host side of the kernels in oslam_arbitrate.hip, and oslam_db_detect, the one call that runs
 * align_instances -> verify -> arbitrate for a database frame.  A call checks its arguments, resolves the tile,
 * uploads one descriptor per hypothesis (the descriptor of the verification stage), zeroes the claims table, runs
 * k_claim and k_arbitrate and reads one record per hypothesis back into pinned memory with one host wait.
 */
#include <math.h>
#include <pthread.h>

#include "oslam_internal.h"
#include "oslam_pose.h"

#define ARB_MAX_TABLE_BYTES ((size_t)256 << 20)

/* the pinned record of a call, [1 + OSLAMK_ARB_MAX_HYP]: one for the process, so arbitration calls take turns */
static oslamk_arb_rec *g_rec;
static pthread_mutex_t g_rec_mu = PTHREAD_MUTEX_INITIALIZER;

void oslam_arbitrate_release(void)
{
    pthread_mutex_lock(&g_rec_mu);
    if (g_rec) (void)hipHostFree(g_rec);
    g_rec = NULL;
    pthread_mutex_unlock(&g_rec_mu);
}

int oslam_arbitrate_params_default(oslam_arbitrate_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->depth_tol = 1.0f;
    p->window = 1;
    p->tile = 0;
    p->tile_spacing = 2.0f;
    p->min_tiles = 4;
    p->min_owned_share = 0.52f;
    return OSLAM_OK;
}

int oslam_arbitrate_check_params(const oslam_arbitrate_params *ap, oslam_arbitrate_params *out)
{
    if (ap) *out = *ap;
    else oslam_arbitrate_params_default(out);
    if (!isfinite(out->depth_tol) || !isfinite(out->tile_spacing) || !isfinite(out->min_owned_share))
        return fail(OSLAM_E_INVALID, "arbitrate parameters must be finite");
    if (!(out->depth_tol > 0.0f)) return fail(OSLAM_E_INVALID, "depth_tol must be > 0");
    if (out->window > 3) return fail(OSLAM_E_INVALID, "window above 3");
    if (out->tile != 0 && (out->tile < 4 || out->tile > 128)) return fail(OSLAM_E_INVALID, "tile must be 0 or lie in 4..128");
    if (!(out->tile_spacing > 0.0f)) return fail(OSLAM_E_INVALID, "tile_spacing must be > 0");
    if (out->min_owned_share < 0.0f || out->min_owned_share > 1.0f)
        return fail(OSLAM_E_INVALID, "min_owned_share must lie in [0, 1]");
    return OSLAM_OK;
}

/* the tile of a call (include/oslam.h, "Tile") */
int oslam_arbitrate_choose_tile(oslam_model *const *ms, const float *T, size_t H, const oslam_view *v,
                                const oslam_arbitrate_params *p)
{
    float d_max = 0.0f, z_near = 0.0f;
    size_t h;
    double t;
    if (p->tile) return (int)p->tile;
    for (h = 0; h < H; h++) {
        const float *A = T + 16 * h;
        float zc;
        if (oslam_is_zero_pose(A)) continue;
        if (ms[h]->d_dist > d_max) d_max = ms[h]->d_dist;
        zc = ((A[8] * ms[h]->inst_c[0] + A[9] * ms[h]->inst_c[1]) + A[10] * ms[h]->inst_c[2]) + A[11];
        if (zc > 0.0f && (z_near == 0.0f || zc < z_near)) z_near = zc;
    }
    if (!(z_near > 0.0f)) return 128;
    t = ceil((((double)p->tile_spacing * (double)d_max) * (double)v->k.fx) / (double)z_near);
    return !(t >= 4.0) ? 4 : t > 128.0 ? 128 : (int)t;
}

/* The elimination of a call whose block `dev` holds the descriptors at 0, the claims table at off_tbl and room for
 * 1 + H records at off_rec: k_arbitrate, the records back through the pinned g_rec (made on first use) with one host
 * wait, res[h] filled for every hypothesis that is not skipped.  The caller holds g_rec_mu. */
static int run_elimination(char *dev, size_t off_tbl, size_t off_rec, const oslamk_verify_member *hm, size_t H,
                           uint32_t n_tiles, uint32_t min_tiles, float min_owned_share, void *stream,
                           oslam_arbitrate_result *res, uint32_t *rounds)
{
    int rc = OSLAM_OK;
    size_t h;
    if (!g_rec)
        HIPCHK(hipHostMalloc((void **)&g_rec, sizeof *g_rec * (1 + OSLAMK_ARB_MAX_HYP), hipHostMallocPortable));
    KCHK(oslamk_arbitrate((const oslamk_verify_member *)dev, (uint32_t)H, n_tiles, (const unsigned long long *)(dev + off_tbl),
                          min_tiles, min_owned_share, (oslamk_arb_rec *)(dev + off_rec), stream));
    HIPCHK(hipMemcpyAsync(g_rec, dev + off_rec, sizeof *g_rec * (1 + H), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    *rounds = g_rec[0].claimed;
    for (h = 0; h < H; h++) {
        const oslamk_arb_rec *k = &g_rec[1 + h];
        oslam_arbitrate_result *r = &res[h];
        if (hm[h].n_blocks == 0) continue;
        r->claimed = k->claimed;
        r->owned = k->owned;
        r->share = k->share;
        r->kept = k->kept;
        r->suppressed_by = k->suppressed_by;
        r->mean_residual = k->cnt_total ? (float)((((double)k->sum_total / (double)k->cnt_total) / 65535.0) * (double)hm[h].tol)
                                        : 0.0f;
    }
done:
    return rc;
}

/* the fields of a call that every hypothesis shares, and suppressed_by -1 for the skipped ones */
static void finish_results(oslam_arbitrate_result *res, const oslamk_verify_member *hm, size_t H, uint32_t rounds,
                           uint32_t launches, double t0)
{
    const float ms_total = (float)(now_ms() - t0);
    size_t h;
    for (h = 0; h < H; h++) {
        if (hm[h].n_blocks == 0) res[h].suppressed_by = -1;
        res[h].rounds = rounds;
        res[h].launches = launches;
        res[h].ms_total = ms_total;
    }
}

/* Hypotheses ms[0 .. H) with T [H][16] (all-zero = skipped) against v.  res != NULL: the whole arbitration.
 * cnt_out / sum_out != NULL (the tap): the table after k_claim, H * n_tiles entries each (cap: what they hold). */
static int arbitrate_members(oslam_model *const *ms, size_t H, const oslam_view *v, const float *T,
                             const oslam_arbitrate_params *p, oslam_arbitrate_result *res, uint32_t *cnt_out,
                             uint64_t *sum_out, size_t cap, uint32_t *tile_out, size_t *n_tiles_out)
{
    int rc = OSLAM_OK, locked = 0;
    const double t0 = now_ms();
    size_t h, max_blocks = 0, off_tbl, off_rec, bytes, tbl_bytes, n_ent;
    oslamk_verify_member *hm = NULL;
    uint64_t *h_tbl = NULL;
    oslamk_arb_grid g;
    uint32_t launches = 0, rounds = 0;
    char *dev = NULL;
    void *stream = oslam_stream();

    if (res) memset(res, 0, sizeof *res * H);
    for (h = 0; h < H; h++)
        if (!oslam_is_zero_pose(T + 16 * h) && (size_t)ms[h]->c.n >= ((size_t)1 << 24))
            return fail(OSLAM_E_LIMIT, "a model of 2^24 points or more cannot be arbitrated");
    g.tile = oslam_arbitrate_choose_tile(ms, T, H, v, p);
    g.tiles_x = (v->k.w + g.tile - 1) / g.tile;
    g.n_tiles = (uint32_t)g.tiles_x * (uint32_t)((v->k.h + g.tile - 1) / g.tile);
    n_ent = H * (size_t)g.n_tiles;
    tbl_bytes = n_ent * sizeof(uint64_t);
    if (tile_out) *tile_out = (uint32_t)g.tile;
    if (n_tiles_out) *n_tiles_out = g.n_tiles;
    if (tbl_bytes > ARB_MAX_TABLE_BYTES) return fail(OSLAM_E_LIMIT, "the claims table (hypotheses x tiles x 8 B) exceeds 256 MiB");
    if (cnt_out && n_ent > cap) return fail(OSLAM_E_INVALID, "the claims arrays are too short for hypotheses x tiles");
    if (res)
        for (h = 0; h < H; h++) res[h].tile = (uint32_t)g.tile;
    hm = (oslamk_verify_member *)calloc(H, sizeof *hm);
    if (cnt_out) h_tbl = (uint64_t *)calloc(n_ent, sizeof *h_tbl);
    if (!hm || (cnt_out && !h_tbl)) { free(hm); free(h_tbl); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    for (h = 0; h < H; h++)
        if (!oslam_is_zero_pose(T + 16 * h)) {
            oslam_verify_set_member(&hm[h], ms[h], T + 16 * h, p->depth_tol);
            if (hm[h].n_blocks > max_blocks) max_blocks = hm[h].n_blocks;
        }
    if (max_blocks == 0) {                      /* every hypothesis skipped: no device work */
        if (cnt_out) {
            memset(cnt_out, 0, sizeof *cnt_out * n_ent);
            memset(sum_out, 0, sizeof *sum_out * n_ent);
        }
        goto done;
    }
    if (hipSetDevice(v->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    pthread_mutex_lock(&g_rec_mu);
    locked = 1;
    off_tbl = align256(sizeof *hm * H);
    off_rec = off_tbl + align256(tbl_bytes);
    bytes = off_rec + sizeof(oslamk_arb_rec) * (1 + H);
    KCHK(oslam_dev_alloc((void **)&dev, bytes));
    HIPCHK(hipMemcpyAsync(dev, hm, sizeof *hm * H, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(dev + off_tbl, 0, tbl_bytes, (hipStream_t)stream));
    KCHK(oslamk_claim(&v->k, (const oslamk_verify_member *)dev, (uint32_t)H, (uint32_t)max_blocks, (int)p->window, g,
                      (unsigned long long *)(dev + off_tbl), stream));
    launches++;
    if (cnt_out) {
        HIPCHK(hipMemcpyAsync(h_tbl, dev + off_tbl, tbl_bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        for (h = 0; h < n_ent; h++) {
            cnt_out[h] = (uint32_t)(h_tbl[h] >> OSLAMK_ARB_CNT_SHIFT);
            sum_out[h] = h_tbl[h] & (((uint64_t)1 << OSLAMK_ARB_CNT_SHIFT) - 1);
        }
        goto done;
    }
    rc = run_elimination(dev, off_tbl, off_rec, hm, H, g.n_tiles, p->min_tiles, p->min_owned_share, stream, res, &rounds);
    if (rc != OSLAM_OK) goto done;
    launches++;
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);    /* nothing may still use the block */
    if (locked) pthread_mutex_unlock(&g_rec_mu);
    if (dev) oslam_dev_free(dev);
    if (rc == OSLAM_OK && res) finish_results(res, hm, H, rounds, launches, t0);
    free(hm);
    free(h_tbl);
    return rc;
}

int oslam_arbitrate(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                    const oslam_arbitrate_params *ap, oslam_arbitrate_result *res)
{
    oslam_arbitrate_params p;
    int rc;
    if (!models || !T || !v || !res) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_arbitrate_check_params(ap, &p);
    if (rc == OSLAM_OK) rc = oslam_check_poses(models, T, H, 1);
    if (rc == OSLAM_OK) rc = oslam_check_handles(models, T, H, v);
    if (rc != OSLAM_OK) return rc;
    return arbitrate_members(models, H, v, T, &p, res, NULL, NULL, 0, NULL, NULL);
}

int oslam_db_arbitrate(oslam_db *db, const oslam_view *v, const float *T, const oslam_arbitrate_params *ap,
                       oslam_arbitrate_result *res)
{
    oslam_arbitrate_params p;
    int rc;
    if (!db || !v || !T || !res) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_arbitrate_check_params(ap, &p);
    if (rc != OSLAM_OK) return rc;
    if (db->n && !db->models) return fail(OSLAM_E_INVALID, "the database holds no models");
    rc = oslam_check_poses(db->models, T, db->n, 1);
    if (rc == OSLAM_OK) rc = oslam_check_handles(db->models, T, db->n, v);
    if (rc != OSLAM_OK) return rc;
    return arbitrate_members(db->models, db->n, v, T, &p, res, NULL, NULL, 0, NULL, NULL);
}

int oslam_arbitrate_claims(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                           const oslam_arbitrate_params *ap, uint32_t *cnt_out, uint64_t *sum_out, size_t cap,
                           uint32_t *tile_out, size_t *n_tiles_out)
{
    oslam_arbitrate_params p;
    int rc;
    if (!models || !T || !v || !cnt_out || !sum_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = oslam_arbitrate_check_params(ap, &p);
    if (rc == OSLAM_OK) rc = oslam_check_poses(models, T, H, 1);
    if (rc == OSLAM_OK) rc = oslam_check_handles(models, T, H, v);
    if (rc != OSLAM_OK) return rc;
    return arbitrate_members(models, H, v, T, &p, NULL, cnt_out, sum_out, cap, tile_out, n_tiles_out);
}

/* test tap: k_arbitrate alone over a table given by the caller (include/oslam.h) */
int oslam_arbitrate_table(const uint32_t *cnt, const uint64_t *sum, const uint8_t *skipped, size_t H, size_t n_tiles,
                          unsigned min_tiles, float min_owned_share, oslam_arbitrate_result *res, uint32_t *rounds_out)
{
    int rc = OSLAM_OK, locked = 0, devsel = 0;
    const double t0 = now_ms();
    size_t h, e, n_ent, tbl_bytes, off_tbl, off_rec, live = 0;
    oslamk_verify_member *hm = NULL;
    uint64_t *h_tbl = NULL;
    uint32_t launches = 0, rounds = 0;
    char *dev = NULL;
    void *stream = oslam_stream();

    if (!cnt || !sum || !skipped || !res || !rounds_out) return fail(OSLAM_E_INVALID, "NULL argument");
    *rounds_out = 0;
    if (!isfinite(min_owned_share)) return fail(OSLAM_E_INVALID, "arbitrate parameters must be finite");
    if (min_owned_share < 0.0f || min_owned_share > 1.0f) return fail(OSLAM_E_INVALID, "min_owned_share must lie in [0, 1]");
    if (H == 0 || H > OSLAM_ARBITRATE_MAX_HYPOTHESES)
        return fail(OSLAM_E_INVALID, "the number of hypotheses must lie in 1..OSLAM_ARBITRATE_MAX_HYPOTHESES");
    if (n_tiles == 0 || n_tiles > ARB_MAX_TABLE_BYTES / sizeof(uint64_t)) return fail(OSLAM_E_INVALID, "n_tiles must lie in 1..2^25");
    n_ent = H * n_tiles;
    tbl_bytes = n_ent * sizeof(uint64_t);
    if (tbl_bytes > ARB_MAX_TABLE_BYTES) return fail(OSLAM_E_LIMIT, "the claims table (hypotheses x tiles x 8 B) exceeds 256 MiB");
    for (e = 0; e < n_ent; e++)
        if (cnt[e] >> (64 - OSLAMK_ARB_CNT_SHIFT) || sum[e] >> OSLAMK_ARB_CNT_SHIFT)
            return fail(OSLAM_E_INVALID, "a count of 2^24 or a sum of 2^40 or more does not fit a claims word");
    memset(res, 0, sizeof *res * H);
    hm = (oslamk_verify_member *)calloc(H, sizeof *hm);
    h_tbl = (uint64_t *)malloc(tbl_bytes);
    if (!hm || !h_tbl) { free(hm); free(h_tbl); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    for (h = 0; h < H; h++) {
        hm[h].n_blocks = skipped[h] ? 0u : 1u;   /* k_arbitrate reads nothing else of a member */
        hm[h].tol = 1.0f;
        live += !skipped[h];
    }
    for (e = 0; e < n_ent; e++) h_tbl[e] = ((uint64_t)cnt[e] << OSLAMK_ARB_CNT_SHIFT) | sum[e];
    if (live == 0) goto done;                   /* every hypothesis skipped: no device work, as oslam_arbitrate */
    rc = oslam_pick_device(0, &devsel);
    if (rc != OSLAM_OK) goto done;
    pthread_mutex_lock(&g_rec_mu);
    locked = 1;
    off_tbl = align256(sizeof *hm * H);
    off_rec = off_tbl + align256(tbl_bytes);
    KCHK(oslam_dev_alloc((void **)&dev, off_rec + sizeof(oslamk_arb_rec) * (1 + H)));
    HIPCHK(hipMemcpyAsync(dev, hm, sizeof *hm * H, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(dev + off_tbl, h_tbl, tbl_bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    rc = run_elimination(dev, off_tbl, off_rec, hm, H, (uint32_t)n_tiles, min_tiles, min_owned_share, stream, res, &rounds);
    if (rc != OSLAM_OK) goto done;
    launches++;
done:
    if (rc != OSLAM_OK && dev) (void)hipStreamSynchronize((hipStream_t)stream);
    if (locked) pthread_mutex_unlock(&g_rec_mu);
    if (dev) oslam_dev_free(dev);
    if (rc == OSLAM_OK) {
        finish_results(res, hm, H, rounds, launches, t0);
        *rounds_out = rounds;
    }
    free(hm);
    free(h_tbl);
    return rc;
}

/* ---- the whole chain ---- */
int oslam_detect_params_default(oslam_detect_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    oslam_instance_params_default(&p->instances);
    p->instances.keep_not_found = 1;            /* a depth frame shows one side: verification judges presence, not refine's fitness */
    oslam_refine_params_default(&p->refine);
    oslam_verify_params_default(&p->verify);
    oslam_arbitrate_params_default(&p->arbitrate);
    return OSLAM_OK;
}

int oslam_db_detect(oslam_db *db, oslam_scene *s, const oslam_view *v, const oslam_detect_params *dp, oslam_detection *out,
                    size_t cap, size_t *n_out)
{
    oslam_detect_params p;
    oslam_refine_params rp;
    oslam_verify_params vp;
    oslam_arbitrate_params ap;
    oslam_instance *inst = NULL;
    size_t *n_inst = NULL, *slot = NULL, j, k, total = 0, at = 0, kept = 0, maxi;
    oslam_model **ms = NULL;
    float *T = NULL, *Tz = NULL;
    oslam_verify_result *vres = NULL;
    oslam_arbitrate_result *ares = NULL;
    int rc, any = 0;
    if (!db || !s || !v || !out || !n_out || cap == 0) return fail(OSLAM_E_INVALID, "NULL argument or cap == 0");
    *n_out = 0;
    if (dp) p = *dp;
    else oslam_detect_params_default(&p);
    maxi = p.instances.max_instances;
    if (oslam_instance_params_check(&p.instances, maxi) != OSLAM_OK)
        return fail(OSLAM_E_INVALID, "instance parameters out of range");
    rc = oslam_refine_check_params(&p.refine, &rp);
    if (rc == OSLAM_OK) rc = oslam_verify_check_params(&p.verify, &vp);
    if (rc == OSLAM_OK) rc = oslam_arbitrate_check_params(&p.arbitrate, &ap);
    if (rc != OSLAM_OK) return rc;
    if (db->n == 0) return OSLAM_OK;
    for (j = 0; j < db->n; j++) {
        rc = oslam_view_check_pair(db->models[j], v);
        if (rc != OSLAM_OK) return rc;
    }
    inst = (oslam_instance *)malloc(sizeof *inst * db->n * maxi);
    n_inst = (size_t *)calloc(db->n, sizeof *n_inst);
    if (!inst || !n_inst) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    rc = oslam_db_align_instances(db, s, &p.instances, &rp, inst, maxi, n_inst, NULL);
    if (rc != OSLAM_OK) goto done;
    for (j = 0; j < db->n; j++) total += n_inst[j];
    if (total == 0) goto done;
    if (total > OSLAM_ARBITRATE_MAX_HYPOTHESES) {
        rc = fail(OSLAM_E_LIMIT, "more instances in the frame than one arbitration takes");
        goto done;
    }
    ms = (oslam_model **)malloc(sizeof *ms * total);
    slot = (size_t *)malloc(sizeof *slot * 2 * total);
    T = (float *)malloc(sizeof(float) * 16 * total);
    Tz = (float *)calloc(16 * total, sizeof(float));
    vres = (oslam_verify_result *)malloc(sizeof *vres * total);
    ares = (oslam_arbitrate_result *)calloc(total, sizeof *ares);
    if (!ms || !slot || !T || !Tz || !vres || !ares) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    for (j = 0; j < db->n; j++)
        for (k = 0; k < n_inst[j]; k++, at++) {
            ms[at] = db->models[j];
            slot[2 * at] = j;
            slot[2 * at + 1] = k;
            memcpy(T + 16 * at, inst[j * maxi + k].T, 16 * sizeof(float));
            rc = oslam_refine_check_rigid(T + 16 * at);
            if (rc != OSLAM_OK) goto done;
        }
    rc = oslam_verify_members(ms, total, v, T, &vp, vres);
    if (rc != OSLAM_OK) goto done;
    for (at = 0; at < total; at++)
        if (vres[at].found) {
            memcpy(Tz + 16 * at, T + 16 * at, 16 * sizeof(float));
            any = 1;
        }
    if (!any) goto done;
    rc = arbitrate_members(ms, total, v, Tz, &ap, ares, NULL, NULL, 0, NULL, NULL);
    if (rc != OSLAM_OK) goto done;
    for (at = 0; at < total; at++) kept += vres[at].found && ares[at].kept;
    *n_out = kept;
    if (kept > cap) { rc = fail(OSLAM_E_LIMIT, "more detections than out holds"); goto done; }
    for (at = 0, kept = 0; at < total; at++) {
        oslam_detection *o;
        if (!(vres[at].found && ares[at].kept)) continue;
        o = &out[kept++];
        memset(o, 0, sizeof *o);
        o->model = (uint32_t)slot[2 * at];
        o->instance = (uint32_t)slot[2 * at + 1];
        memcpy(o->T, T + 16 * at, sizeof o->T);
        o->verify = vres[at];
        o->arbitrate = ares[at];
    }
done:
    free(inst);
    free(n_inst);
    free(ms);
    free(slot);
    free(T);
    free(Tz);
    free(vres);
    free(ares);
    return rc;
}
