/*
 * oslam_explain.c -- hypotheses judged against their own z-buffers and arbitrated by their conflict rates
 * (include/oslam.h at oslam_explain): the host side of the kernels in oslam_explain.hip.  A call checks its arguments,
 * resolves the tile, gives every hypothesis a rectangle of the image that holds whatever it can draw (oslam_explain_rect,
 * from the model's bounding sphere) and lays the rectangles out in one pool by a prefix sum.  It uploads one block (the
 * descriptors of the verification stage, the splat radii, the rectangles and the zeroed records), zeroes the claims
 * table, presets the pool to all ones, runs k_explain_splat, k_explain_score, k_explain_claims and k_arbitrate back to
 * back and reads the records of both stages back with one copy and one host wait.
 */
#include <math.h>

#include "oslam_internal.h"

#define EXPLAIN_MAX_TABLE_BYTES ((size_t)256 << 20)
#define EXPLAIN_MAX_POOL_BYTES ((size_t)256 << 20)

enum { EXPLAIN_ALL, EXPLAIN_TAP_Z, EXPLAIN_TAP_CLAIMS };

int oslam_explain_params_default(oslam_explain_params *p)
{
    oslam_render_params rp;
    oslam_arbitrate_params ap;
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    oslam_render_params_default(&rp);
    oslam_arbitrate_params_default(&ap);
    p->footprint = rp.footprint;
    p->max_splat = rp.max_splat;
    p->keep_back = rp.keep_back;
    p->depth_tol = 1.0f;
    p->tile = ap.tile;
    p->tile_spacing = ap.tile_spacing;
    p->min_tiles = ap.min_tiles;
    p->min_owned_share = 0.52f;
    return OSLAM_OK;
}

/* the checks of the render and of the arbitration for the fields explain shares with them */
static int explain_check_params(const oslam_explain_params *ep, oslam_explain_params *out, oslam_arbitrate_params *ap)
{
    oslam_render_params rp, rq;
    int rc;
    if (ep) *out = *ep;
    else oslam_explain_params_default(out);
    oslam_render_params_default(&rp);
    rp.footprint = out->footprint;
    rp.max_splat = out->max_splat;
    rp.keep_back = out->keep_back;
    rp.depth_tol = out->depth_tol;
    rc = oslam_render_check_params(&rp, &rq);
    if (rc != OSLAM_OK) return rc;
    oslam_arbitrate_params_default(ap);
    ap->depth_tol = out->depth_tol;
    ap->tile = out->tile;
    ap->tile_spacing = out->tile_spacing;
    ap->min_tiles = out->min_tiles;
    ap->min_owned_share = out->min_owned_share;
    return oslam_arbitrate_check_params(ap, ap);
}

/* clip a pixel coordinate given as a double to [0, n] before it becomes an int */
static int clip_px(double x, int n) { return !(x > 0.0) ? 0 : x > (double)n ? n : (int)x; }

/* The rectangle of include/oslam.h ("Rectangle"), arguments checked: rect = x0, y0, w, h. */
static void explain_rect(const double centre[3], double radius, const float T[16], const oslam_camera *cam, int width,
                         int height, unsigned max_splat, int rect[4])
{
    const double pad = (double)max_splat + 2.0;
    double A[12], c[3], e2 = 0.0, r, zlo, zhi, lo[2], hi[2];
    int a, b, k, x0, x1, y0, y1;
    rect[0] = rect[1] = rect[2] = rect[3] = 0;
    for (a = 0; a < 12; a++) A[a] = (double)T[a];
    oslam_rigid_apply(A, centre, c);
    /* |R d| <= sqrt(1 + |R^T R - I|_F) |d|: a pose passes the rigid test with a rotation that is orthonormal to 1e-3 only */
    for (a = 0; a < 3; a++)
        for (b = 0; b < 3; b++) {
            const double g = ((A[a] * A[b] + A[4 + a] * A[4 + b]) + A[8 + a] * A[8 + b]) - (a == b ? 1.0 : 0.0);
            e2 += g * g;
        }
    /* and the device transforms in float32: a relative 1e-6 of everything that enters the sum */
    r = radius * sqrt(1.0 + sqrt(e2)) * (1.0 + 1e-6) + 1e-6 * (((fabs(c[0]) + fabs(c[1])) + fabs(c[2])) + radius);
    zlo = c[2] - r;
    zhi = c[2] + r;
    if (zhi < (double)cam->z_min || zlo > (double)cam->z_max) return;    /* every point is OUT */
    if (!(zlo > 0.0)) {                          /* the sphere reaches the camera's plane: no bound on the projection */
        rect[2] = width;
        rect[3] = height;
        return;
    }
    for (k = 0; k < 2; k++) {
        const double f = k ? (double)cam->fy : (double)cam->fx, o = k ? (double)cam->cy : (double)cam->cx;
        const double xl = c[k] - r, xh = c[k] + r;
        const double p[4] = {f * xl / zlo + o, f * xl / zhi + o, f * xh / zlo + o, f * xh / zhi + o};
        lo[k] = hi[k] = p[0];
        for (a = 1; a < 4; a++) {
            if (p[a] < lo[k]) lo[k] = p[a];
            if (p[a] > hi[k]) hi[k] = p[a];
        }
    }
    x0 = clip_px(floor(lo[0]) - pad, width);
    x1 = clip_px(ceil(hi[0]) + pad + 1.0, width);       /* one past the last column */
    y0 = clip_px(floor(lo[1]) - pad, height);
    y1 = clip_px(ceil(hi[1]) + pad + 1.0, height);
    if (x1 <= x0 || y1 <= y0) return;
    rect[0] = x0;
    rect[1] = y0;
    rect[2] = x1 - x0;
    rect[3] = y1 - y0;
}

int oslam_explain_rect(const double centre[3], double radius, const float T[16], const oslam_camera *cam, int width,
                       int height, unsigned max_splat, int rect_out[4])
{
    int rc;
    if (!centre || !T || !cam || !rect_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rect_out[0] = rect_out[1] = rect_out[2] = rect_out[3] = 0;
    if (!isfinite(centre[0]) || !isfinite(centre[1]) || !isfinite(centre[2]) || !isfinite(radius) || radius < 0.0)
        return fail(OSLAM_E_INVALID, "the bounding sphere must be finite with a radius >= 0");
    if (max_splat > OSLAM_RENDER_MAX_SPLAT) return fail(OSLAM_E_INVALID, "max_splat above OSLAM_RENDER_MAX_SPLAT");
    if (!oslam_view_camera_ok(cam, width, height, 1, 1)) return fail(OSLAM_E_INVALID, "bad camera or size");
    if (oslam_is_zero_pose(T)) return OSLAM_OK;  /* a skipped hypothesis draws nothing */
    rc = oslam_refine_check_rigid(T);
    if (rc != OSLAM_OK) return rc;
    explain_rect(centre, radius, T, cam, width, height, max_splat, rect_out);
    return OSLAM_OK;
}

/* the largest distance of a model point from the model's double mean: once per model, from the host copy of the cloud */
static double model_radius(oslam_model *m)
{
    if (!m->bound_set) {
        double r2 = 0.0;
        size_t i;
        for (i = 0; i < (size_t)m->c.n; i++) {
            const double dx = (double)m->c.h_xyz[3 * i] - m->cm[0], dy = (double)m->c.h_xyz[3 * i + 1] - m->cm[1],
                         dz = (double)m->c.h_xyz[3 * i + 2] - m->cm[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 > r2) r2 = d2;
        }
        m->bound_r = sqrt(r2) * (1.0 + 1e-12);
        m->bound_set = 1;
    }
    return m->bound_r;
}

/* Hypotheses ms[0 .. H) with T [H][16] (all-zero = skipped) against v, every argument and handle checked.
 * EXPLAIN_ALL: res [H].  EXPLAIN_TAP_Z: z_out [w * h] = the solo z image of hypothesis tap_h.  EXPLAIN_TAP_CLAIMS:
 * cnt_out / sum_out = the table after k_explain_claims, H * n_tiles entries each (cap: what they hold). */
static int explain_members(oslam_model *const *ms, size_t H, const oslam_view *v, const float *T,
                           const oslam_explain_params *p, const oslam_arbitrate_params *ap, int mode,
                           oslam_explain_result *res, size_t tap_h, float *z_out, uint32_t *cnt_out, uint64_t *sum_out,
                           size_t cap, uint32_t *tile_out, size_t *n_tiles_out)
{
    int rc = OSLAM_OK, max_w = 0, max_h = 0;
    const double t0 = now_ms();
    const int width = v->k.w, height = v->k.h;
    size_t h, e, max_blocks = 0, off_rho, off_rect, off_arb, off_rec, off_tbl, off_pool, up_bytes, n_ent, tbl_bytes,
           pool_words = 0;
    char *up = NULL, *dev = NULL;
    oslamk_verify_member *hm;
    oslamk_explain_rect *rect;
    oslamk_explain_rec *rec;
    oslamk_arb_rec *arb;
    float *rho;
    void *back = NULL;
    oslamk_arb_grid g;
    oslam_camera cam;
    uint32_t launches = 0, rounds = 0;
    void *stream = oslam_stream();

    if (res) memset(res, 0, sizeof *res * H);
    g.tile = oslam_arbitrate_choose_tile(ms, T, H, v, ap);
    g.tiles_x = (width + g.tile - 1) / g.tile;
    g.n_tiles = (uint32_t)g.tiles_x * (uint32_t)((height + g.tile - 1) / g.tile);
    n_ent = H * (size_t)g.n_tiles;
    tbl_bytes = n_ent * sizeof(uint64_t);
    if (tile_out) *tile_out = (uint32_t)g.tile;
    if (n_tiles_out) *n_tiles_out = g.n_tiles;
    if (tbl_bytes > EXPLAIN_MAX_TABLE_BYTES) return fail(OSLAM_E_LIMIT, "the claims table (hypotheses x tiles x 8 B) exceeds 256 MiB");
    if (mode == EXPLAIN_TAP_CLAIMS && n_ent > cap) return fail(OSLAM_E_INVALID, "the claims arrays are too short for hypotheses x tiles");

    off_rho = align256(sizeof *hm * H);
    off_rect = off_rho + align256(sizeof(float) * H);
    off_arb = off_rect + align256(sizeof *rect * H);
    off_rec = off_arb + align256(sizeof *arb * (1 + H));
    up_bytes = off_rec + align256(sizeof *rec * H);
    off_tbl = up_bytes;
    off_pool = off_tbl + align256(tbl_bytes);
    up = (char *)calloc(1, up_bytes);
    if (!up) return fail(OSLAM_E_NOMEM, "host allocation failed");
    hm = (oslamk_verify_member *)up;
    rho = (float *)(up + off_rho);
    rect = (oslamk_explain_rect *)(up + off_rect);
    arb = (oslamk_arb_rec *)(up + off_arb);
    rec = (oslamk_explain_rec *)(up + off_rec);
    oslam_view_camera(v, &cam);
    for (h = 0; h < H; h++) {
        int r4[4];
        if (oslam_is_zero_pose(T + 16 * h)) continue;
        oslam_verify_set_member(&hm[h], ms[h], T + 16 * h, p->depth_tol);
        rho[h] = (float)((double)p->footprint * (double)ms[h]->d_dist);
        if (hm[h].n_blocks > max_blocks) max_blocks = hm[h].n_blocks;
        explain_rect(ms[h]->cm, model_radius(ms[h]), T + 16 * h, &cam, width, height, p->max_splat, r4);
        rect[h].x0 = r4[0];
        rect[h].y0 = r4[1];
        rect[h].w = r4[2];
        rect[h].h = r4[3];
        rect[h].off = pool_words;
        pool_words += (size_t)r4[2] * (size_t)r4[3];
        if (r4[2] > max_w) max_w = r4[2];
        if (r4[3] > max_h) max_h = r4[3];
        if (pool_words * sizeof(uint32_t) > EXPLAIN_MAX_POOL_BYTES) {
            rc = fail(OSLAM_E_LIMIT, "the hypotheses' z-buffers exceed 256 MiB in total");
            goto done;
        }
    }
    if (res)
        for (h = 0; h < H; h++) res[h].tile = (uint32_t)g.tile;
    if (max_blocks == 0) {                      /* every hypothesis skipped: no device work */
        if (mode == EXPLAIN_TAP_Z) memset(z_out, 0, sizeof(float) * (size_t)width * (size_t)height);
        if (mode == EXPLAIN_TAP_CLAIMS) {
            memset(cnt_out, 0, sizeof *cnt_out * n_ent);
            memset(sum_out, 0, sizeof *sum_out * n_ent);
        }
        goto finish;
    }
    if (hipSetDevice(v->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    KCHK(oslam_dev_alloc((void **)&dev, off_pool + align256(pool_words * sizeof(uint32_t))));
    HIPCHK(hipMemcpyAsync(dev, up, up_bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipMemsetAsync(dev + off_tbl, 0, align256(tbl_bytes), (hipStream_t)stream));
    if (pool_words) HIPCHK(hipMemsetAsync(dev + off_pool, 0xff, pool_words * sizeof(uint32_t), (hipStream_t)stream));
    KCHK(oslamk_explain_splat(&v->k, (const oslamk_verify_member *)dev, (const float *)(dev + off_rho),
                              (const oslamk_explain_rect *)(dev + off_rect), (uint32_t)H, (uint32_t)max_blocks,
                              (int)p->max_splat, p->keep_back, (uint32_t *)(dev + off_pool),
                              (oslamk_explain_rec *)(dev + off_rec), stream));
    launches++;
    if (mode == EXPLAIN_TAP_Z) {
        const oslamk_explain_rect *r = &rect[tap_h];
        const size_t nw = (size_t)r->w * (size_t)r->h;
        uint32_t *zb;
        int x, y;
        memset(z_out, 0, sizeof(float) * (size_t)width * (size_t)height);
        back = malloc(sizeof *rec * H + sizeof(uint32_t) * (nw ? nw : 1));
        if (!back) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        zb = (uint32_t *)((char *)back + sizeof *rec * H);
        HIPCHK(hipMemcpyAsync(back, dev + off_rec, sizeof *rec * H, hipMemcpyDeviceToHost, (hipStream_t)stream));
        if (nw)
            HIPCHK(hipMemcpyAsync(zb, dev + off_pool + sizeof(uint32_t) * (size_t)r->off, sizeof(uint32_t) * nw,
                                  hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        for (h = 0; h < H; h++)
            if (((const oslamk_explain_rec *)back)[h].clipped) {
                rc = fail(OSLAM_E_DEVICE, "a splat left its hypothesis's rectangle (explain)");
                goto done;
            }
        for (y = 0; y < r->h; y++)
            for (x = 0; x < r->w; x++) {
                const uint32_t b = zb[(size_t)y * (size_t)r->w + (size_t)x];
                if (b != 0xffffffffu) memcpy(&z_out[(size_t)(r->y0 + y) * (size_t)width + (size_t)(r->x0 + x)], &b, sizeof b);
            }
        goto finish;
    }
    KCHK(oslamk_explain_score(&v->k, (const oslamk_verify_member *)dev, (const oslamk_explain_rect *)(dev + off_rect),
                              (uint32_t)H, max_w, max_h, (const uint32_t *)(dev + off_pool), g,
                              (unsigned long long *)(dev + off_tbl), (oslamk_explain_rec *)(dev + off_rec), stream));
    launches++;
    KCHK(oslamk_explain_claims((const oslamk_explain_rec *)(dev + off_rec), (uint32_t)H, g.n_tiles,
                               (unsigned long long *)(dev + off_tbl), stream));
    launches++;
    if (mode == EXPLAIN_TAP_CLAIMS) {
        uint64_t *tb;
        back = malloc(sizeof *rec * H + tbl_bytes);
        if (!back) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        tb = (uint64_t *)((char *)back + sizeof *rec * H);
        HIPCHK(hipMemcpyAsync(back, dev + off_rec, sizeof *rec * H, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipMemcpyAsync(tb, dev + off_tbl, tbl_bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        for (h = 0; h < H; h++)
            if (((const oslamk_explain_rec *)back)[h].clipped) {
                rc = fail(OSLAM_E_DEVICE, "a splat left its hypothesis's rectangle (explain)");
                goto done;
            }
        for (e = 0; e < n_ent; e++) {
            cnt_out[e] = (uint32_t)(tb[e] >> OSLAMK_ARB_CNT_SHIFT);
            sum_out[e] = tb[e] & (((uint64_t)1 << OSLAMK_ARB_CNT_SHIFT) - 1);
        }
        goto finish;
    }
    KCHK(oslamk_arbitrate((const oslamk_verify_member *)dev, (uint32_t)H, g.n_tiles,
                          (const unsigned long long *)(dev + off_tbl), p->min_tiles, p->min_owned_share,
                          (oslamk_arb_rec *)(dev + off_arb), stream));
    launches++;
    /* both stages' records lie side by side: one copy, into the block that was uploaded */
    HIPCHK(hipMemcpyAsync(up + off_arb, dev + off_arb, up_bytes - off_arb, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    rounds = arb[0].claimed;
    for (h = 0; h < H; h++) {
        const oslamk_explain_rec *k = &rec[h];
        const oslamk_arb_rec *a = &arb[1 + h];
        oslam_explain_result *r = &res[h];
        const uint64_t at = (uint64_t)k->agree + k->through, aot = at + k->occluded;
        if (k->clipped) { rc = fail(OSLAM_E_DEVICE, "a splat left its hypothesis's rectangle (explain)"); goto done; }
        if (hm[h].n_blocks == 0) continue;
        r->drawn = k->drawn;
        r->agree = k->agree;
        r->occluded = k->occluded;
        r->through = k->through;
        r->unknown = k->unknown;
        r->pixels = ((k->agree + k->occluded) + k->through) + k->unknown;
        r->resid_sum = k->resid_sum;
        r->explained = at ? (float)k->agree / (float)at : 0.0f;
        r->visible = aot ? (float)k->agree / (float)aot : 0.0f;
        r->mean_residual = k->agree ? (float)((((double)k->resid_sum / (double)k->agree) / 65535.0) * (double)hm[h].tol) : 0.0f;
        r->conflict_q = k->agree ? (uint32_t)((65535 * (uint64_t)k->through) / at) : 0u;
        r->claimed = a->claimed;
        r->owned = a->owned;
        r->share = a->share;
        r->kept = a->kept;
        r->suppressed_by = a->suppressed_by;
    }
finish:
    if (res) {
        const float ms_total = (float)(now_ms() - t0);
        for (h = 0; h < H; h++) {
            if (hm[h].n_blocks == 0) res[h].suppressed_by = -1;
            res[h].rounds = rounds;
            res[h].launches = launches;
            res[h].ms_total = ms_total;
        }
    }
done:
    if (rc != OSLAM_OK && dev) (void)hipStreamSynchronize((hipStream_t)stream);    /* nothing may still use the block */
    if (dev) oslam_dev_free(dev);
    free(back);
    free(up);
    return rc;
}

/* both halves of the argument checks; *p and *ap: the parameters in force */
static int explain_check(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                         const oslam_explain_params *ep, oslam_explain_params *p, oslam_arbitrate_params *ap)
{
    int rc = explain_check_params(ep, p, ap);
    if (rc == OSLAM_OK) rc = oslam_check_poses(models, T, H, 1);
    if (rc == OSLAM_OK) rc = oslam_check_handles(models, T, H, v);
    return rc;
}

int oslam_explain(oslam_model *const *models, const float *T, size_t H, const oslam_view *v, const oslam_explain_params *ep,
                  oslam_explain_result *res)
{
    oslam_explain_params p;
    oslam_arbitrate_params ap;
    int rc;
    if (!models || !T || !v || !res) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = explain_check(models, T, H, v, ep, &p, &ap);
    if (rc != OSLAM_OK) return rc;
    return explain_members(models, H, v, T, &p, &ap, EXPLAIN_ALL, res, 0, NULL, NULL, NULL, 0, NULL, NULL);
}

int oslam_db_explain(oslam_db *db, const oslam_view *v, const float *T, const oslam_explain_params *ep,
                     oslam_explain_result *res)
{
    oslam_explain_params p;
    oslam_arbitrate_params ap;
    int rc;
    if (!db || !v || !T || !res) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = explain_check_params(ep, &p, &ap);
    if (rc != OSLAM_OK) return rc;
    if (db->n && !db->models) return fail(OSLAM_E_INVALID, "the database holds no models");
    rc = oslam_check_poses(db->models, T, db->n, 1);
    if (rc == OSLAM_OK) rc = oslam_check_handles(db->models, T, db->n, v);
    if (rc != OSLAM_OK) return rc;
    return explain_members(db->models, db->n, v, T, &p, &ap, EXPLAIN_ALL, res, 0, NULL, NULL, NULL, 0, NULL, NULL);
}

int oslam_explain_z(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                    const oslam_explain_params *ep, size_t h, float *z_out)
{
    oslam_explain_params p;
    oslam_arbitrate_params ap;
    int rc;
    if (!models || !T || !v || !z_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = explain_check_params(ep, &p, &ap);
    if (rc == OSLAM_OK) rc = oslam_check_poses(models, T, H, 1);
    if (rc == OSLAM_OK && h >= H) rc = fail(OSLAM_E_INVALID, "h names no hypothesis of the call");
    if (rc == OSLAM_OK) rc = oslam_check_handles(models, T, H, v);
    if (rc != OSLAM_OK) return rc;
    return explain_members(models, H, v, T, &p, &ap, EXPLAIN_TAP_Z, NULL, h, z_out, NULL, NULL, 0, NULL, NULL);
}

int oslam_explain_claims(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                         const oslam_explain_params *ep, uint32_t *cnt_out, uint64_t *sum_out, size_t cap,
                         uint32_t *tile_out, size_t *n_tiles_out)
{
    oslam_explain_params p;
    oslam_arbitrate_params ap;
    int rc;
    if (!models || !T || !v || !cnt_out || !sum_out) return fail(OSLAM_E_INVALID, "NULL argument");
    rc = explain_check(models, T, H, v, ep, &p, &ap);
    if (rc != OSLAM_OK) return rc;
    return explain_members(models, H, v, T, &p, &ap, EXPLAIN_TAP_CLAIMS, NULL, 0, NULL, cnt_out, sum_out, cap, tile_out,
                           n_tiles_out);
}
