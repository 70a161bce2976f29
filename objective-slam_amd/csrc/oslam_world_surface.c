/*
 * oslam_world_surface.c -- the surface of the whole map, voxel store plus window (include/oslam.h at
 * oslam_world_surface): the host side of the kernels in oslam_world_surface.hip, and the map on the device that the mesh
 * of the whole map (oslam_world_mesh.c) extracts from too (oslam_world_map_open).  A call unites the store's brick keys
 * (oslam_world.c) with the keys of the bricks the window's box overlaps into one ascending table, sends the table and the
 * store's bricks up in one copy from the store's pinned buffer, lets the device write the window's words into their
 * bricks, counts, waits for the totals, allocates exactly that and emits, under the volume lock and the store's.
 */
#include "oslam_internal.h"
#include "oslam_window.h"
#include "oslam_world.h"

int oslam_world_surface_params_default(oslam_world_surface_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->min_weight = 1;
    return OSLAM_OK;
}

int oslam_world_surface_check_params(const oslam_world_surface_params *sp, oslam_world_surface_params *out)
{
    if (sp) *out = *sp; else oslam_world_surface_params_default(out);
    if (out->min_weight < 1 || out->min_weight > 65535) return fail(OSLAM_E_INVALID, "min_weight must lie in 1..65535");
    if (out->anchor_set && !oslamk_shift_ok(out->anchor)) return fail(OSLAM_E_INVALID, "an anchor is at most 2^20 voxels");
    return OSLAM_OK;
}

int oslam_world_map_open(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *p, int plane, void *stream,
                         oslam_world_map *o)
{
    int rc = OSLAM_OK, a, kb0[3] = {0, 0, 0}, nb[3] = {0, 0, 0}, launched = 0;
    float voxel, origin0[3];
    int32_t *skeys = NULL;
    uint8_t *d_map = NULL;
    size_t ns, nw = 0, n = 0, i, j, off_slots, off_words;
    oslamk_brick_map m;
    oslamk_volume kv;
    oslam_world_stage *st;
    memset(o, 0, sizeof *o);
    memset(&m, 0, sizeof m);
    oslam_world_frame(w, &voxel, origin0);
    if (vol && !oslam_world_compatible(w, vol->p.voxel, vol->p.origin)) {
        rc = fail(OSLAM_E_INVALID, "the voxel store was made for another voxel size or origin");
        goto done;
    }
    for (a = 0; a < 3; a++) {
        m.anchor[a] = p->anchor_set ? p->anchor[a] : vol ? vol->off[a] : 0;
        o->anchor[a] = m.anchor[a];
    }
    oslam_window_origin(origin0, voxel, m.anchor, m.origin);        /* oslam_volume_shift's origin of an offset */
    m.voxel = voxel;
    m.inv_voxel = 1.0f / voxel;
    /* the table: the store's keys and the window's, both ascending, united; a store brick's slot is its rank among the
     * store's, a window-only brick's follows them */
    ns = oslam_world_brick_count(w);
    if (vol) {
        const unsigned sides[3] = {vol->p.nx, vol->p.ny, vol->p.nz};
        oslam_window_bricks(sides, vol->off, kb0, nb);
        nw = (size_t)nb[0] * (size_t)nb[1] * (size_t)nb[2];
    }
    o->window_bricks = (uint32_t)nw;
    if (ns + nw == 0) goto done;                                    /* an empty map: no device call */
    if (ns > OSLAMK_BRICK_MAX || ns + nw > OSLAMK_BRICK_MAX) { rc = fail(OSLAM_E_LIMIT, "a map holds at most 2^22 bricks"); goto done; }
    if (vol) o->dev = vol->dev;
    else {
        rc = oslam_pick_device(p->dev, &o->dev);
        if (rc != OSLAM_OK) goto done;
    }
    if (hipSetDevice(o->dev) != hipSuccess) { rc = fail(OSLAM_E_DEVICE, "hipSetDevice failed"); goto done; }
    skeys = (int32_t *)malloc(sizeof(int32_t) * 3 * (ns ? ns : 1));
    if (!skeys) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    oslam_world_brick_keys(w, skeys);
    /* one pinned block laid out as the device's: keys [n], slots [n], then the store's bricks; n is not known before the
     * merge, so the offsets are those of the largest table */
    off_slots = align256(sizeof(uint64_t) * (ns + nw));
    off_words = off_slots + align256(sizeof(uint32_t) * (ns + nw));
    st = oslam_world_stages(w);
    rc = oslam_world_stage_fit(&st[1], off_words + sizeof(uint32_t) * OSLAMK_BRICK_WORDS * ns);
    if (rc != OSLAM_OK) goto done;
    {
        uint64_t *hk = (uint64_t *)st[1].p;
        uint32_t *hs = (uint32_t *)((uint8_t *)st[1].p + off_slots), *hw = (uint32_t *)((uint8_t *)st[1].p + off_words);
        int wb[3] = {0, 0, 0};                                      /* the window brick the merge stands at */
        size_t only = 0;
        i = j = 0;
        while (i < ns || j < nw) {
            const uint64_t ks = i < ns ? OSLAMK_BRICK_KEY(skeys[3 * i], skeys[3 * i + 1], skeys[3 * i + 2]) : UINT64_MAX;
            const uint64_t kw = j < nw ? OSLAMK_BRICK_KEY(kb0[0] + wb[0], kb0[1] + wb[1], kb0[2] + wb[2]) : UINT64_MAX;
            if (ks <= kw) {
                hk[n] = ks;
                hs[n] = (uint32_t)i;
                memcpy(hw + OSLAMK_BRICK_WORDS * i,
                       plane == OSLAM_MAP_COLOUR ? oslam_world_brick_colours(w, skeys + 3 * i) : oslam_world_brick_words(w, skeys + 3 * i),
                       sizeof(uint32_t) * OSLAMK_BRICK_WORDS);
                i++;
            } else {
                hk[n] = kw;
                hs[n] = (uint32_t)(ns + only++);
            }
            if (kw <= ks) {                                         /* the window's next brick, x fastest */
                j++;
                if (++wb[0] == nb[0]) {
                    wb[0] = 0;
                    if (++wb[1] == nb[1]) { wb[1] = 0; wb[2]++; }
                }
            }
            n++;
        }
        /* the device block: the same layout, then the window-only bricks, zeroed */
        KCHK(oslam_dev_alloc((void **)&d_map, off_words + sizeof(uint32_t) * OSLAMK_BRICK_WORDS * n));
        HIPCHK(hipMemcpyAsync(d_map, st[1].p, off_words + sizeof(uint32_t) * OSLAMK_BRICK_WORDS * ns, hipMemcpyHostToDevice,
                              (hipStream_t)stream));
        launched = 1;
        if (n > ns)
            HIPCHK(hipMemsetAsync(d_map + off_words + sizeof(uint32_t) * OSLAMK_BRICK_WORDS * ns, 0,
                                  sizeof(uint32_t) * OSLAMK_BRICK_WORDS * (n - ns), (hipStream_t)stream));
    }
    m.keys = (const uint64_t *)d_map;
    m.slots = (const uint32_t *)(d_map + off_slots);
    m.words = (uint32_t *)(d_map + off_words);
    m.n = (uint32_t)n;
    if (nw) {
        kv = vol->k;                                                /* the kernel copies words whatever they mean */
        if (plane == OSLAM_MAP_COLOUR) kv.words = vol->colour.words;
        KCHK(oslamk_brick_window(&m, &kv, vol->off, kb0, nb, stream));
        o->launches++;
    }
    o->m = m;
    o->d_map = d_map;
    o->bricks = (uint32_t)n;
done:
    if (rc != OSLAM_OK) {
        if (launched) (void)hipStreamSynchronize((hipStream_t)stream);
        if (d_map) oslam_dev_free(d_map);
    }
    free(skeys);
    return rc;
}

void oslam_world_map_close(oslam_world_map *o)
{
    if (o->d_map) oslam_dev_free(o->d_map);
    o->d_map = NULL;
}

/* what one extraction leaves: the device blocks (NULL without points, or when they were not asked for) and the figures */
typedef struct world_run {
    float *d_out6;
    int32_t *d_key;
    uint32_t crossings, points, bricks, window_bricks, launches;
    int32_t anchor[3];
    int dev;
} world_run;

/* The extraction after the argument checks.  cap: the most points the caller takes; with_out 0 only counts; with_keys:
 * the points' keys too.  p is checked.  Both locks are taken here and every device block but the outputs is freed */
static int world_surface_run(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *p, size_t cap, int with_out,
                             int with_keys, world_run *o)
{
    int rc = OSLAM_OK, launched = 0;
    uint32_t *d_cnt = NULL, tot[64];
    size_t n, c;
    oslam_world_map wm;
    oslamk_brick_bases bases;
    void *stream = oslam_stream();
    memset(o, 0, sizeof *o);
    memset(&bases, 0, sizeof bases);
    oslam_volume_lock();
    oslam_world_lock(w);
    rc = oslam_world_map_open(w, vol, p, OSLAM_MAP_TSDF, stream, &wm);
    memcpy(o->anchor, wm.anchor, sizeof o->anchor);
    o->window_bricks = wm.window_bricks;
    o->bricks = wm.bricks;
    o->launches = wm.launches;
    o->dev = wm.dev;
    n = wm.bricks;
    if (rc != OSLAM_OK || n == 0) goto done;                        /* an empty map: no points, no device call */
    launched = 1;
    KCHK(oslam_counters_open(&d_cnt, n, stream));
    KCHK(oslamk_brick_count(&wm.m, p->min_weight, d_cnt + 64, d_cnt, stream));
    o->launches += 1 + (uint32_t)((n + OSLAMK_BRICK_SCAN - 1) / OSLAMK_BRICK_SCAN);
    HIPCHK(hipMemcpyAsync(tot, d_cnt, sizeof tot, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    o->crossings = tot[0];
    {
        uint64_t sum = 0;
        for (c = 0; c * OSLAMK_BRICK_SCAN < n; c++) {
            bases.base[c] = (uint32_t)sum;
            sum += tot[2 + c];
        }
        if (sum > UINT32_MAX) { rc = fail(OSLAM_E_LIMIT, "the map's surface has more than 2^32 points"); goto done; }
        o->points = (uint32_t)sum;
    }
    if (with_out && o->points > 0 && (size_t)o->points <= cap) {
        KCHK(oslam_dev_alloc((void **)&o->d_out6, sizeof(float) * 6 * (size_t)o->points));
        if (with_keys) KCHK(oslam_dev_alloc((void **)&o->d_key, sizeof(int32_t) * 4 * (size_t)o->points));
        KCHK(oslamk_brick_emit(&wm.m, p->min_weight, d_cnt + 64, &bases, o->points, o->d_out6, o->d_key, stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        o->launches++;
    }
done:
    if (rc != OSLAM_OK) {
        if (launched) (void)hipStreamSynchronize((hipStream_t)stream);
        if (o->d_out6) { oslam_dev_free(o->d_out6); o->d_out6 = NULL; }
        if (o->d_key) { oslam_dev_free(o->d_key); o->d_key = NULL; }
    }
    oslam_world_unlock(w);
    oslam_volume_unlock();
    if (d_cnt) oslam_dev_free(d_cnt);
    oslam_world_map_close(&wm);
    return rc;
}

int oslam_world_surface(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, float *xyz_out, float *nrm_out,
                        int32_t *key_out, size_t cap, size_t *n_out, oslam_world_surface_result *res)
{
    int rc;
    const double t0 = now_ms();
    oslam_world_surface_params p;
    world_run o;
    float *h_out = NULL;
    if (!w || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!xyz_out != !nrm_out) return fail(OSLAM_E_INVALID, "xyz_out and nrm_out must both be given or both be NULL");
    if (!xyz_out && (cap != 0 || key_out)) return fail(OSLAM_E_INVALID, "cap must be 0 and key_out NULL without outputs");
    rc = oslam_world_surface_check_params(sp, &p);
    if (rc != OSLAM_OK) return rc;
    *n_out = 0;
    if (res) memset(res, 0, sizeof *res);
    rc = world_surface_run(w, vol, &p, cap, xyz_out != NULL, key_out != NULL, &o);
    if (rc != OSLAM_OK) return rc;
    *n_out = o.points;
    if (xyz_out && (size_t)o.points > cap) rc = fail(OSLAM_E_LIMIT, "output capacity too small");
    if (o.d_out6) {
        const size_t np = o.points;
        h_out = (float *)malloc(sizeof(float) * 6 * np);
        if (!h_out) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        HIPCHK(hipMemcpy(h_out, o.d_out6, sizeof(float) * 6 * np, hipMemcpyDeviceToHost));
        if (o.d_key) HIPCHK(hipMemcpy(key_out, o.d_key, sizeof(int32_t) * 4 * np, hipMemcpyDeviceToHost));
        split_points(h_out, np, xyz_out, nrm_out);
    }
done:
    free(h_out);
    if (o.d_out6) oslam_dev_free(o.d_out6);
    if (o.d_key) oslam_dev_free(o.d_key);
    if ((rc == OSLAM_OK || rc == OSLAM_E_LIMIT) && res) {
        res->crossings = o.crossings;
        res->points = o.points;
        res->bricks = o.bricks;
        res->window_bricks = o.window_bricks;
        res->launches = o.launches;
        memcpy(res->anchor, o.anchor, sizeof o.anchor);
        res->ms_total = (float)(now_ms() - t0);
    }
    return rc;
}

int oslam_world_surface_cloud(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *p, int *dev, float **d_pts6,
                              uint32_t *np)
{
    world_run o;
    const int rc = world_surface_run(w, vol, p, (size_t)-1, 1, 0, &o);
    *d_pts6 = rc == OSLAM_OK ? o.d_out6 : NULL;
    *np = rc == OSLAM_OK ? o.points : 0;
    if (rc == OSLAM_OK && o.bricks) *dev = o.dev;
    return rc;
}
