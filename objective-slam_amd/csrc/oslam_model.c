/*
 * oslam_model.c -- a model: its key tables built once and kept in HBM (model.cu), saved to and loaded from
 * a file, its point weights, and its cloud's shape (centroid and extent, made where the cloud is).
 */
#include <stdio.h>

#include "oslam_internal.h"
#include "oslam_pose.h"
#include "ppf_core.h"

void oslam_model_destroy(oslam_model *m)
{
    if (!m) return;
    (void)hipSetDevice(m->dev);
    oslam_cloud_free(&m->c);
    if (m->table.slots) (void)hipFree(m->table.slots);
    if (m->ent.e4) (void)hipFree(m->ent.e4);
    if (m->ent.uv) (void)hipFree(m->ent.uv);
    if (m->ent.pw) (void)hipFree(m->ent.pw);
    if (m->ent.puv) (void)hipFree(m->ent.puv);
    if (m->ent.pdir) (void)hipFree(m->ent.pdir);
    if (m->ent.mi) (void)hipFree(m->ent.mi);
    if (m->table.ukeys && !m->shared_union) (void)hipFree(m->table.ukeys);
    if (m->table.reach && !m->shared_union) (void)hipFree(m->table.reach);
    if (m->table.kmap && !m->shared_union) (void)hipFree(m->table.kmap);
    if (m->table.uids && !m->shared_union) (void)hipFree(m->table.uids);
    if (m->d_counters) (void)hipFree(m->d_counters);
    if (m->d_out) (void)hipFree(m->d_out);
    if (m->d_union) (void)hipFree(m->d_union);
    if (m->table.uinfo) (void)hipFree(m->table.uinfo);
    if (m->d_Tm16) (void)hipFree(m->d_Tm16);
    if (m->d_weights) (void)hipFree(m->d_weights);
    if (m->d_pose_cells) (void)hipFree(m->d_pose_cells);
    if (m->d_pose_T) (void)hipFree(m->d_pose_T);
    free(m->h_out);
    free(m->weights);
    free(m->last_cells);
    free(m->last_poses);
    free(m->h_slots);
    free(m);
}

/* one key of a union table, for the ranking below */
typedef struct key_rank {
    uint64_t weight;
    uint32_t key, slot;
} key_rank;

/* one stable pass of a radix sort over 16 bits of `weight` (descending) or of `key` (ascending); count: 65536 words */
static void rank_pass(const key_rank *src, key_rank *dst, size_t n, int by_weight, unsigned shift, uint32_t *count)
{
    size_t i;
    uint32_t run = 0, d;
    memset(count, 0, sizeof(uint32_t) * 65536);
    for (i = 0; i < n; i++) {
        d = by_weight ? 0xffffu - (uint32_t)((src[i].weight >> shift) & 0xffffu) : (src[i].key >> shift) & 0xffffu;
        count[d]++;
    }
    for (d = 0; d < 65536; d++) {
        const uint32_t c = count[d];
        count[d] = run;
        run += c;
    }
    for (i = 0; i < n; i++) {
        d = by_weight ? 0xffffu - (uint32_t)((src[i].weight >> shift) & 0xffffu) : (src[i].key >> shift) & 0xffffu;
        dst[count[d]++] = src[i];
    }
}

/* The numbers 0 .. n-1 of n keys, by descending weight, ties by ascending key: r[i].slot's number is i afterwards.
 * tmp [n], count [65536]; returns the array that holds the result (r or tmp). */
static key_rank *rank_keys(key_rank *r, key_rank *tmp, size_t n, uint32_t *count)
{
    uint64_t top = 0;
    unsigned shift;
    size_t i;
    key_rank *t;
    for (i = 0; i < n; i++) if (r[i].weight > top) top = r[i].weight;
    for (shift = 0; shift < 32; shift += 16) {            /* least significant first: the key, then the weight */
        rank_pass(r, tmp, n, 0, shift, count);
        t = r; r = tmp; tmp = t;
    }
    for (shift = 0; shift < 64 && (top >> shift); shift += 16) {
        rank_pass(r, tmp, n, 1, shift, count);
        t = r; r = tmp; tmp = t;
    }
    return r;
}

/* table.uids, table.kmap and table.reach_words from table.ukeys / table.reach (both complete on oslam_stream()): the keys
 * numbered, and the number of every key a reachable distance bin can produce, so that the scene-key kernel looks a
 * pair up with one load.  17^3 words per reachable distance bin (0.8 MB for a model that spans 41 bins).
 *
 * parts[n_parts]: the slice tables of every model that looks its buckets up under this union table (one model, or the
 * members of a group).  A key's weight is the number of entries in its buckets over all of them, and the keys are
 * numbered by descending weight, ties by ascending key: the hit sort orders a reference point's runs by key number, so
 * every vote workgroup meets its long buckets first and its waves end on short ones.  The numbers depend on the
 * tables alone: two builds, or a build and a load, give the same.  vote_order 1 and 3 (oslam_params) number the keys
 * in union-slot order instead. */
int oslam_build_kmap(oslamk_table *t, float d_dist, const oslamk_table *parts, int n_parts, int vote_order)
{
    int rc = OSLAM_OK, j;
    uint32_t h_reach[OSLAMK_REACH_BINS / 32], w, top = 0, n_ids = 0, slot;
    uint32_t *h_keys = NULL, *h_ids = NULL, *count = NULL;
    uint64_t *h_w = NULL;
    key_rank *r = NULL, *r2 = NULL, *res;
    const size_t ucap = t->ucap;
    const int ranked = vote_order == 0 || vote_order == 2;
    t->kmap = NULL;
    t->kmap_bins = 0;
    t->reach_words = 0;
    t->uids = NULL;
    t->n_ids = t->id_bits = t->uinfo_stride = 0;
    /* the keys of the union table numbered 0 .. n_ids-1: what the hit lists carry and sort on, and what the bucket
     * records are indexed by */
    HIPCHK(hipMalloc((void **)&t->uids, (sizeof(uint32_t) + sizeof(uint64_t)) * ucap));
    HIPCHK(hipMemsetAsync(t->uids, 0, (sizeof(uint32_t) + sizeof(uint64_t)) * ucap, (hipStream_t)oslam_stream()));
    for (j = 0; j < n_parts; j++) {
        oslamk_table p = parts[j];
        p.ukeys = t->ukeys;
        p.ucap = t->ucap;
        p.ushift = t->ushift;
        KCHK(oslamk_union_weights(p, OSLAMK_UWEIGHTS(*t), oslam_stream()));
    }
    h_keys = (uint32_t *)malloc(sizeof(uint32_t) * ucap);
    h_ids = (uint32_t *)calloc(ucap, sizeof(uint32_t));
    h_w = (uint64_t *)malloc(sizeof(uint64_t) * ucap);
    count = (uint32_t *)malloc(sizeof(uint32_t) * 65536);
    if (!h_keys || !h_ids || !h_w || !count) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    HIPCHK(hipMemcpy(h_keys, t->ukeys, sizeof(uint32_t) * ucap, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_w, OSLAMK_UWEIGHTS(*t), sizeof(uint64_t) * ucap, hipMemcpyDeviceToHost));
    for (slot = 0; slot < ucap; slot++) n_ids += h_keys[slot] != 0u;
    if (ranked) {
        size_t i = 0;
        r = (key_rank *)malloc(sizeof *r * (n_ids ? n_ids : 1));
        r2 = (key_rank *)malloc(sizeof *r2 * (n_ids ? n_ids : 1));
        if (!r || !r2) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        for (slot = 0; slot < ucap; slot++)
            if (h_keys[slot] != 0u) {
                r[i].weight = h_w[slot];
                r[i].key = h_keys[slot];
                r[i].slot = slot;
                i++;
            }
        res = rank_keys(r, r2, n_ids, count);
        for (i = 0; i < n_ids; i++) h_ids[res[i].slot] = (uint32_t)i;
    } else {
        uint32_t next = 0;
        for (slot = 0; slot < ucap; slot++)
            if (h_keys[slot] != 0u) h_ids[slot] = next++;
    }
    HIPCHK(hipMemcpy(t->uids, h_ids, sizeof(uint32_t) * ucap, hipMemcpyHostToDevice));
    t->n_ids = n_ids;
    t->id_bits = 1;
    while (t->id_bits < 32u && ((uint64_t)1 << t->id_bits) < (uint64_t)n_ids) t->id_bits++;
    t->uinfo_stride = (n_ids + 63u) & ~63u;
    if (t->uinfo_stride == 0) t->uinfo_stride = 64;
    HIPCHK(hipMemcpy(h_reach, t->reach, sizeof h_reach, hipMemcpyDeviceToHost));
    for (w = 0; w < OSLAMK_REACH_BINS / 32; w++)
        if (h_reach[w]) {
            t->reach_words = w + 1;
            top = 32u * w + (32u - (uint32_t)__builtin_clz(h_reach[w]));    /* highest reachable bin + 1 */
        }
    t->kmap_bins = top < OSLAMK_KMAP_MAX_BINS ? top : OSLAMK_KMAP_MAX_BINS;
    if (t->kmap_bins) {
        HIPCHK(hipMalloc((void **)&t->kmap, sizeof(uint32_t) * (size_t)t->kmap_bins * PC_ANGLE_COMBOS));
        KCHK(oslamk_kmap_build(*t, d_dist, oslam_stream()));
    }
done:
    free(h_keys);
    free(h_ids);
    free(h_w);
    free(count);
    free(r);
    free(r2);
    return rc;
}

/* table.ukeys (every distinct key of the model once, at most a quarter full; `distinct` = an upper bound of
 * their number) and table.reach (the distance bins that can produce a key); d_n_keys / d_overflow: device words */
int oslam_build_union(oslam_model *m, uint32_t distinct, uint32_t *d_n_keys, uint32_t *d_overflow)
{
    int rc = OSLAM_OK;
    uint32_t lg = 16;
    while ((1u << lg) < 4u * distinct && lg < OSLAMK_RUN_SHIFT) lg++;
    if ((1u << lg) < 2u * distinct) return fail(OSLAM_E_LIMIT, "more distinct pair keys than the union table can index");
    if (m->table.ukeys && !m->shared_union) (void)hipFree(m->table.ukeys);
    if (m->table.reach && !m->shared_union) (void)hipFree(m->table.reach);
    if (m->table.kmap && !m->shared_union) (void)hipFree(m->table.kmap);
    if (m->table.uids && !m->shared_union) (void)hipFree(m->table.uids);
    m->table.ukeys = NULL;
    m->table.reach = NULL;
    m->table.kmap = NULL;
    m->table.uids = NULL;
    m->shared_union = 0;
    m->table.ucap = 1u << lg;
    m->table.ushift = 32 - lg;
    HIPCHK(hipMalloc((void **)&m->table.ukeys, sizeof(uint32_t) * (size_t)m->table.ucap));
    HIPCHK(hipMemsetAsync(m->table.ukeys, 0, sizeof(uint32_t) * (size_t)m->table.ucap, (hipStream_t)oslam_stream()));
    HIPCHK(hipMemsetAsync(d_overflow, 0, sizeof(uint32_t), (hipStream_t)oslam_stream()));
    HIPCHK(hipMemsetAsync(d_n_keys, 0, sizeof(uint32_t), (hipStream_t)oslam_stream()));
    KCHK(oslamk_union_build(m->table, d_n_keys, d_overflow, oslam_stream()));
    /* which distance bins can produce a model key at all (lets the scene-key kernel drop far pairs) */
    HIPCHK(hipMalloc((void **)&m->table.reach, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32)));
    HIPCHK(hipMemsetAsync(m->table.reach, 0, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32), (hipStream_t)oslam_stream()));
    KCHK(oslamk_reach_build(m->table, m->d_dist, oslam_stream()));
    rc = oslam_build_kmap(&m->table, m->d_dist, &m->table, 1, m->params.vote_order);
done:
    return rc;
}

/* table.uinfo: the bucket of every union-table slot in every slice (what the vote kernel reads) */
int oslam_build_uinfo(oslam_model *m)
{
    int rc = OSLAM_OK;
    const size_t bytes = sizeof(oslamk_uinfo) * (size_t)m->table.n_slices * (size_t)m->table.uinfo_stride;
    if (m->table.uinfo) { (void)hipFree(m->table.uinfo); m->table.uinfo = NULL; }
    HIPCHK(hipMalloc((void **)&m->table.uinfo, bytes));
    HIPCHK(hipMemsetAsync(m->table.uinfo, 0, bytes, (hipStream_t)oslam_stream()));
    KCHK(oslamk_uinfo_build(m->table, oslam_stream()));
done:
    return rc;
}

int oslam_model_create(const float *xyz, const float *nrm, size_t n, size_t stride_bytes,
                       float d_dist, const oslam_params *params, oslam_model **out)
{
    int rc = OSLAM_OK;
    oslam_model *m = NULL;
    uint32_t *d_small = NULL;        /* [0..n_slices) n_unique, then overflow, total, n_first */
    uint32_t h_small[64 + 3];
    float *h_tmg = NULL, *d_tmg = NULL;
    int n_slices, s;
    uint32_t cap;
    size_t n_pairs;

    if (!out) return fail(OSLAM_E_INVALID, "out is NULL");
    *out = NULL;
    if (!xyz || !nrm || stride_bytes < 12 || !(d_dist > 0.0f)) return fail(OSLAM_E_INVALID, "bad model arguments");
    if (n < 2) return fail(OSLAM_E_INVALID, "model needs at least 2 points");
    if (n > 46340) return fail(OSLAM_E_LIMIT, "model larger than 46340 points (32-bit pair index, kernel.cu:433)");
    m = (oslam_model *)calloc(1, sizeof *m);
    if (!m) return fail(OSLAM_E_NOMEM, "host allocation failed");
    if (params) m->params = *params; else oslam_params_default(&m->params);
    if (m->params.max_cells == 0) m->params.max_cells = 1u << 22;
    rc = oslam_pick_device(m->params.dev, &m->dev);
    if (rc != OSLAM_OK) goto done;
    rc = oslam_cloud_make(&m->c, xyz, nrm, stride_bytes, NULL, n);
    if (rc != OSLAM_OK) goto done;
    oslam_cloud_shape(m->c.h_xyz, n, m->cm, m->inst_c, &m->inst_extent);
    m->d_dist = d_dist;
    m->inv_d_dist = 1.0f / d_dist;
    m->weights = (float *)malloc(sizeof(float) * n);
    if (!m->weights) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    for (s = 0; s < (int)n; s++) m->weights[s] = 1.0f;          /* model.cu:67 */

    n_slices = (int)((n + OSLAMK_SLICE - 1) / OSLAMK_SLICE);
    if (n_slices > 64) { rc = fail(OSLAM_E_LIMIT, "too many model slices"); goto done; }
    HIPCHK(hipMalloc((void **)&d_small, sizeof(uint32_t) * (64 + 3)));

    /* pass 1 with table growth: a slice table is kept at most half full */
    for (cap = 1u << 16;; cap <<= 1) {
        int grow = 0;
        uint32_t lg = 0;
        while ((1u << lg) < cap) lg++;
        if (m->table.slots) { (void)hipFree(m->table.slots); m->table.slots = NULL; }
        HIPCHK(hipMalloc((void **)&m->table.slots, sizeof(oslamk_slot) * (size_t)cap * n_slices));
        HIPCHK(hipMemsetAsync(m->table.slots, 0, sizeof(oslamk_slot) * (size_t)cap * n_slices, (hipStream_t)oslam_stream()));
        HIPCHK(hipMemsetAsync(d_small, 0, sizeof(uint32_t) * (64 + 3), (hipStream_t)oslam_stream()));
        m->table.cap = cap;
        m->table.shift = 32 - lg;
        m->table.n_slices = n_slices;
        KCHK(oslamk_model_count(m->c.k, m->d_dist, m->inv_d_dist, m->table, d_small, d_small + 64, oslam_stream()));
        HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
        HIPCHK(hipMemcpy(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost));
        if (h_small[64]) grow = 1;
        for (s = 0; s < n_slices; s++) if (h_small[s] > cap / 2) grow = 1;
        if (!grow) break;
        if (cap >= (1u << 26)) { rc = fail(OSLAM_E_LIMIT, "model hash table would exceed 2^26 slots per slice"); goto done; }
    }
    KCHK(oslamk_table_scan(m->table, d_small + 65, oslam_stream()));
    /* union of all slices' keys, kept at most a quarter full */
    {
        uint32_t sum = 0;
        for (s = 0; s < n_slices; s++) sum += h_small[s];
        rc = oslam_build_union(m, sum, d_small + 66, d_small + 64);
        if (rc != OSLAM_OK) goto done;
    }
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    HIPCHK(hipMemcpy(h_small, d_small, sizeof h_small, hipMemcpyDeviceToHost));
    if (h_small[64]) { rc = fail(OSLAM_E_LIMIT, "union key table overflow"); goto done; }
    m->n_entries = h_small[65];
    m->ent.n_real = m->n_entries;
    m->num_model_keys = (uint64_t)h_small[66] + 1;    /* + the key-0 bucket of the n self pairs */
    n_pairs = m->n_entries ? m->n_entries : 1;

    /* rows y,z of T_m_g per model point, on the host with libm (kernel.cu:310-318) */
    h_tmg = (float *)malloc(sizeof(float) * 8 * n);
    if (!h_tmg) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    oslam_T_g_rows(m->c.h_xyz, m->c.h_nrm, NULL, n, h_tmg);
    HIPCHK(hipMalloc((void **)&d_tmg, sizeof(float) * 8 * n));
    HIPCHK(hipMemcpy(d_tmg, h_tmg, sizeof(float) * 8 * n, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&m->ent.e4, sizeof(uint32_t) * (n_pairs + 256)));   /* + a chunk: the vote kernel loads whole chunks */
    HIPCHK(hipMalloc((void **)&m->ent.mi, sizeof(uint16_t) * n_pairs));
    if (m->params.vote_mode != OSLAM_VOTE_FAST)
        HIPCHK(hipMalloc((void **)&m->ent.uv, sizeof(oslamk_uv) * n_pairs));
    /* every word a padding entry until the fill pass writes it: padding votes into the accumulator's sink row */
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)m->ent.e4, (int)PC_ROW_SINK, n_pairs + 256, (hipStream_t)oslam_stream()));
    KCHK(oslamk_model_fill(m->c.k, m->d_dist, m->inv_d_dist, m->table, d_tmg, m->ent, oslam_stream()));
    if (!m->params.no_bucket_spread) KCHK(oslamk_bucket_spread(m->table, m->ent, oslam_stream()));   /* the switch is for A/B measurements */
    if (m->ent.uv) {
        /* exact mode: every bucket once more in the order of the votes' positions inside their bins, with the uv of
         * its entries (oslamk_entries.pw / .puv); the uv in bucket order are not needed after that */
        HIPCHK(hipMalloc((void **)&m->ent.pw, sizeof(uint32_t) * n_pairs));
        HIPCHK(hipMalloc((void **)&m->ent.puv, sizeof(oslamk_uv) * n_pairs));
        HIPCHK(hipMalloc((void **)&m->ent.pdir, sizeof(uint16_t) * ((n_pairs + 256) << OSLAMK_PDIR_SHIFT)));
        KCHK(oslamk_bucket_psort(m->table, m->ent, oslam_stream()));
        HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
        (void)hipFree(m->ent.uv);
        m->ent.uv = NULL;
    }
    rc = oslam_build_uinfo(m);
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));

    m->out_cap = m->params.max_cells;
    HIPCHK(hipMalloc((void **)&m->d_counters, sizeof(oslamk_counters)));
    HIPCHK(hipMalloc((void **)&m->d_out, sizeof(oslamk_cell) * (size_t)m->out_cap));
    m->h_out = (oslam_cell *)malloc(sizeof(oslam_cell) * (size_t)m->out_cap);
    if (!m->h_out) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
done:
    free(h_tmg);
    if (d_tmg) (void)hipFree(d_tmg);
    if (d_small) (void)hipFree(d_small);
    if (rc != OSLAM_OK) { oslam_model_destroy(m); return rc; }
    *out = m;
    return OSLAM_OK;
}

/* ------------------------------------------------------------------------
 * persistent model database: one file per built model
 * ---------------------------------------------------------------------- */
#define OSLAM_DB_MAGIC 0x4c444d4f534c4f00ull     /* "\0OLSOMDL" */
#define OSLAM_DB_VERSION 7u                      /* table layout: 16-B slots, slices of 2046 points, e4 = theta (2^-21 turn) << 11 | half << 10 | row,
                                                  * padding words = row 1023; checksum covers the header;
                                                  * 7: exact mode stores the buckets a second time in vote-position order (pw, puv) instead of uv */
typedef struct db_header {
    uint64_t magic;
    uint32_t version, vote_mode;
    uint32_t n_points, n_slices, cap, shift, ucap, ushift, n_entries, has_uv;
    uint64_t num_model_keys;
    float d_dist, inv_d_dist;
    uint64_t checksum;                           /* FNV-1a 64 over the header (this field zero) and every payload byte, in file order */
} db_header;

static uint64_t fnv64(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t i;
    for (i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}

/* device array <-> file through a bounded staging buffer */
static int db_write_dev(FILE *f, const void *dev, size_t bytes, uint64_t *sum)
{
    int rc = OSLAM_OK;
    const size_t chunk = (size_t)64 << 20;
    char *h = (char *)malloc(bytes < chunk ? (bytes ? bytes : 1) : chunk);
    size_t off;
    if (!h) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (off = 0; off < bytes; off += chunk) {
        const size_t n = bytes - off < chunk ? bytes - off : chunk;
        HIPCHK(hipMemcpy(h, (const char *)dev + off, n, hipMemcpyDeviceToHost));
        *sum = fnv64(*sum, h, n);
        if (fwrite(h, 1, n, f) != n) { rc = fail(OSLAM_E_INVALID, "short write"); goto done; }
    }
done:
    free(h);
    return rc;
}

static int db_read_dev(FILE *f, void *dev, size_t bytes, uint64_t *sum)
{
    int rc = OSLAM_OK;
    const size_t chunk = (size_t)64 << 20;
    char *h = (char *)malloc(bytes < chunk ? (bytes ? bytes : 1) : chunk);
    size_t off;
    if (!h) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (off = 0; off < bytes; off += chunk) {
        const size_t n = bytes - off < chunk ? bytes - off : chunk;
        if (fread(h, 1, n, f) != n) { rc = fail(OSLAM_E_INVALID, "model file is truncated"); goto done; }
        *sum = fnv64(*sum, h, n);
        HIPCHK(hipMemcpy((char *)dev + off, h, n, hipMemcpyHostToDevice));
    }
done:
    free(h);
    return rc;
}

static uint32_t log2_exact(uint32_t v)            /* v a power of two */
{
    uint32_t lg = 0;
    while ((1u << lg) < v) lg++;
    return lg;
}

int oslam_model_save(const oslam_model *m, const char *path)
{
    int rc = OSLAM_OK;
    FILE *f = NULL;
    db_header hd;
    uint64_t sum = 0xcbf29ce484222325ull;
    const size_t n = m ? (size_t)m->c.n : 0;
    if (!m || !path) return fail(OSLAM_E_INVALID, "NULL argument");
    if (hipSetDevice(m->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    memset(&hd, 0, sizeof hd);
    hd.magic = OSLAM_DB_MAGIC;
    hd.version = OSLAM_DB_VERSION;
    hd.vote_mode = (uint32_t)m->params.vote_mode;
    hd.n_points = (uint32_t)n;
    hd.n_slices = (uint32_t)m->table.n_slices;
    hd.cap = m->table.cap;
    hd.shift = m->table.shift;
    hd.ucap = m->table.ucap;
    hd.ushift = m->table.ushift;
    hd.n_entries = m->n_entries;
    hd.has_uv = m->ent.pw ? 1u : 0u;
    hd.num_model_keys = m->num_model_keys;
    hd.d_dist = m->d_dist;
    hd.inv_d_dist = m->inv_d_dist;
    f = fopen(path, "wb");
    if (!f) return fail(OSLAM_E_INVALID, "cannot open the model file for writing");
    if (fwrite(&hd, sizeof hd, 1, f) != 1) { rc = fail(OSLAM_E_INVALID, "short write"); goto done; }
    /* checksummed: the header (checksum field still zero), host cloud, weights, then the device arrays */
    sum = fnv64(sum, &hd, sizeof hd);
    sum = fnv64(sum, m->c.h_xyz, 12 * n);
    sum = fnv64(sum, m->c.h_nrm, 12 * n);
    sum = fnv64(sum, m->weights, 4 * n);
    if (fwrite(m->c.h_xyz, 12, n, f) != n || fwrite(m->c.h_nrm, 12, n, f) != n || fwrite(m->weights, 4, n, f) != n) {
        rc = fail(OSLAM_E_INVALID, "short write");
        goto done;
    }
    rc = db_write_dev(f, m->table.slots, sizeof(oslamk_slot) * (size_t)hd.cap * hd.n_slices, &sum);
    if (rc == OSLAM_OK) rc = db_write_dev(f, m->table.ukeys, sizeof(uint32_t) * (size_t)hd.ucap, &sum);
    if (rc == OSLAM_OK) rc = db_write_dev(f, m->table.reach, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32), &sum);
    if (rc == OSLAM_OK) rc = db_write_dev(f, m->ent.e4, sizeof(uint32_t) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK) rc = db_write_dev(f, m->ent.mi, sizeof(uint16_t) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK && hd.has_uv) rc = db_write_dev(f, m->ent.pw, sizeof(uint32_t) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK && hd.has_uv) rc = db_write_dev(f, m->ent.puv, sizeof(oslamk_uv) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK && hd.has_uv) rc = db_write_dev(f, m->ent.pdir, sizeof(uint16_t) * ((size_t)hd.n_entries << OSLAMK_PDIR_SHIFT), &sum);
    if (rc != OSLAM_OK) goto done;
    hd.checksum = sum;
    if (fseek(f, 0, SEEK_SET) != 0 || fwrite(&hd, sizeof hd, 1, f) != 1) rc = fail(OSLAM_E_INVALID, "short write");
done:
    if (f && fclose(f) != 0 && rc == OSLAM_OK) rc = fail(OSLAM_E_INVALID, "short write");
    return rc;
}

int oslam_model_load(const char *path, const oslam_params *params, oslam_model **out)
{
    int rc = OSLAM_OK;
    FILE *f = NULL;
    db_header hd, hz;
    oslam_model *m = NULL;
    float *xyz = NULL, *nrm = NULL;
    oslamk_slot *h_slots = NULL;
    uint64_t sum = 0xcbf29ce484222325ull;
    size_t n, n_pairs, n_slots, i;
    if (!out) return fail(OSLAM_E_INVALID, "out is NULL");
    *out = NULL;
    if (!path) return fail(OSLAM_E_INVALID, "path is NULL");
    f = fopen(path, "rb");
    if (!f) return fail(OSLAM_E_INVALID, "cannot open the model file");
    if (fread(&hd, sizeof hd, 1, f) != 1 || hd.magic != OSLAM_DB_MAGIC) { rc = fail(OSLAM_E_INVALID, "not a model file"); goto done; }
    if (hd.version != OSLAM_DB_VERSION) { rc = fail(OSLAM_E_INVALID, "model file has another table layout version"); goto done; }
    /* every field a kernel indexes with is checked against the others: a stale or damaged header must not
     * reach the GPU (slot_of() shifts by `shift`, the vote kernel dereferences uv in exact mode) */
    n = hd.n_points;
    if (n < 2 || n > 46340 || hd.n_slices != (n + OSLAMK_SLICE - 1) / OSLAMK_SLICE || hd.n_slices > 64 ||
        hd.cap < 2 || (hd.cap & (hd.cap - 1)) || hd.cap > (1u << 26) || hd.ucap < 2 || (hd.ucap & (hd.ucap - 1)) ||
        hd.ucap > (1u << OSLAMK_RUN_SHIFT) || hd.shift != 32u - log2_exact(hd.cap) || hd.ushift != 32u - log2_exact(hd.ucap) ||
        !(hd.d_dist > 0.0f) || hd.inv_d_dist != 1.0f / hd.d_dist || hd.has_uv > 1u ||
        hd.vote_mode > (uint32_t)OSLAM_VOTE_FAST || (hd.vote_mode != (uint32_t)OSLAM_VOTE_FAST && !hd.has_uv) ||
        (uint64_t)hd.n_entries > (uint64_t)n * (n - 1) + 3ull * (uint64_t)hd.cap * hd.n_slices ||
        hd.num_model_keys > (uint64_t)hd.ucap + 1) {
        rc = fail(OSLAM_E_INVALID, "model file header is inconsistent");
        goto done;
    }
    hz = hd;
    hz.checksum = 0;
    sum = fnv64(sum, &hz, sizeof hz);
    m = (oslam_model *)calloc(1, sizeof *m);
    if (!m) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    if (params) m->params = *params; else oslam_params_default(&m->params);
    if (m->params.max_cells == 0) m->params.max_cells = 1u << 22;
    if (params && (uint32_t)params->vote_mode != hd.vote_mode && !(hd.has_uv && params->vote_mode == OSLAM_VOTE_FAST)) {
        rc = fail(OSLAM_E_INVALID, "model file was built in fast vote mode: it has no exact entries");
        goto done;
    }
    if (!params) m->params.vote_mode = (int)hd.vote_mode;
    rc = oslam_pick_device(m->params.dev, &m->dev);
    if (rc != OSLAM_OK) goto done;
    xyz = (float *)malloc(12 * n);
    nrm = (float *)malloc(12 * n);
    m->weights = (float *)malloc(4 * n);
    n_slots = (size_t)hd.cap * hd.n_slices;
    h_slots = (oslamk_slot *)malloc(sizeof(oslamk_slot) * n_slots);
    if (!xyz || !nrm || !m->weights || !h_slots) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    if (fread(xyz, 12, n, f) != n || fread(nrm, 12, n, f) != n || fread(m->weights, 4, n, f) != n ||
        fread(h_slots, sizeof(oslamk_slot), n_slots, f) != n_slots) {
        rc = fail(OSLAM_E_INVALID, "model file is truncated");
        goto done;
    }
    sum = fnv64(sum, xyz, 12 * n);
    sum = fnv64(sum, nrm, 12 * n);
    sum = fnv64(sum, m->weights, 4 * n);
    sum = fnv64(sum, h_slots, sizeof(oslamk_slot) * n_slots);
    /* the buckets lie one behind the other in slot order, each rounded up to four entries (k_table_scan), and none
     * reaches past the entry arrays: the vote kernel addresses a slice's entries relative to its first slot's start */
    {
        uint64_t run = 0;
        for (i = 0; i < n_slots; i++) {
            if (h_slots[i].start != run || run + h_slots[i].len > hd.n_entries) {
                rc = fail(OSLAM_E_INVALID, "model file: a bucket lies outside the entry arrays or out of order");
                goto done;
            }
            run += ((uint64_t)h_slots[i].len + 3u) & ~(uint64_t)3u;
        }
    }
    rc = oslam_cloud_make(&m->c, xyz, nrm, 12, NULL, n);
    if (rc != OSLAM_OK) goto done;
    oslam_cloud_shape(m->c.h_xyz, n, m->cm, m->inst_c, &m->inst_extent);
    m->d_dist = hd.d_dist;
    m->inv_d_dist = hd.inv_d_dist;
    m->table.cap = hd.cap;
    m->table.shift = hd.shift;
    m->table.n_slices = (int)hd.n_slices;
    m->table.ucap = hd.ucap;
    m->table.ushift = hd.ushift;
    m->n_entries = hd.n_entries;
    m->ent.n_real = hd.n_entries;
    m->num_model_keys = hd.num_model_keys;
    n_pairs = hd.n_entries ? hd.n_entries : 1;
    HIPCHK(hipMalloc((void **)&m->table.slots, sizeof(oslamk_slot) * n_slots));
    HIPCHK(hipMalloc((void **)&m->table.ukeys, sizeof(uint32_t) * (size_t)hd.ucap));
    HIPCHK(hipMalloc((void **)&m->table.reach, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32)));
    HIPCHK(hipMalloc((void **)&m->ent.e4, sizeof(uint32_t) * (n_pairs + 256)));   /* + a chunk: the vote kernel loads whole chunks */
    HIPCHK(hipMalloc((void **)&m->ent.mi, sizeof(uint16_t) * n_pairs));
    if (hd.has_uv) {
        HIPCHK(hipMalloc((void **)&m->ent.pw, sizeof(uint32_t) * n_pairs));
        HIPCHK(hipMalloc((void **)&m->ent.puv, sizeof(oslamk_uv) * n_pairs));
        HIPCHK(hipMalloc((void **)&m->ent.pdir, sizeof(uint16_t) * ((n_pairs + 256) << OSLAMK_PDIR_SHIFT)));
    }
    HIPCHK(hipMemcpy(m->table.slots, h_slots, sizeof(oslamk_slot) * n_slots, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)m->ent.e4, (int)PC_ROW_SINK, n_pairs + 256, (hipStream_t)oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    rc = db_read_dev(f, m->table.ukeys, sizeof(uint32_t) * (size_t)hd.ucap, &sum);
    if (rc == OSLAM_OK) rc = db_read_dev(f, m->table.reach, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32), &sum);
    if (rc == OSLAM_OK) rc = db_read_dev(f, m->ent.e4, sizeof(uint32_t) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK) rc = db_read_dev(f, m->ent.mi, sizeof(uint16_t) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK && hd.has_uv) rc = db_read_dev(f, m->ent.pw, sizeof(uint32_t) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK && hd.has_uv) rc = db_read_dev(f, m->ent.puv, sizeof(oslamk_uv) * (size_t)hd.n_entries, &sum);
    if (rc == OSLAM_OK && hd.has_uv) rc = db_read_dev(f, m->ent.pdir, sizeof(uint16_t) * ((size_t)hd.n_entries << OSLAMK_PDIR_SHIFT), &sum);
    if (rc != OSLAM_OK) goto done;
    if (sum != hd.checksum) { rc = fail(OSLAM_E_INVALID, "model file checksum mismatch"); goto done; }
    m->h_slots = h_slots;                         /* the bucket tap reads it */
    h_slots = NULL;
    rc = oslam_build_kmap(&m->table, m->d_dist, &m->table, 1, m->params.vote_order);
    if (rc != OSLAM_OK) goto done;
    rc = oslam_build_uinfo(m);
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    m->out_cap = m->params.max_cells;
    HIPCHK(hipMalloc((void **)&m->d_counters, sizeof(oslamk_counters)));
    HIPCHK(hipMalloc((void **)&m->d_out, sizeof(oslamk_cell) * (size_t)m->out_cap));
    m->h_out = (oslam_cell *)malloc(sizeof(oslam_cell) * (size_t)m->out_cap);
    if (!m->h_out) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
done:
    if (f) fclose(f);
    free(xyz);
    free(nrm);
    free(h_slots);
    if (rc != OSLAM_OK) { oslam_model_destroy(m); return rc; }
    *out = m;
    return OSLAM_OK;
}

int oslam_model_info(const oslam_model *m, size_t *n_points, float *d_dist, uint64_t *table_bytes)
{
    if (!m) return fail(OSLAM_E_INVALID, "NULL handle");
    if (n_points) *n_points = (size_t)m->c.n;
    if (d_dist) *d_dist = m->d_dist;
    if (table_bytes)
        *table_bytes = sizeof(oslamk_slot) * (uint64_t)m->table.cap * (uint64_t)m->table.n_slices +
                       sizeof(uint32_t) * (uint64_t)m->table.ucap + sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32) +
                       sizeof(oslamk_uinfo) * (uint64_t)m->table.uinfo_stride * (uint64_t)m->table.n_slices +
                       (uint64_t)m->n_entries * (4 + 2 + (m->ent.pw ? 12 + (2 << OSLAMK_PDIR_SHIFT) : 0)) + 24ull * (uint64_t)m->c.n;
    return OSLAM_OK;
}

int oslam_model_set_point_weights(oslam_model *m, const float *weights, size_t n)
{
    if (!m || !weights || n != (size_t)m->c.n) return fail(OSLAM_E_INVALID, "bad weights");
    memcpy(m->weights, weights, sizeof(float) * n);
    if (m->d_weights) {
        if (hipSetDevice(m->dev) != hipSuccess ||
            hipMemcpy(m->d_weights, m->weights, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess)
            return fail(OSLAM_E_DEVICE, "cannot update the weights on the device");
    }
    return OSLAM_OK;
}
