/*
 * oslam_taps.c -- the parity taps (pair keys, buckets, the accumulator of one reference point, the hit sort and the
 * bucket orders alone, a model's tables, the last result) and the device math self-test.
 */

#include "oslam_internal.h"
#include "oslam_pose.h"
#include "ppf_core.h"

/* parity taps */
static int cloud_row_keys(cloud_buf *c, size_t ref, float d_dist, uint32_t *keys_out)
{
    int rc = OSLAM_OK;
    uint32_t *d = NULL;
    if (!keys_out || ref >= (size_t)c->n) return fail(OSLAM_E_INVALID, "bad reference index");
    HIPCHK(hipMalloc((void **)&d, sizeof(uint32_t) * c->n));
    KCHK(oslamk_row_keys(c->k, (int)ref, d_dist, 1.0f / d_dist, d, oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    HIPCHK(hipMemcpy(keys_out, d, sizeof(uint32_t) * c->n, hipMemcpyDeviceToHost));
done:
    if (d) (void)hipFree(d);
    return rc;
}

int oslam_scene_keys(oslam_scene *s, size_t ref_index, uint32_t *keys_out)
{
    if (!s) return fail(OSLAM_E_INVALID, "NULL handle");
    if (!(s->d_dist > 0.0f)) return fail(OSLAM_E_INVALID, "this scene was made for models of any d_dist (d_dist 0): it has no keys of its own");
    if (hipSetDevice(s->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    return cloud_row_keys(&s->c, ref_index, s->d_dist, keys_out);
}

int oslam_model_keys(oslam_model *m, size_t ref_index, uint32_t *keys_out)
{
    if (!m) return fail(OSLAM_E_INVALID, "NULL handle");
    if (hipSetDevice(m->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    return cloud_row_keys(&m->c, ref_index, m->d_dist, keys_out);
}

static int u32_order(const void *a, const void *b)
{
    uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : (x > y);
}

int oslam_model_bucket(oslam_model *m, uint32_t key, uint32_t *pairs_out, size_t cap, size_t *count_out)
{
    int rc = OSLAM_OK;
    size_t total = 0, written = 0, n_slots;
    int s;
    uint32_t *tmp = NULL;
    uint16_t *tmi = NULL;
    if (!m || !count_out) return fail(OSLAM_E_INVALID, "NULL argument");
    *count_out = 0;
    if (key == 0) return OSLAM_OK;             /* never matched: kernel.cu:491 */
    if (hipSetDevice(m->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    n_slots = (size_t)m->table.cap * m->table.n_slices;
    if (!m->h_slots) {
        m->h_slots = (oslamk_slot *)malloc(sizeof(oslamk_slot) * n_slots);
        if (!m->h_slots) return fail(OSLAM_E_NOMEM, "host allocation failed");
        HIPCHK(hipMemcpy(m->h_slots, m->table.slots, sizeof(oslamk_slot) * n_slots, hipMemcpyDeviceToHost));
    }
    for (s = 0; s < m->table.n_slices; s++) {
        const oslamk_slot *tab = m->h_slots + (size_t)s * m->table.cap;
        uint32_t mask = m->table.cap - 1, slot = oslamk_slot_of(key, m->table.shift), probe;
        for (probe = 0; probe <= mask; probe++) {
            if (tab[slot].key == key) {
                uint32_t len = tab[slot].len, e;
                tmp = (uint32_t *)realloc(tmp, sizeof(uint32_t) * (len ? len : 1));
                tmi = (uint16_t *)realloc(tmi, sizeof(uint16_t) * (len ? len : 1));
                HIPCHK(hipMemcpy(tmp, m->ent.e4 + tab[slot].start, sizeof(uint32_t) * len, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(tmi, m->ent.mi + tab[slot].start, sizeof(uint16_t) * len, hipMemcpyDeviceToHost));
                for (e = 0; e < len; e++, total++)
                    if (pairs_out && written < cap)
                        pairs_out[written++] = ((uint32_t)s * OSLAMK_SLICE + pc_local_of_row11(tmp[e] & PC_ROW_MASK)) * (uint32_t)m->c.n + tmi[e];
                break;
            }
            if (tab[slot].key == 0) break;
            slot = (slot + 1) & mask;
        }
    }
    if (pairs_out) qsort(pairs_out, written, sizeof(uint32_t), u32_order);
    *count_out = total;
done:
    free(tmp);
    free(tmi);
    return rc;
}

int oslam_model_bucket_words(oslam_model *m, uint32_t key, int slice, uint32_t *words_out, size_t cap, size_t *count_out)
{
    int rc = OSLAM_OK;
    oslamk_slot *tab = NULL;
    uint32_t mask, slot, probe;
    if (!m || !count_out || slice < 0 || slice >= m->table.n_slices) return fail(OSLAM_E_INVALID, "bad argument");
    *count_out = 0;
    if (hipSetDevice(m->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    tab = (oslamk_slot *)malloc(sizeof(oslamk_slot) * m->table.cap);
    if (!tab) return fail(OSLAM_E_NOMEM, "host allocation failed");
    HIPCHK(hipMemcpy(tab, m->table.slots + (size_t)slice * m->table.cap, sizeof(oslamk_slot) * m->table.cap, hipMemcpyDeviceToHost));
    mask = m->table.cap - 1;
    slot = oslamk_slot_of(key, m->table.shift);
    for (probe = 0; probe <= mask; probe++, slot = (slot + 1) & mask) {
        if (tab[slot].key == key) {
            size_t n = tab[slot].len < cap ? tab[slot].len : cap;
            *count_out = tab[slot].len;
            if (words_out && n) HIPCHK(hipMemcpy(words_out, m->ent.e4 + tab[slot].start, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
            break;
        }
        if (tab[slot].key == 0) break;
    }
done:
    free(tab);
    return rc;
}

typedef struct key_row {
    uint64_t weight;
    uint32_t key, number;
} key_row;

static int key_row_order(const void *a, const void *b)
{
    const uint32_t x = ((const key_row *)a)->key, y = ((const key_row *)b)->key;
    return x < y ? -1 : (x > y);
}

int oslam_model_key_numbers(oslam_model *m, uint32_t *keys_out, uint32_t *numbers_out, uint64_t *weights_out, size_t cap,
                            size_t *n_out)
{
    int rc = OSLAM_OK;
    uint32_t *h_keys = NULL, *h_ids = NULL, slot;
    uint64_t *h_w = NULL;
    key_row *rows = NULL;
    size_t n = 0, i, ucap;
    if (!m || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = 0;
    if (m->unusable || !m->table.ukeys || !m->table.uids) return fail(OSLAM_E_INVALID, "this model has no key tables");
    if (hipSetDevice(m->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    ucap = m->table.ucap;
    h_keys = (uint32_t *)malloc(sizeof(uint32_t) * ucap);
    h_ids = (uint32_t *)malloc(sizeof(uint32_t) * ucap);
    h_w = (uint64_t *)malloc(sizeof(uint64_t) * ucap);
    rows = (key_row *)malloc(sizeof *rows * ucap);
    if (!h_keys || !h_ids || !h_w || !rows) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    HIPCHK(hipMemcpy(h_keys, m->table.ukeys, sizeof(uint32_t) * ucap, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_ids, m->table.uids, sizeof(uint32_t) * ucap, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h_w, OSLAMK_UWEIGHTS(m->table), sizeof(uint64_t) * ucap, hipMemcpyDeviceToHost));
    for (slot = 0; slot < ucap; slot++)
        if (h_keys[slot] != 0u) {
            rows[n].key = h_keys[slot];
            rows[n].number = h_ids[slot];
            rows[n].weight = h_w[slot];
            n++;
        }
    qsort(rows, n, sizeof *rows, key_row_order);
    for (i = 0; i < n && i < cap; i++) {
        if (keys_out) keys_out[i] = rows[i].key;
        if (numbers_out) numbers_out[i] = rows[i].number;
        if (weights_out) weights_out[i] = rows[i].weight;
    }
    *n_out = n;
done:
    free(h_keys);
    free(h_ids);
    free(h_w);
    free(rows);
    return rc;
}

int oslam_vote_ref_order(const uint32_t *keep, size_t n, uint32_t *order_out)
{
    if ((!keep || !order_out) && n) return fail(OSLAM_E_INVALID, "NULL argument");
    oslam_ref_order(keep, n, order_out);
    return OSLAM_OK;
}

/* one reference point through the kernels of a registration: its accumulator (acc_out, may be NULL) and, with n_out, its
 * sorted hit list and demand (oslam_pool_read_hits) */
static int tap_one_ref(oslam_model *m, oslam_scene *s, size_t ref_index, uint32_t *acc_out, uint32_t *numbers_out,
                       uint32_t *theta_out, uint32_t *idx_out, size_t cap, size_t *n_out, uint32_t *keep_out)
{
    int rc = OSLAM_OK;
    uint32_t *d_dump = NULL, *d_ref = NULL, *h_dump = NULL;
    float *d_tsg = NULL;
    float rows[8];
    uint32_t ref = (uint32_t)ref_index;
    oslamk_counters cnt;
    scratch_pool *pool = NULL;
    size_t cells;
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (ref_index >= (size_t)s->c.n) return fail(OSLAM_E_INVALID, "bad reference index");
    cells = (size_t)m->table.n_slices * OSLAMK_SLICE * OSLAMK_NBIN;
    oslam_T_g_rows(s->c.h_xyz, s->c.h_nrm, &ref, 1, rows);
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc != OSLAM_OK) return rc;
    HIPCHK(hipMalloc((void **)&d_dump, sizeof(uint32_t) * cells));
    HIPCHK(hipMalloc((void **)&d_ref, sizeof(uint32_t)));
    HIPCHK(hipMalloc((void **)&d_tsg, sizeof rows));
    HIPCHK(hipMemcpy(d_ref, &ref, sizeof ref, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_tsg, rows, sizeof rows, hipMemcpyHostToDevice));
    /* one reference point through the same kernels; fixed_gmax = all ones: nothing is emitted */
    rc = oslam_run_votes_group(pool, &m, 1, s, d_ref, d_tsg, 1, 0xffffffffu, d_dump, &cnt, NULL);
    if (rc != OSLAM_OK) goto done;
    if (n_out) {
        rc = oslam_pool_read_hits(pool, numbers_out, theta_out, idx_out, cap, n_out, keep_out);
        if (rc != OSLAM_OK) goto done;
    }
    if (acc_out) {
        h_dump = (uint32_t *)malloc(sizeof(uint32_t) * cells);
        if (!h_dump) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        HIPCHK(hipMemcpy(h_dump, d_dump, sizeof(uint32_t) * cells, hipMemcpyDeviceToHost));
        memcpy(acc_out, h_dump, sizeof(uint32_t) * OSLAMK_NBIN * (size_t)m->c.n);
    }
done:
    oslam_pool_unlock(pool);
    free(h_dump);
    if (d_dump) (void)hipFree(d_dump);
    if (d_ref) (void)hipFree(d_ref);
    if (d_tsg) (void)hipFree(d_tsg);
    return rc;
}

int oslam_vote_accumulator(oslam_model *m, oslam_scene *s, size_t ref_index, uint32_t *acc_out)
{
    if (!acc_out) return fail(OSLAM_E_INVALID, "bad reference index");
    return tap_one_ref(m, s, ref_index, acc_out, NULL, NULL, NULL, 0, NULL, NULL);
}

int oslam_vote_hits(oslam_model *m, oslam_scene *s, size_t ref_index, uint32_t *numbers_out, uint32_t *theta_out,
                    uint32_t *idx_out, size_t cap, size_t *n_out, uint32_t *keep_out)
{
    if (!n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = 0;
    return tap_one_ref(m, s, ref_index, NULL, numbers_out, theta_out, idx_out, cap, n_out, keep_out);
}

/* k_sort_hits alone, on lists the caller supplies: one launch over n_lists lists, every array copied back whole.  What
 * the kernel does not own (hit_sorted, runs and run_count past a list's hits) is filled with 0xA5 bytes before the launch */
int oslam_sort_hits_tap(const uint32_t *numbers, const uint32_t *theta, const uint32_t *idx, const uint32_t *offsets,
                        const uint32_t *counts, size_t n_lists, uint32_t id_bits, int dev, uint32_t *numbers_out,
                        uint32_t *theta_out, uint32_t *idx_out, uint32_t *runs_out, uint32_t *run_counts_out)
{
    int rc = OSLAM_OK, devsel;
    size_t total, i, slots;
    oslamk_pay *h_pay = NULL;
    uint32_t *d_off = NULL, *d_cnt = NULL, *d_key = NULL, *d_rc = NULL;
    oslamk_pay *d_pay = NULL, *d_sorted = NULL;
    oslamk_run *d_runs = NULL;
    oslamk_vote_args a;
    hipStream_t st;
    if (!numbers || !theta || !idx || !offsets || !counts || !numbers_out || !theta_out || !idx_out || !runs_out || !run_counts_out)
        return fail(OSLAM_E_INVALID, "NULL argument");
    if (id_bits < 1u || id_bits > OSLAMK_RUN_SHIFT) return fail(OSLAM_E_INVALID, "id_bits outside 1 .. 26");
    if (n_lists > 0x7fffffffu) return fail(OSLAM_E_INVALID, "too many lists");
    for (i = 0; i < n_lists; i++)
        if (offsets[i + 1] < offsets[i]) return fail(OSLAM_E_INVALID, "the offsets descend");
    total = offsets[n_lists];
    for (i = 0; i < total; i++)
        if (numbers[i] >> id_bits) return fail(OSLAM_E_INVALID, "a key number does not fit id_bits");
    if (n_lists == 0) return OSLAM_OK;
    rc = oslam_pick_device(dev, &devsel);
    if (rc != OSLAM_OK) return rc;
    st = (hipStream_t)oslam_stream();
    slots = total ? total : 1;
    h_pay = (oslamk_pay *)malloc(sizeof *h_pay * slots);
    if (!h_pay) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (i = 0; i < total; i++) {
        h_pay[i].theta_t22 = theta[i];
        h_pay[i].idx = idx[i];
    }
    HIPCHK(hipMalloc((void **)&d_off, sizeof(uint32_t) * (n_lists + 1)));
    HIPCHK(hipMalloc((void **)&d_cnt, sizeof(uint32_t) * n_lists));
    HIPCHK(hipMalloc((void **)&d_rc, sizeof(uint32_t) * n_lists));
    HIPCHK(hipMalloc((void **)&d_key, sizeof(uint32_t) * slots));
    HIPCHK(hipMalloc((void **)&d_pay, sizeof(oslamk_pay) * slots));
    HIPCHK(hipMalloc((void **)&d_sorted, sizeof(oslamk_pay) * slots));
    HIPCHK(hipMalloc((void **)&d_runs, sizeof(oslamk_run) * slots));
    HIPCHK(hipMemcpy(d_off, offsets, sizeof(uint32_t) * (n_lists + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_cnt, counts, sizeof(uint32_t) * n_lists, hipMemcpyHostToDevice));
    if (total) {
        HIPCHK(hipMemcpy(d_key, numbers, sizeof(uint32_t) * total, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_pay, h_pay, sizeof(oslamk_pay) * total, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemsetAsync(d_sorted, 0xA5, sizeof(oslamk_pay) * slots, st));
    HIPCHK(hipMemsetAsync(d_runs, 0xA5, sizeof(oslamk_run) * slots, st));
    HIPCHK(hipMemsetAsync(d_rc, 0xA5, sizeof(uint32_t) * n_lists, st));
    memset(&a, 0, sizeof a);                   /* only what k_sort_hits reads */
    a.hit_off = d_off;
    a.hit_count = d_cnt;
    a.hit_key = d_key;
    a.hit_pay = d_pay;
    a.hit_sorted = d_sorted;
    a.runs = d_runs;
    a.run_count = d_rc;
    a.table.id_bits = id_bits;
    a.n_launch = (int)n_lists;
    KCHK(oslamk_sort_hits(&a, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(run_counts_out, d_rc, sizeof(uint32_t) * n_lists, hipMemcpyDeviceToHost));
    if (total) {
        HIPCHK(hipMemcpy(numbers_out, d_key, sizeof(uint32_t) * total, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(runs_out, d_runs, sizeof(oslamk_run) * total, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_pay, d_sorted, sizeof(oslamk_pay) * total, hipMemcpyDeviceToHost));
        for (i = 0; i < total; i++) {
            theta_out[i] = h_pay[i].theta_t22;
            idx_out[i] = h_pay[i].idx;
        }
    }
done:
    free(h_pay);
    if (d_off) (void)hipFree(d_off);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_rc) (void)hipFree(d_rc);
    if (d_key) (void)hipFree(d_key);
    if (d_pay) (void)hipFree(d_pay);
    if (d_sorted) (void)hipFree(d_sorted);
    if (d_runs) (void)hipFree(d_runs);
    return rc;
}

/* k_bucket_spread and k_bucket_psort alone, on buckets the caller supplies: a slot table of one slice with one slot per
 * bucket, in bucket order (the kernels read t.slots[blockIdx.x] and nothing else of the table, so its cap need not be a
 * power of two), start as k_table_scan gives it, cur = len.  pw, puv and pdir are filled with 0xA5 bytes before the
 * launches; all six arrays are copied back whole */
#define BUCKET_TAP_MAX_LEN (1u << 20)
#define BUCKET_TAP_MAX_TOTAL ((size_t)1 << 24)
int oslam_bucket_order_tap(const uint32_t *lens, const uint32_t *keys, size_t n_buckets, const uint32_t *e4, const float *uv,
                           const uint16_t *mi, int with_uv, int spread, int dev, uint32_t *e4_out, float *uv_out,
                           uint16_t *mi_out, uint32_t *pw_out, float *puv_out, uint16_t *pdir_out)
{
    int rc = OSLAM_OK, devsel;
    size_t total = 0, i, places;
    oslamk_slot *h_slots = NULL;
    oslamk_table t;
    oslamk_entries ent;
    oslamk_uv *d_uv = NULL;
    hipStream_t st;
    memset(&t, 0, sizeof t);
    memset(&ent, 0, sizeof ent);
    if (!lens || !e4 || !uv || !mi || !e4_out || !uv_out || !mi_out || !pw_out || !puv_out || !pdir_out)
        return fail(OSLAM_E_INVALID, "NULL argument");
    if (n_buckets > BUCKET_TAP_MAX_TOTAL) return fail(OSLAM_E_INVALID, "too many buckets");
    for (i = 0; i < n_buckets; i++) {
        if (lens[i] > BUCKET_TAP_MAX_LEN) return fail(OSLAM_E_INVALID, "a bucket is longer than 2^20 entries");
        total += ((size_t)lens[i] + 3u) & ~(size_t)3u;
        if (total > BUCKET_TAP_MAX_TOTAL) return fail(OSLAM_E_INVALID, "the buckets hold more than 2^24 entries");
    }
    if (n_buckets == 0) return OSLAM_OK;
    rc = oslam_pick_device(dev, &devsel);
    if (rc != OSLAM_OK) return rc;
    st = (hipStream_t)oslam_stream();
    h_slots = (oslamk_slot *)malloc(sizeof *h_slots * n_buckets);
    if (!h_slots) return fail(OSLAM_E_NOMEM, "host allocation failed");
    for (i = 0, total = 0; i < n_buckets; i++) {
        h_slots[i].key = keys ? keys[i] : (uint32_t)i + 1u;
        h_slots[i].start = (uint32_t)total;
        h_slots[i].len = h_slots[i].cur = lens[i];
        total += ((size_t)lens[i] + 3u) & ~(size_t)3u;
    }
    places = total ? total : 4;
    t.cap = (uint32_t)n_buckets;
    t.n_slices = 1;
    HIPCHK(hipMalloc((void **)&t.slots, sizeof(oslamk_slot) * n_buckets));
    HIPCHK(hipMalloc((void **)&ent.e4, sizeof(uint32_t) * places));
    HIPCHK(hipMalloc((void **)&d_uv, sizeof(oslamk_uv) * places));
    HIPCHK(hipMalloc((void **)&ent.mi, sizeof(uint16_t) * places));
    HIPCHK(hipMalloc((void **)&ent.pw, sizeof(uint32_t) * places));
    HIPCHK(hipMalloc((void **)&ent.puv, sizeof(oslamk_uv) * places));
    HIPCHK(hipMalloc((void **)&ent.pdir, sizeof(uint16_t) * ((total + 256) << OSLAMK_PDIR_SHIFT)));
    HIPCHK(hipMemcpy(t.slots, h_slots, sizeof(oslamk_slot) * n_buckets, hipMemcpyHostToDevice));
    if (total) {
        HIPCHK(hipMemcpy(ent.e4, e4, sizeof(uint32_t) * total, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_uv, uv, sizeof(oslamk_uv) * total, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ent.mi, mi, sizeof(uint16_t) * total, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemsetAsync(ent.pw, 0xA5, sizeof(uint32_t) * places, st));
    HIPCHK(hipMemsetAsync(ent.puv, 0xA5, sizeof(oslamk_uv) * places, st));
    HIPCHK(hipMemsetAsync(ent.pdir, 0xA5, sizeof(uint16_t) * ((total + 256) << OSLAMK_PDIR_SHIFT), st));
    ent.uv = with_uv ? d_uv : NULL;            /* the fast-mode build has none */
    ent.n_real = (uint32_t)total;
    if (spread) KCHK(oslamk_bucket_spread(t, ent, st));
    if (with_uv) KCHK(oslamk_bucket_psort(t, ent, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total) {
        HIPCHK(hipMemcpy(e4_out, ent.e4, sizeof(uint32_t) * total, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(uv_out, d_uv, sizeof(oslamk_uv) * total, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(mi_out, ent.mi, sizeof(uint16_t) * total, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pw_out, ent.pw, sizeof(uint32_t) * total, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(puv_out, ent.puv, sizeof(oslamk_uv) * total, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(pdir_out, ent.pdir, sizeof(uint16_t) * ((total + 256) << OSLAMK_PDIR_SHIFT), hipMemcpyDeviceToHost));
done:
    free(h_slots);
    if (t.slots) (void)hipFree(t.slots);
    if (ent.e4) (void)hipFree(ent.e4);
    if (d_uv) (void)hipFree(d_uv);
    if (ent.mi) (void)hipFree(ent.mi);
    if (ent.pw) (void)hipFree(ent.pw);
    if (ent.puv) (void)hipFree(ent.puv);
    if (ent.pdir) (void)hipFree(ent.pdir);
    return rc;
}

/* a built model's tables as they lie in device memory -- created, loaded or a member of a database group alike (a member
 * shows its group's union tables): the scalars into *info, then every array whose pointer is given, copied whole.  Nothing
 * is sorted or interpreted here */
int oslam_model_tables_tap(oslam_model *m, oslam_model_tables *info, uint32_t *slots, uint32_t *ukeys, uint32_t *uids,
                           uint64_t *weights, uint32_t *reach, uint32_t *kmap, uint32_t *uinfo, uint32_t *e4, uint16_t *mi,
                           uint32_t *pw, float *puv, uint16_t *pdir)
{
    int rc = OSLAM_OK;
    size_t n_slots, ne;
    const oslamk_table *t;
    if (!m || !info) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(info, 0, sizeof *info);
    t = &m->table;
    if (m->unusable || !t->slots || !t->ukeys || !t->uids || !t->reach || !t->uinfo || !m->ent.e4 || !m->ent.mi)
        return fail(OSLAM_E_INVALID, "this model has no key tables");
    info->cap = t->cap;
    info->shift = t->shift;
    info->n_slices = (uint32_t)t->n_slices;
    info->ucap = t->ucap;
    info->ushift = t->ushift;
    info->n_entries = m->n_entries;
    info->n_ids = t->n_ids;
    info->id_bits = t->id_bits;
    info->uinfo_stride = t->uinfo_stride;
    info->kmap_bins = t->kmap_bins;
    info->reach_words = t->reach_words;
    info->has_pw = m->ent.pw != NULL;
    info->num_model_keys = m->num_model_keys;
    if (!m->ent.pw && (pw || puv || pdir)) return fail(OSLAM_E_INVALID, "a fast-mode model has no second order");
    if (!slots && !ukeys && !uids && !weights && !reach && !kmap && !uinfo && !e4 && !mi && !pw && !puv && !pdir) return OSLAM_OK;
    if (hipSetDevice(m->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    n_slots = (size_t)t->cap * (size_t)t->n_slices;
    ne = m->n_entries;
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    if (slots) HIPCHK(hipMemcpy(slots, t->slots, sizeof(oslamk_slot) * n_slots, hipMemcpyDeviceToHost));
    if (ukeys) HIPCHK(hipMemcpy(ukeys, t->ukeys, sizeof(uint32_t) * t->ucap, hipMemcpyDeviceToHost));
    if (uids) HIPCHK(hipMemcpy(uids, t->uids, sizeof(uint32_t) * t->ucap, hipMemcpyDeviceToHost));
    if (weights) HIPCHK(hipMemcpy(weights, OSLAMK_UWEIGHTS(*t), sizeof(uint64_t) * t->ucap, hipMemcpyDeviceToHost));
    if (reach) HIPCHK(hipMemcpy(reach, t->reach, sizeof(uint32_t) * (OSLAMK_REACH_BINS / 32), hipMemcpyDeviceToHost));
    if (kmap && t->kmap_bins)
        HIPCHK(hipMemcpy(kmap, t->kmap, sizeof(uint32_t) * (size_t)t->kmap_bins * PC_ANGLE_COMBOS, hipMemcpyDeviceToHost));
    if (uinfo) HIPCHK(hipMemcpy(uinfo, t->uinfo, sizeof(oslamk_uinfo) * (size_t)t->n_slices * t->uinfo_stride, hipMemcpyDeviceToHost));
    if (e4) HIPCHK(hipMemcpy(e4, m->ent.e4, sizeof(uint32_t) * (ne + 256), hipMemcpyDeviceToHost));
    if (mi && ne) HIPCHK(hipMemcpy(mi, m->ent.mi, sizeof(uint16_t) * ne, hipMemcpyDeviceToHost));
    if (pw && ne) HIPCHK(hipMemcpy(pw, m->ent.pw, sizeof(uint32_t) * ne, hipMemcpyDeviceToHost));
    if (puv && ne) HIPCHK(hipMemcpy(puv, m->ent.puv, sizeof(oslamk_uv) * ne, hipMemcpyDeviceToHost));
    if (pdir) HIPCHK(hipMemcpy(pdir, m->ent.pdir, sizeof(uint16_t) * ((ne + 256) << OSLAMK_PDIR_SHIFT), hipMemcpyDeviceToHost));
done:
    return rc;
}

/* the taps read the last result from the host: fetch it if it is still on the device */
static int materialise_last(oslam_model *m)
{
    int rc = OSLAM_OK;
    const size_t n = m->n_last;
    if (!m->last_on_device) return OSLAM_OK;
    if (hipSetDevice(m->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    m->last_cells = (oslam_cell *)malloc(sizeof(oslam_cell) * (n ? n : 1));
    m->last_poses = (float *)malloc(sizeof(float) * 16 * (n ? n : 1));
    if (!m->last_cells || !m->last_poses) { oslam_drop_last(m); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    HIPCHK(hipMemcpy(m->last_cells, m->d_pose_cells, sizeof(oslam_cell) * n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(m->last_poses, m->d_pose_T, sizeof(float) * 16 * n, hipMemcpyDeviceToHost));
    m->last_on_device = 0;
done:
    return rc;
}

int oslam_last_result(oslam_model *m, oslam_scene *s, float *trans_out, float *rots_out, float *vote_counts_out,
                      size_t cap, size_t *n_out, uint32_t *max_idx_out)
{
    int rc;
    size_t n;
    float T[16], *tr = NULL, *ro = NULL, *sc = NULL;
    uint32_t best = 0;
    if (!n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    *n_out = 0;
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (materialise_last(m) != OSLAM_OK) return OSLAM_E_DEVICE;
    n = m->n_last;
    if (max_idx_out) *max_idx_out = 0;
    if (n == 0) return OSLAM_OK;
    tr = (float *)calloc(3 * n, sizeof(float));
    ro = (float *)calloc(4 * n, sizeof(float));
    sc = (float *)calloc(n, sizeof(float));
    if (!tr || !ro || !sc) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    rc = oslam_pose_stage_ex(m->last_cells, n, m->c.h_xyz, m->c.h_nrm, (size_t)m->c.n, s->c.h_xyz, s->c.h_nrm, (size_t)s->c.n,
                             m->d_dist, m->params.cpu_clustering, m->params.use_l1_norm, m->params.use_averaged_clusters,
                             m->weights, T, NULL, tr, ro, sc, &best);
    if (rc != OSLAM_OK) { rc = fail(rc, "pose stage failed"); goto done; }
    if (n > cap) n = cap;
    if (trans_out) memcpy(trans_out, tr, sizeof(float) * 3 * n);
    if (rots_out) memcpy(rots_out, ro, sizeof(float) * 4 * n);
    if (vote_counts_out) memcpy(vote_counts_out, sc, sizeof(float) * n);
    if (max_idx_out) *max_idx_out = best;
    *n_out = n;
done:
    free(tr);
    free(ro);
    free(sc);
    return rc;
}

int oslam_last_cells(oslam_model *m, oslam_cell *cells_out, float *poses_out, size_t cap, size_t *n_out)
{
    size_t n;
    if (!m || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if ((cells_out || poses_out) && materialise_last(m) != OSLAM_OK) return OSLAM_E_DEVICE;
    n = m->n_last < cap ? m->n_last : cap;
    if (cells_out) memcpy(cells_out, m->last_cells, sizeof(oslam_cell) * n);
    if (poses_out) memcpy(poses_out, m->last_poses, sizeof(float) * 16 * n);
    *n_out = m->n_last;
    return OSLAM_OK;
}

/* The clustering scores a chosen pose tail really computed (oslam_last_result's are always the host loop's).  The records
 * go through the tail as oslam_align_finish's do, but the tail is named, not chosen by size: path 0 = the host loop,
 * 1 = the host tail with k_cluster_scores behind the hook from two poses on, 2 = the device tail from two kept cells
 * on.  *path_out says which of the three made the scores: a tail that fell back to the host loop reports 0. */
int oslam_tail_scores(oslam_model *m, oslam_scene *s, const oslam_cell *cells, size_t n, uint32_t global_max, int path,
                      oslam_cell *cells_out, float *scores_out, size_t cap, size_t *n_out, uint32_t *max_idx_out,
                      float T[16], int *path_out)
{
    int rc;
    oslam_cell *tmp = NULL;
    float *sc = NULL;
    uint32_t best = 0;
    size_t kept = 0, i;
    scratch_pool *pool = NULL;
    if (!n_out || !path_out || !T || (!cells && n) || path < 0 || path > 2) return fail(OSLAM_E_INVALID, "bad argument");
    *n_out = 0;
    *path_out = -1;
    if (max_idx_out) *max_idx_out = 0;
    memset(T, 0, 16 * sizeof(float));
    rc = oslam_check_pair(m, s);
    if (rc != OSLAM_OK) return rc;
    if (m->params.cpu_clustering || m->params.use_averaged_clusters)
        return fail(OSLAM_E_INVALID, "the host-only clustering variants have no device tail");
    for (i = 0; i < n; i++) {
        const uint32_t sr = (uint32_t)(cells[i].code >> 32), mr = ((uint32_t)cells[i].code) >> 6;
        if (sr >= (uint32_t)s->c.n || sr % s->df != 0 || mr >= (uint32_t)m->c.n)
            return fail(OSLAM_E_INVALID, "a record names no reference point of this scene or no point of this model");
    }
    rc = oslam_pool_enter(m->dev, &pool);
    if (rc != OSLAM_OK) return rc;
    tmp = (oslam_cell *)malloc(sizeof(oslam_cell) * (n ? n : 1));
    sc = (float *)calloc(n ? n : 1, sizeof(float));
    if (!tmp || !sc) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    if (path == 2) {
        uint32_t n_kept = 0;
        int k;
        if (n > m->out_cap) { rc = fail(OSLAM_E_LIMIT, "more records than the record buffer holds"); goto done; }
        oslam_drop_last(m);                        /* the chain writes the buffers a result left on the device lives in */
        rc = oslam_pose_tables(m, s);
        if (rc == OSLAM_OK) rc = oslam_ensure_pose_buffers(m, n);
        if (rc != OSLAM_OK) goto done;
        if (n) HIPCHK(hipMemcpy(m->d_out, cells, sizeof(oslam_cell) * n, hipMemcpyHostToDevice));
        k = oslamk_pose_stage(m->d_out, (uint32_t)n, m->params.vote_count_threshold * global_max, m->d_Tm16, s->d_Ts16, s->df,
                              m->d_weights, oslam_rotx(), m->d_dist, m->params.use_l1_norm, m->d_pose_cells, m->d_pose_T, global_max,
                              (uint32_t)m->c.n, (uint32_t)s->c.n, m->params.pose_two_sorts, NULL, &n_kept, &best, T, NULL,
                              oslam_stream());
        if (k == -2) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        if (k != 0) { rc = fail(OSLAM_E_DEVICE, hipGetErrorString((hipError_t)k)); goto done; }
        if (n_kept < 2) { rc = fail(OSLAM_E_NO_VOTES, "fewer than two cells survive: the device tail leaves them to the host"); goto done; }
        kept = n_kept;
        KCHK(oslamk_pose_scores(n_kept, sc, oslam_stream()));
        HIPCHK(hipMemcpy(tmp, m->d_pose_cells, sizeof(oslam_cell) * kept, hipMemcpyDeviceToHost));
        *path_out = 2;
    } else {
        if (n) memcpy(tmp, cells, sizeof(oslam_cell) * n);
        kept = oslam_filter_cells(tmp, n, m->params.vote_count_threshold, global_max);
        oslam_sort_cells(tmp, kept);
        if (path == 1) {
            oslam_pose_set_cluster_hook(oslam_cluster_scores_on_device);
            oslam_pose_set_cluster_hook_min(1);
        }
        rc = oslam_pose_stage_ex(tmp, kept, m->c.h_xyz, m->c.h_nrm, (size_t)m->c.n, s->c.h_xyz, s->c.h_nrm, (size_t)s->c.n,
                                 m->d_dist, 0, m->params.use_l1_norm, 0, m->weights, T, NULL, NULL, NULL, sc, &best);
        oslam_pose_set_cluster_hook(NULL);
        oslam_pose_set_cluster_hook_min(0);
        if (rc != OSLAM_OK) { rc = fail(rc, rc == OSLAM_E_NO_VOTES ? "no record above the threshold" : "pose stage failed"); goto done; }
        *path_out = kept > 1 && oslam_pose_cluster_hook_used() ? 1 : 0;
    }
    if (cells_out) memcpy(cells_out, tmp, sizeof(oslam_cell) * (kept < cap ? kept : cap));
    if (scores_out) memcpy(scores_out, sc, sizeof(float) * (kept < cap ? kept : cap));
    if (max_idx_out) *max_idx_out = best;
    *n_out = kept;
done:
    oslam_pool_unlock(pool);
    free(tmp);
    free(sc);
    return rc;
}

/* ------------------------------------------------------------------------ */
static uint64_t sm64(uint64_t *s)
{
    uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int oslam_selftest_math(size_t n, uint64_t seed, uint64_t *mismatches)
{
    int rc = OSLAM_OK, dev;
    float *h = NULL, *d = NULL, *ho = NULL;
    size_t i;
    uint64_t bad = 0;
    if (!mismatches || n == 0) return fail(OSLAM_E_INVALID, "bad arguments");
    rc = oslam_pick_device(0, &dev);
    if (rc != OSLAM_OK) return rc;
    h = (float *)malloc(sizeof(float) * 3 * n);
    ho = (float *)malloc(sizeof(float) * 4 * n);
    if (!h || !ho) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    for (i = 0; i < n; i++) {
        uint64_t r = sm64(&seed), r2 = sm64(&seed);
        float x, y, x2;
        switch (i & 3) {
        case 0:   /* acos domain, dense near +-1 and +-0.5 */
            x = (float)((double)(int32_t)(uint32_t)r / 2147483648.0);
            y = (float)((double)(int32_t)(uint32_t)(r >> 32) / 2147483648.0 * 3.0);
            x2 = (float)((double)(int32_t)(uint32_t)r2 / 2147483648.0 * 3.0);
            break;
        case 1:
            x = 1.0f - (float)((double)(uint32_t)r / 4294967296.0) * 1e-3f;
            if (r2 & 1) x = -x;
            y = (float)((double)(int32_t)(uint32_t)(r >> 32) / 2147483648.0);
            x2 = y * ((r2 & 2) ? 0.4375f : 2.4375f) * (1.0f + (float)(int)((r2 >> 8) & 15) * 1e-7f);
            break;
        case 2:   /* raw bit patterns */
            x = PM_BITS_U2F((uint32_t)r);
            y = PM_BITS_U2F((uint32_t)(r >> 32));
            x2 = PM_BITS_U2F((uint32_t)r2);
            break;
        default:
            x = (float)((double)(int32_t)(uint32_t)r / 2147483648.0 * 1.00001);
            y = (float)((double)(int32_t)(uint32_t)(r >> 32) / 2147483648.0 * 1e-3);
            x2 = (float)((double)(int32_t)(uint32_t)r2 / 2147483648.0 * 1e3);
            break;
        }
        h[i] = x; h[n + i] = y; h[2 * n + i] = x2;
    }
    HIPCHK(hipMalloc((void **)&d, sizeof(float) * 7 * n));
    HIPCHK(hipMemcpy(d, h, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    KCHK(oslamk_selftest(d, d + n, d + 2 * n, n, d + 3 * n, d + 4 * n, (uint32_t *)(d + 5 * n),
                         (uint32_t *)(d + 6 * n), oslam_stream()));
    HIPCHK(hipStreamSynchronize((hipStream_t)oslam_stream()));
    HIPCHK(hipMemcpy(ho, d + 3 * n, sizeof(float) * 4 * n, hipMemcpyDeviceToHost));
    for (i = 0; i < n; i++) {
        float x = h[i], y = h[n + i], x2 = h[2 * n + i];
        float a = pm_acosf(x), t = pm_atan2f(y, x2);
        float st = 0.0371f + pm_fabsf(x) * 0.01f;
        uint32_t q = pc_quant_bits(pm_fabsf(y) * 7.0f, st, 1.0f / st);
        uint32_t b = pc_alpha_bin_exact(y, x2, x, y - x2);
        uint32_t ga = PM_BITS_F2U(ho[i]), gt = PM_BITS_F2U(ho[n + i]);
        int a_ok = pm_isnan(a) ? pm_isnan(ho[i]) : (PM_BITS_F2U(a) == ga);
        int t_ok = pm_isnan(t) ? pm_isnan(ho[n + i]) : (PM_BITS_F2U(t) == gt);
        if (!a_ok || !t_ok || q != ((uint32_t *)ho)[2 * n + i] || b != ((uint32_t *)ho)[3 * n + i]) bad++;
    }
    *mismatches = bad;
done:
    free(h);
    free(ho);
    if (d) (void)hipFree(d);
    return rc;
}
