/*
 * oslam_vote.c -- the votes of one registration: the scratch pool of each device, the batches of reference
 * points, the kernels of the scene pass and the votes, the record buffers, and the clustering hook of the
 * pose stage (which works in the pool).
 */
#include <pthread.h>
#include <stdio.h>

#include "oslam_internal.h"

int oslam_check_pair(const oslam_model *m, const oslam_scene *s)
{
    if (!m || !s) return fail(OSLAM_E_INVALID, "NULL handle");
    if (m->unusable) return fail(OSLAM_E_INVALID, "this model lost its key tables with its database: it can only be destroyed");
    if (m->dev != s->dev) return fail(OSLAM_E_INVALID, "model and scene live on different devices");
    /* d_dist 0 = a scene for models of any d_dist: nothing a scene holds here depends on it */
    if (s->d_dist != 0.0f && m->d_dist != s->d_dist) return fail(OSLAM_E_INVALID, "scene d_dist differs from the model's (ppf.cu:64-67)");
    return OSLAM_OK;
}

/* Scratch for the hit lists of one batch of reference points: one pool per device, shared by all
 * models and only live inside a call (calls on one device are serialised by the pool's lock).  The
 * lists are sized by demand: a counting kernel gives, per reference point, the number of scene pairs
 * that can reach a model key at all (an upper bound of its hits, 16 % above them on the bench scene);
 * the host turns the counts into offsets and cuts the reference points into batches that fit the
 * pool.  The pool grows to what a call needs, up to OSLAM_SCRATCH_GIB GiB (default 4; a single
 * reference point that needs more still gets it); oslam_release_scratch frees it. */
#define MAX_DEVICES 64
#define MAX_BATCH_EVENTS 64
#define SLOT_BYTES (sizeof(oslamk_pay) * 2 + sizeof(oslamk_run) + sizeof(uint32_t))
struct scratch_pool {
    pthread_mutex_t lock;
    char *buf;                         /* hit arrays of one batch */
    size_t bytes;
    uint32_t *d_counts;                /* keep_count[cap], hit_count[cap], run_count[cap], hit_off[cap + 1 + batches] */
    uint32_t *h_counts;                /* host staging: keep counts, then offsets */
    size_t counts_cap;
    hipEvent_t ev[4 + 3 * MAX_BATCH_EVENTS];
    int have_events;
    char *d_cluster;                   /* workspace of oslam_cluster_scores_on_device */
    size_t cluster_bytes;
    uint32_t *d_redo;                  /* vote workgroups of a batch whose 16-bit counters overflowed */
    oslamk_vote_args *d_vargs, *h_vargs;   /* a group's vote arguments, one per member (h: pinned), for the one-grid launch */
    size_t vargs_cap;
    size_t redo_cap;
    uint32_t *d_order, *h_order;       /* the order in which a batch's reference points are voted (h: pinned), see oslam_ref_order */
    size_t order_cap;
};
static scratch_pool g_pool[MAX_DEVICES];
static pthread_once_t g_pool_once = PTHREAD_ONCE_INIT;

static void pool_init_all(void)
{
    int i;
    for (i = 0; i < MAX_DEVICES; i++) pthread_mutex_init(&g_pool[i].lock, NULL);
}

/* the pool the calling thread holds (the clustering hook has no other way to reach it) */
static __thread scratch_pool *g_cur_pool;

/* the pool of a device, locked: every entry point that launches on the device holds it for the call */
static scratch_pool *pool_lock(int dev)
{
    pthread_once(&g_pool_once, pool_init_all);
    if (dev < 0 || dev >= MAX_DEVICES) return NULL;
    pthread_mutex_lock(&g_pool[dev].lock);
    g_cur_pool = &g_pool[dev];
    return g_cur_pool;
}

void oslam_pool_unlock(scratch_pool *p)
{
    if (!p) return;
    g_cur_pool = NULL;
    pthread_mutex_unlock(&p->lock);
}

int oslam_pool_enter(int dev, scratch_pool **pool)
{
    *pool = NULL;
    if (hipSetDevice(dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    *pool = pool_lock(dev);
    return *pool ? OSLAM_OK : fail(OSLAM_E_LIMIT, "device ordinal too large");
}

int oslam_release_scratch(int dev)
{
    scratch_pool *p = pool_lock(dev);
    int i;
    if (!p) return fail(OSLAM_E_INVALID, "device ordinal out of range");
    if (p->buf || p->d_counts || p->have_events || p->d_cluster || p->d_redo || p->d_vargs || p->h_vargs || p->d_order || p->h_order) {
        if (hipSetDevice(dev) != hipSuccess) { oslam_pool_unlock(p); return fail(OSLAM_E_DEVICE, "hipSetDevice failed"); }
        if (p->buf) (void)hipFree(p->buf);
        if (p->d_counts) (void)hipFree(p->d_counts);
        if (p->d_cluster) (void)hipFree(p->d_cluster);
        if (p->d_redo) (void)hipFree(p->d_redo);
        if (p->d_vargs) (void)hipFree(p->d_vargs);
        if (p->h_vargs) (void)hipHostFree(p->h_vargs);
        if (p->d_order) (void)hipFree(p->d_order);
        if (p->h_order) (void)hipHostFree(p->h_order);
        oslamk_pose_release();
        if (p->have_events)
            for (i = 0; i < 4 + 3 * MAX_BATCH_EVENTS; i++) (void)hipEventDestroy(p->ev[i]);
    }
    if (hipSetDevice(dev) == hipSuccess) oslam_dev_cache_release(dev);   /* the kept blocks of the scene path */
    oslam_arbitrate_release();
    oslam_track_release();
    oslam_ego_release();
    free(p->h_counts);
    p->buf = NULL;
    p->bytes = 0;
    p->d_counts = NULL;
    p->h_counts = NULL;
    p->counts_cap = 0;
    p->have_events = 0;
    p->d_cluster = NULL;
    p->cluster_bytes = 0;
    p->d_redo = NULL;
    p->redo_cap = 0;
    p->d_vargs = NULL;
    p->h_vargs = NULL;
    p->vargs_cap = 0;
    p->d_order = NULL;
    p->h_order = NULL;
    p->order_cap = 0;
    oslam_pool_unlock(p);
    return OSLAM_OK;
}

static size_t scratch_limit(const oslam_model *m)
{
    return (size_t)(m && m->params.scratch_gib > 0 ? m->params.scratch_gib : 4) << 30;
}

/* per-reference counters for n_ref reference points, events */
int oslam_pool_reserve_counts(scratch_pool *p, size_t n_ref)
{
    int rc = OSLAM_OK, i;
    if (!p->have_events) {
        for (i = 0; i < 4 + 3 * MAX_BATCH_EVENTS; i++) HIPCHK(hipEventCreate(&p->ev[i]));
        p->have_events = 1;
    }
    if (p->counts_cap < n_ref) {
        const size_t cap = n_ref + n_ref / 4 + 64;
        if (p->d_counts) { (void)hipFree(p->d_counts); p->d_counts = NULL; }
        free(p->h_counts);
        p->h_counts = NULL;
        p->counts_cap = 0;
        /* offsets: one more than reference points per batch; a batch holds at least one reference point */
        HIPCHK(hipMalloc((void **)&p->d_counts, sizeof(uint32_t) * (5 * cap + 2)));
        p->h_counts = (uint32_t *)malloc(sizeof(uint32_t) * (3 * cap + 2));
        if (!p->h_counts) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        p->counts_cap = cap;
    }
done:
    return rc;
}

static int pool_reserve_slots(scratch_pool *p, size_t slots, size_t limit)
{
    const size_t base = (slots ? slots : 1) * SLOT_BYTES + 1024;      /* + a wave of hits: the vote kernel loads 64 at a time */
    size_t want = base;
    if (p->bytes >= want) return OSLAM_OK;
    if (p->buf) { (void)hipFree(p->buf); p->buf = NULL; p->bytes = 0; }
    want += want / 8;                 /* head room: the next scene is rarely the same size */
    /* batches are cut to the limit: no head room beyond it, but never less than the batch itself needs (a pool
     * below `base` would be freed and mapped again by every registration) */
    if (want > limit + 1024) want = base > limit + 1024 ? base : limit + 1024;
    if (hipMalloc((void **)&p->buf, want) != hipSuccess) {
        (void)hipGetLastError();
        p->buf = NULL;
        want = (slots ? slots : 1) * SLOT_BYTES + 1024;
        if (hipMalloc((void **)&p->buf, want) != hipSuccess) {
            (void)hipGetLastError();
            p->buf = NULL;
            return fail(OSLAM_E_NOMEM, "no device memory for the hit lists");
        }
    }
    p->bytes = want;
    return OSLAM_OK;
}

/* the arrays of a batch with `slots` places inside the pool */
static void carve_scratch(oslamk_vote_args *a, const scratch_pool *p, size_t slots)
{
    char *b = p->buf;
    a->redo = p->d_redo;
    a->hit_pay = (oslamk_pay *)b;
    b += slots * sizeof(oslamk_pay);
    a->hit_sorted = (oslamk_pay *)b;
    b += slots * sizeof(oslamk_pay);
    a->runs = (oslamk_run *)b;
    b += slots * sizeof(oslamk_run);
    a->hit_key = (uint32_t *)b;
}

/* The batch that starts at reference point `first`: as many reference points as fit `limit_slots` places
 * (at least one).  A list gets its count rounded up to even, so that every list starts 8-byte aligned in
 * the 4-byte key array too.  off (may be NULL) receives the n + 1 offsets; *slots the batch total. */
static int batch_extent(const uint32_t *keep, int first, int n_ref, size_t limit_slots, uint32_t *off, size_t *slots)
{
    size_t t = 0;
    int n = 0;
    while (first + n < n_ref) {
        const size_t need = ((size_t)keep[first + n] + 1u) & ~(size_t)1u;
        if (n > 0 && (t + need > limit_slots || t + need > 0xfffffff0u)) break;
        if (off) off[n] = (uint32_t)t;
        t += need;
        n++;
    }
    if (off) off[n] = (uint32_t)t;
    *slots = t;
    return n;
}

/* The order in which the vote grid takes the n reference points of a batch: order[p] = the reference point of dispatch
 * position p, by descending demand keep[] (the pairs within reach: what the hit lists are sized by, and a measure of
 * the votes that needs no pass of its own).  The vote workgroups fill a CU each and go out in position order, so the
 * last rounds of a grid are then its lightest workgroups and the CUs run dry together.  A counting sort over
 * REF_ORDER_CLASSES classes of demand, stable (equal classes stay in index order), O(n): the tail has to be light, not
 * sorted.  order is a permutation of 0 .. n-1 whatever keep holds. */
#define REF_ORDER_CLASSES 1024
void oslam_ref_order(const uint32_t *keep, size_t n, uint32_t *order)
{
    uint32_t start[REF_ORDER_CLASSES + 1], top = 0;
    size_t i;
    int c;
    for (i = 0; i < n; i++) if (keep[i] > top) top = keep[i];
    if (top == 0) top = 1;
    memset(start, 0, sizeof start);
    /* class 0 = the heaviest */
    for (i = 0; i < n; i++) start[1 + (REF_ORDER_CLASSES - 1) - (int)((uint64_t)keep[i] * (REF_ORDER_CLASSES - 1) / top)]++;
    for (c = 0; c < REF_ORDER_CLASSES; c++) start[c + 1] += start[c];
    for (i = 0; i < n; i++) order[start[(REF_ORDER_CLASSES - 1) - (int)((uint64_t)keep[i] * (REF_ORDER_CLASSES - 1) / top)]++] = (uint32_t)i;
}

/* The kernels of one registration (or of one reference point for the accumulator tap): count, then per
 * batch scene keys -> hit sort -> votes.  d_ref_idx / d_tsg: the reference points and their frame rows.
 * The caller holds the pool of the device. */
int oslam_run_votes_group(scratch_pool *pool, oslam_model *const *ms, int nm, oslam_scene *s, const uint32_t *d_ref_idx,
                           const float *d_tsg, int n_ref, uint32_t fixed_gmax, uint32_t *acc_dump,
                           oslamk_counters *cnt, float *ms_out, float *ms_vote_kernel, float *ms_key_kernel,
                           uint32_t *launches, uint64_t *probed)
{
    /* ms[0..nm): models that share one union table and d_dist (a database group, or one model): the scene
     * pass -- count, keys, hit sort -- runs once for all of them, then each model votes with its own buckets.
     * cnt[nm]; the vote-kernel time is the sum over the models. */
    oslam_model *m = ms[0];
    int rc = OSLAM_OK, first, nb = 0, i, j;
    oslamk_vote_args a;
    hipStream_t st = (hipStream_t)oslam_stream();
    hipEvent_t *ev;
    const size_t limit_slots = scratch_limit(ms[0]) / SLOT_BYTES;
    size_t cap, max_batch_slots = 0, redo_stride = 0;
    int one_grid = 0;
    /* heaviest reference points first (oslam_params.vote_order); the accumulator tap votes one reference point */
    const int ordered = (m->params.vote_order == 0 || m->params.vote_order == 3) && !acc_dump && n_ref > 1;
    uint32_t *h_keep, *h_off, *d_keep, *d_hitc, *d_runc, *d_off;
    float k0 = 0.0f;
    rc = oslam_pool_reserve_counts(pool, (size_t)(n_ref > 0 ? n_ref : 1));
    if (rc != OSLAM_OK) return rc;
    {
        /* one place per vote workgroup of the largest launch: (reference points padded to 8) x slices */
        size_t nsl = 1, need;
        for (j = 0; j < nm; j++) if ((size_t)ms[j]->table.n_slices > nsl) nsl = (size_t)ms[j]->table.n_slices;
        need = (((size_t)(n_ref > 0 ? n_ref : 1) + 7) / 8 * 8) * nsl;
        redo_stride = need;
        if (nm > 1) need *= (size_t)nm;           /* a group voted in one grid: every member its own list */
        if (pool->redo_cap < need) {
            if (pool->d_redo) { (void)hipFree(pool->d_redo); pool->d_redo = NULL; pool->redo_cap = 0; }
            HIPCHK(hipMalloc((void **)&pool->d_redo, sizeof(uint32_t) * (need + need / 4)));
            pool->redo_cap = need + need / 4;
        }
    }
    if (ordered && pool->order_cap < (size_t)n_ref) {
        const size_t want = (size_t)n_ref + (size_t)n_ref / 4 + 64;
        if (pool->d_order) { (void)hipFree(pool->d_order); pool->d_order = NULL; }
        if (pool->h_order) { (void)hipHostFree(pool->h_order); pool->h_order = NULL; }
        pool->order_cap = 0;
        HIPCHK(hipMalloc((void **)&pool->d_order, sizeof(uint32_t) * want));
        HIPCHK(hipHostMalloc((void **)&pool->h_order, sizeof(uint32_t) * want, hipHostMallocDefault));
        pool->order_cap = want;
    }
    ev = pool->ev;
    cap = pool->counts_cap;
    d_keep = pool->d_counts;
    d_hitc = d_keep + cap;
    d_runc = d_hitc + cap;
    d_off = d_runc + cap;                       /* [2 * cap + 2] */
    h_keep = pool->h_counts;
    h_off = h_keep + cap;
    memset(&a, 0, sizeof a);
    a.scene = s->c.k;
    a.ref_idx = d_ref_idx;
    a.tsg = d_tsg;
    a.n_ref = n_ref;
    a.d_dist = m->d_dist;
    a.inv_d_dist = m->inv_d_dist;
    a.table = m->table;
    a.ent = m->ent;
    a.thresh = m->params.vote_count_threshold;
    a.fixed_gmax = fixed_gmax;
    a.counters = m->d_counters;
    a.out = m->d_out;
    a.out_cap = m->out_cap;
    a.acc_dump = acc_dump;
    a.dump_ref = acc_dump ? 0 : -1;
    a.mode = (m->params.vote_mode == OSLAM_VOTE_FAST) ? 1 : 0;
    for (j = 0; j < nm; j++) HIPCHK(hipMemsetAsync(ms[j]->d_counters, 0, sizeof(oslamk_counters), st));
    HIPCHK(hipEventRecord(ev[0], st));
    /* 1. demand: pairs within reach, per reference point */
    if (n_ref > 0) {
        HIPCHK(hipMemsetAsync(d_keep, 0, sizeof(uint32_t) * (size_t)n_ref, st));
        a.first_ref = 0;
        a.n_launch = n_ref;
        a.keep_count = d_keep;
        KCHK(oslamk_scene_count(&a, oslam_stream()));
        HIPCHK(hipEventRecord(ev[2], st));
        HIPCHK(hipMemcpyAsync(h_keep, d_keep, sizeof(uint32_t) * (size_t)n_ref, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipEventElapsedTime(&k0, ev[0], ev[2]));
        if (ms_key_kernel) *ms_key_kernel += k0;
        if (probed) {
            uint64_t t = 0;
            for (i = 0; i < n_ref; i++) t += h_keep[i];
            *probed = t;
        }
    }
    /* 2. batches that fit the pool; the offsets of every batch start at 0.  h_off holds, batch after
     * batch, the n + 1 offsets of its n reference points */
    {
        size_t pos = 0;
        for (first = 0; first < n_ref;) {
            size_t slots;
            const int n = batch_extent(h_keep, first, n_ref, limit_slots, h_off + pos, &slots);
            if (slots > max_batch_slots) max_batch_slots = slots;
            pos += (size_t)n + 1;
            first += n;
        }
        rc = pool_reserve_slots(pool, max_batch_slots, scratch_limit(ms[0]));
        if (rc != OSLAM_OK) goto done;
        if (pos) HIPCHK(hipMemcpyAsync(d_off, h_off, sizeof(uint32_t) * pos, hipMemcpyHostToDevice, st));
    }
    /* A group whose frame is one batch votes in ONE grid (k_vote_group): fifty small models are fifty grids of little
     * more than one round of workgroups otherwise, each with its own tail and its own three launches. */
    if (nm > 1 && n_ref > 0 && !acc_dump) {
        size_t slots;
        size_t nsl = 1;
        for (j = 0; j < nm; j++) if ((size_t)ms[j]->table.n_slices > nsl) nsl = (size_t)ms[j]->table.n_slices;
        /* ... where it pays: members whose own grid is a few rounds of workgroups at most.  A member with tens of
         * thousands of workgroups fills the chip by itself, and the kernel that takes its arguments from memory keeps
         * more of them in registers than the one that gets them as kernel arguments (10 x 5000 points against 100k:
         * 342 ms in one grid, 313 ms in ten). */
        one_grid = batch_extent(h_keep, 0, n_ref, limit_slots, NULL, &slots) == n_ref &&
                   ((size_t)n_ref + 7) / 8 * 8 * nsl <= 2048;
        for (j = 1; j < nm && one_grid; j++)
            if ((ms[j]->params.vote_mode == OSLAM_VOTE_FAST) != (ms[0]->params.vote_mode == OSLAM_VOTE_FAST)) one_grid = 0;
        if (one_grid && pool->vargs_cap < (size_t)nm) {
            const size_t want = (size_t)nm + (size_t)nm / 2 + 8;
            if (pool->d_vargs) { (void)hipFree(pool->d_vargs); pool->d_vargs = NULL; }
            if (pool->h_vargs) { (void)hipHostFree(pool->h_vargs); pool->h_vargs = NULL; }
            pool->vargs_cap = 0;
            HIPCHK(hipMalloc((void **)&pool->d_vargs, sizeof(oslamk_vote_args) * want));
            HIPCHK(hipHostMalloc((void **)&pool->h_vargs, sizeof(oslamk_vote_args) * want, hipHostMallocDefault));
            pool->vargs_cap = want;
        }
    }
    /* 3. the batches */
    {
        size_t pos = 0;
        for (first = 0; first < n_ref; nb++) {
            const int timed = nb < MAX_BATCH_EVENTS;
            size_t slots;
            const int n = batch_extent(h_keep, first, n_ref, limit_slots, NULL, &slots);
            a.first_ref = first;
            a.n_launch = n;
            a.keep_count = NULL;
            a.hit_off = d_off + pos;
            a.hit_count = d_hitc;
            a.run_count = d_runc;
            carve_scratch(&a, pool, slots);
            HIPCHK(hipMemsetAsync(d_hitc, 0, sizeof(uint32_t) * (size_t)n, st));
            if (timed) HIPCHK(hipEventRecord(ev[4 + 3 * nb], st));
            KCHK(oslamk_scene_hits(&a, oslam_stream()));
            KCHK(oslamk_sort_hits(&a, oslam_stream()));
            if (timed) HIPCHK(hipEventRecord(ev[4 + 3 * nb + 1], st));
            a.ref_order = NULL;
            if (ordered) {
                /* made while the two kernels above run; every batch has its own piece of the pinned buffer, which
                 * nothing writes again before the call's last wait */
                oslam_ref_order(h_keep + first, (size_t)n, pool->h_order + first);
                HIPCHK(hipMemcpyAsync(pool->d_order + first, pool->h_order + first, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
                a.ref_order = pool->d_order + first;
            }
            for (j = 0; j < nm; j++) {
                const oslam_model *mj = ms[j];
                a.table.uinfo = mj->table.uinfo;          /* its buckets, under the shared union slots */
                a.table.n_slices = mj->table.n_slices;
                a.table.slots = mj->table.slots;
                a.table.cap = mj->table.cap;
                a.ent = mj->ent;
                a.thresh = mj->params.vote_count_threshold;
                a.counters = mj->d_counters;
                a.out = mj->d_out;
                a.out_cap = mj->out_cap;
                a.mode = (mj->params.vote_mode == OSLAM_VOTE_FAST) ? 1 : 0;
                if (one_grid) {
                    a.redo = pool->d_redo + (size_t)j * redo_stride;
                    pool->h_vargs[j] = a;
                    continue;
                }
                KCHK(oslamk_vote(&a, oslam_stream()));
                /* the redo list belongs to this launch */
                HIPCHK(hipMemsetAsync(&mj->d_counters->redo_count, 0, sizeof(uint32_t), st));
            }
            if (one_grid) {
                HIPCHK(hipMemcpyAsync(pool->d_vargs, pool->h_vargs, sizeof(oslamk_vote_args) * (size_t)nm, hipMemcpyHostToDevice, st));
                KCHK(oslamk_vote_group(pool->d_vargs, pool->h_vargs, nm, oslam_stream()));
            }
            if (timed) HIPCHK(hipEventRecord(ev[4 + 3 * nb + 2], st));
            if (launches) *launches += 1;
            pos += (size_t)n + 1;
            first += n;
        }
    }
    HIPCHK(hipEventRecord(ev[1], st));
    for (j = 0; j < nm; j++) HIPCHK(hipMemcpyAsync(&cnt[j], ms[j]->d_counters, sizeof *cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (one_grid) {
        /* the one-grid launch leaves the re-vote of workgroups whose 16-bit counters overflowed to here: a member that
         * has any (large planes in a small model: next to never) gets its two passes now and its counters again */
        int again = 0;
        for (j = 0; j < nm; j++)
            if (cnt[j].redo_count) {
                KCHK(oslamk_vote_wide(&pool->h_vargs[j], oslam_stream()));
                HIPCHK(hipMemcpyAsync(&cnt[j], ms[j]->d_counters, sizeof *cnt, hipMemcpyDeviceToHost, st));
                again = 1;
            }
        if (again) HIPCHK(hipStreamSynchronize(st));
    }
    for (j = 0; j < nm; j++)
        if (cnt[j].list_overflow) {
            rc = fail(OSLAM_E_DEVICE, cnt[j].list_overflow & 1u
                          ? "a hit list overflowed: the counting pass and the hit pass disagreed on the pairs within reach"
                          : cnt[j].list_overflow & 2u ? "near-edge search: a hit's key number lies outside the model's bucket records"
                          : cnt[j].list_overflow & 4u ? "near-edge search: a bucket lies outside the model's entry arrays"
                                                      : "near-edge search: a directory place lies outside its bucket segment");
            goto done;
        }
    if (ms_out) HIPCHK(hipEventElapsedTime(ms_out, ev[0], ev[1]));
    for (i = 0; i < nb && i < MAX_BATCH_EVENTS; i++) {
        float k = 0.0f, v = 0.0f;
        HIPCHK(hipEventElapsedTime(&k, ev[4 + 3 * i], ev[4 + 3 * i + 1]));
        HIPCHK(hipEventElapsedTime(&v, ev[4 + 3 * i + 1], ev[4 + 3 * i + 2]));
        if (ms_key_kernel) *ms_key_kernel += k;
        if (ms_vote_kernel) *ms_vote_kernel += v;
    }
done:
    return rc;
}

static int run_votes(scratch_pool *pool, oslam_model *m, oslam_scene *s, uint32_t fixed_gmax, oslamk_counters *cnt,
                     float *ms_out, float *ms_vote_kernel, float *ms_key_kernel, uint32_t *launches, uint64_t *probed)
{
    return oslam_run_votes_group(pool, &m, 1, s, s->d_ref_idx, s->d_tsg, s->n_ref, fixed_gmax, NULL, cnt, ms_out, ms_vote_kernel,
                                 ms_key_kernel, launches, probed);
}

/* record buffers (device and host) for at least `need` records; the contents are dropped */
int oslam_grow_records(oslam_model *m, uint64_t need)
{
    oslamk_cell *d_new = NULL;
    oslam_cell *h_new;
    if (need > ((uint64_t)1 << 28)) return fail(OSLAM_E_LIMIT, "more than 2^28 accumulator peaks above the threshold");
    if (hipMalloc((void **)&d_new, sizeof(oslamk_cell) * need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OSLAM_E_NOMEM, "no device memory for the accumulator peaks");
    }
    h_new = (oslam_cell *)malloc(sizeof(oslam_cell) * need);
    if (!h_new) { (void)hipFree(d_new); return fail(OSLAM_E_NOMEM, "host allocation failed"); }
    (void)hipFree(m->d_out);
    free(m->h_out);
    m->d_out = d_new;
    m->h_out = h_new;
    m->out_cap = (uint32_t)need;
    m->n_local = 0;
    return OSLAM_OK;
}

/* the statistics of one model's votes: its counters, and the times, launches and probes of the pass they came from */
void oslam_vote_stats(oslam_stats *st, const scratch_pool *pool, const oslam_model *m, const oslam_scene *s,
                      const oslamk_counters *cnt, float ms_vote, float ms_vote_kernel, float ms_key_kernel,
                      uint32_t launches, uint64_t probed)
{
    st->num_scene_ppfs = (uint64_t)s->n_ref * (uint64_t)(s->c.n - 1);
    st->num_hits = cnt->hits;
    st->num_votes = cnt->votes;
    st->num_unique_votes = cnt->nonzero_cells;
    st->num_model_keys = m->num_model_keys;
    st->max_count = cnt->gmax;
    st->num_emitted = cnt->out_count;
    st->ms_vote = ms_vote;
    st->ms_vote_kernel = ms_vote_kernel;
    st->ms_key_kernel = ms_key_kernel;
    st->vote_launches = launches;
    st->num_pairs_probed = probed;
    st->num_entries_streamed = cnt->entries;
    st->num_items = cnt->items;
    st->wide_workgroups = cnt->redo_total;
    st->scratch_bytes = pool->bytes;
}

/* The votes of one model: *n_cells records in m->d_out, and in m->h_out too when to_host is set.  An overflowing
 * record buffer takes a second, exactly thresholded launch. */
int oslam_vote_records(scratch_pool *pool, oslam_model *m, oslam_scene *s, oslamk_counters *cnt, size_t *n_cells,
                       oslam_stats *st, int to_host)
{
    int rc = OSLAM_OK;
    float ms = 0.0f, ms2 = 0.0f, msv = 0.0f, msk = 0.0f;
    uint32_t launches = 0;
    uint64_t probed = 0;
    rc = run_votes(pool, m, s, 0, cnt, &ms, &msv, &msk, &launches, &probed);
    if (rc != OSLAM_OK) return rc;
    if (cnt->out_count > m->out_cap) {
        uint32_t g = cnt->gmax;
        rc = run_votes(pool, m, s, g, cnt, &ms2, &msv, &msk, &launches, &probed);
        if (rc != OSLAM_OK) return rc;
        cnt->gmax = g;
        if (cnt->out_count > m->out_cap) {
            /* even the exactly thresholded set is larger than the record buffer: the count is known now, so
             * the buffers grow to it (up to 2^28 records = 4 GiB) and the launch is repeated */
            rc = oslam_grow_records(m, (uint64_t)cnt->out_count + cnt->out_count / 8 + 1024);
            if (rc != OSLAM_OK) return rc;
            rc = run_votes(pool, m, s, g, cnt, &ms2, &msv, &msk, &launches, &probed);
            if (rc != OSLAM_OK) return rc;
            cnt->gmax = g;
            if (cnt->out_count > m->out_cap)
                return fail(OSLAM_E_LIMIT, "more accumulator peaks than the record buffer after growing it");
        }
    }
    if (getenv("OSLAM_PROF"))      /* only a -DVOTE_PROF build fills these */
        fprintf(stderr, "[oslam prof] k_vote wave cycles: pre-scan %llu, voting %llu, wait at the barrier behind it %llu, "
                        "of the voting: near-edge search %llu\n",
                cnt->prof[0], cnt->prof[1], cnt->prof[2], cnt->prof[3]);
    *n_cells = cnt->out_count;
    if (to_host && *n_cells) HIPCHK(hipMemcpy(m->h_out, m->d_out, sizeof(oslam_cell) * *n_cells, hipMemcpyDeviceToHost));
    if (st) oslam_vote_stats(st, pool, m, s, cnt, ms + ms2, msv, msk, launches, probed);
done:
    return rc;
}

/* clustering scores on the bound device (see oslam_pose.h); any failure makes the host loop run */
int oslam_cluster_scores_on_device(size_t n, const float *trans, const float *quat, const float *wv,
                                    const int32_t *cell, const uint32_t *hash_idx, float d_dist, int use_l1,
                                    float *score)
{
    int rc = OSLAM_OK;
    char *d = NULL, *h = NULL;
    /* pose order: cell [n][3]; sorted order: hash [n], pose index [n], quat, trans, votes; out: score (pose order) */
    const size_t o_c = 0, o_sh = o_c + 12 * n, o_si = o_sh + 4 * n, o_sq = o_si + 4 * n,
                 o_st = o_sq + 16 * n, o_sw = o_st + 12 * n, o_sc = o_sw + 4 * n, o_tab = o_sc + 4 * n,
                 total = o_tab + 4 * oslamk_cluster_table_words((int)n);
    size_t j;
    int whole = 1;
    uint64_t whole_sum = 0;
    hipStream_t st = (hipStream_t)oslam_stream();
    h = (char *)malloc(o_sc);
    if (!h) return OSLAM_E_NOMEM;
    memcpy(h + o_c, cell, 12 * n);
    for (j = 0; j < n; j++) {
        const uint32_t o = hash_idx[2 * j + 1];
        ((uint32_t *)(h + o_sh))[j] = hash_idx[2 * j];
        ((uint32_t *)(h + o_si))[j] = o;
        memcpy(h + o_sq + 16 * j, quat + 4 * o, 16);
        memcpy(h + o_st + 12 * j, trans + 3 * o, 12);
        ((float *)(h + o_sw))[j] = wv[o];
        /* whole numbers with a sum below 2^24: any order of adding them gives the same float (oslamk_cluster_scores) */
        if (whole && wv[o] >= 0.0f && wv[o] < 16777216.0f && wv[o] == (float)(uint32_t)wv[o]) whole_sum += (uint32_t)wv[o];
        else whole = 0;
    }
    if (whole_sum >= (1u << 24) - 1u) whole = 0;
    /* persistent workspace in the device's pool (the caller holds its lock) */
    if (!g_cur_pool) { rc = OSLAM_E_DEVICE; goto done; }
    if (g_cur_pool->cluster_bytes < total) {
        if (g_cur_pool->d_cluster) (void)hipFree(g_cur_pool->d_cluster);
        g_cur_pool->d_cluster = NULL;
        g_cur_pool->cluster_bytes = 0;
        HIPCHK(hipMalloc((void **)&g_cur_pool->d_cluster, total + total / 4));
        g_cur_pool->cluster_bytes = total + total / 4;
    }
    d = g_cur_pool->d_cluster;
    HIPCHK(hipMemcpyAsync(d, h, o_sc, hipMemcpyHostToDevice, st));
    KCHK(oslamk_cluster_scores((int)n, (const int *)(d + o_c), (const uint32_t *)(d + o_sh), (const uint32_t *)(d + o_si),
                               (const float *)(d + o_sq), (const float *)(d + o_st),
                               (const float *)(d + o_sw), d_dist, use_l1, (float *)(d + o_sc), whole, NULL, (uint32_t *)(d + o_tab), oslam_stream()));
    HIPCHK(hipMemcpyAsync(score, d + o_sc, 4 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
done:
    free(h);
    return rc;
}
