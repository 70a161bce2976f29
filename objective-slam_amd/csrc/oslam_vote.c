/*
 * oslam_vote.c -- the votes of one registration: the scratch pool of each device, the batches of reference
 * points, the kernels of the scene pass and the votes, the record buffers, and the clustering hook of the
 * pose stage (which works in the pool).
 */
#include <pthread.h>
#include <stdio.h>

#include "oslam_internal.h"
#include "oslam_vote_plan.h"

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
 * pool (oslam_vote_plan.h).  The pool grows to what a call needs, up to OSLAM_SCRATCH_GIB GiB (default 4; a single
 * reference point that needs more still gets it); oslam_release_scratch frees it. */
#define MAX_DEVICES 64
#define MAX_BATCH_EVENTS 64
#define N_EVENTS (4 + 3 * MAX_BATCH_EVENTS)
#define SLOT_BYTES (sizeof(oslamk_pay) * 2 + sizeof(oslamk_run) + sizeof(uint32_t))

/* One grow-only block of the pool: device memory, and for a block that is staged through the host its host twin. */
enum { HOST_NONE, HOST_PINNED, HOST_MALLOC };
typedef struct pool_buf {
    void *d, *h;
    int host;                          /* what h is: one of the above, set once */
    size_t cap;                        /* elements (BUF_HITS, BUF_CLUSTER: bytes) */
} pool_buf;

enum {
    BUF_HITS,                          /* hit arrays of one batch */
    BUF_COUNTS,                        /* d: keep_count[cap], hit_count[cap], run_count[cap], hit_off[2 * cap + 2];
                                          h (pageable): keep counts [cap], then offsets */
    BUF_CLUSTER,                       /* workspace of oslam_cluster_scores_on_device */
    BUF_REDO,                          /* vote workgroups of a batch whose 16-bit counters overflowed */
    BUF_VARGS,                         /* a group's vote arguments, one per member, for the one-grid launch */
    BUF_ORDER,                         /* the order in which a batch's reference points are voted, see oslam_ref_order */
    N_BUFS
};
static const int g_buf_host[N_BUFS] = {HOST_NONE, HOST_MALLOC, HOST_NONE, HOST_NONE, HOST_PINNED, HOST_PINNED};

struct scratch_pool {
    pthread_mutex_t lock;
    pool_buf b[N_BUFS];
    oslam_vote_plan plan;              /* the batches of the pass in flight */
    hipEvent_t ev[N_EVENTS];
    int have_events;
};
static scratch_pool g_pool[MAX_DEVICES];
static pthread_once_t g_pool_once = PTHREAD_ONCE_INIT;

static void pool_init_all(void)
{
    int i, k;
    for (i = 0; i < MAX_DEVICES; i++) {
        pthread_mutex_init(&g_pool[i].lock, NULL);
        for (k = 0; k < N_BUFS; k++) g_pool[i].b[k].host = g_buf_host[k];
    }
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

static void pool_buf_free(pool_buf *b)
{
    if (b->d) (void)hipFree(b->d);
    if (b->h && b->host == HOST_PINNED) (void)hipHostFree(b->h);
    if (b->host == HOST_MALLOC) free(b->h);
    b->d = NULL;
    b->h = NULL;
    b->cap = 0;
}

/* The pool's one grow rule.  Nothing happens while b holds `need` elements; otherwise both blocks are given back and
 * made again for cap elements (need and the caller's head room), d_bytes and h_bytes large.  A failure leaves b empty. */
static int pool_buf_grow(pool_buf *b, size_t need, size_t cap, size_t d_bytes, size_t h_bytes)
{
    int rc = OSLAM_OK;
    if (b->cap >= need) return OSLAM_OK;
    pool_buf_free(b);
    HIPCHK(hipMalloc(&b->d, d_bytes));
    if (b->host == HOST_PINNED) HIPCHK(hipHostMalloc(&b->h, h_bytes, hipHostMallocDefault));
    if (b->host == HOST_MALLOC && !(b->h = malloc(h_bytes))) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    b->cap = cap;
done:
    if (rc != OSLAM_OK) pool_buf_free(b);
    return rc;
}

int oslam_release_scratch(int dev)
{
    scratch_pool *p = pool_lock(dev);
    int i, any;
    if (!p) return fail(OSLAM_E_INVALID, "device ordinal out of range");
    any = p->have_events;
    for (i = 0; i < N_BUFS; i++) any |= p->b[i].d != NULL || p->b[i].h != NULL;
    if (any) {
        if (hipSetDevice(dev) != hipSuccess) { oslam_pool_unlock(p); return fail(OSLAM_E_DEVICE, "hipSetDevice failed"); }
        for (i = 0; i < N_BUFS; i++) pool_buf_free(&p->b[i]);
        oslamk_pose_release();
        if (p->have_events)
            for (i = 0; i < N_EVENTS; i++) (void)hipEventDestroy(p->ev[i]);
        p->have_events = 0;
    }
    if (hipSetDevice(dev) == hipSuccess) oslam_dev_cache_release(dev);   /* the kept blocks of the scene path */
    oslam_arbitrate_release();
    oslam_track_release();
    oslam_ego_release();
    free(p->plan.b);
    memset(&p->plan, 0, sizeof p->plan);
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
    /* offsets: one more than reference points per batch; a batch holds at least one reference point */
    const size_t cap = n_ref + n_ref / 4 + 64;
    if (!p->have_events) {
        for (i = 0; i < N_EVENTS; i++) HIPCHK(hipEventCreate(&p->ev[i]));
        p->have_events = 1;
    }
    rc = pool_buf_grow(&p->b[BUF_COUNTS], n_ref, cap, sizeof(uint32_t) * (5 * cap + 2), sizeof(uint32_t) * (3 * cap + 2));
done:
    return rc;
}

/* The hit lists' own rule, on the same record (its cap is bytes, and what oslam_stats.scratch_bytes reports): head room
 * of an eighth, clamped to the limit but never below what the batch needs, and a second try without head room. */
static int pool_reserve_slots(scratch_pool *p, size_t slots, size_t limit)
{
    pool_buf *b = &p->b[BUF_HITS];
    const size_t base = (slots ? slots : 1) * SLOT_BYTES + 1024;      /* + a wave of hits: the vote kernel loads 64 at a time */
    size_t want = base;
    if (b->cap >= want) return OSLAM_OK;
    pool_buf_free(b);
    want += want / 8;                 /* head room: the next scene is rarely the same size */
    /* batches are cut to the limit: no head room beyond it, but never less than the batch itself needs (a pool
     * below `base` would be freed and mapped again by every registration) */
    if (want > limit + 1024) want = base > limit + 1024 ? base : limit + 1024;
    if (hipMalloc(&b->d, want) != hipSuccess) {
        (void)hipGetLastError();
        b->d = NULL;
        want = base;
        if (hipMalloc(&b->d, want) != hipSuccess) {
            (void)hipGetLastError();
            b->d = NULL;
            return fail(OSLAM_E_NOMEM, "no device memory for the hit lists");
        }
    }
    b->cap = want;
    return OSLAM_OK;
}

/* the arrays of a batch with `slots` places inside the pool */
static void carve_scratch(oslamk_vote_args *a, const scratch_pool *p, size_t slots)
{
    char *b = (char *)p->b[BUF_HITS].d;
    a->redo = (uint32_t *)p->b[BUF_REDO].d;
    a->hit_pay = (oslamk_pay *)b;
    b += slots * sizeof(oslamk_pay);
    a->hit_sorted = (oslamk_pay *)b;
    b += slots * sizeof(oslamk_pay);
    a->runs = (oslamk_run *)b;
    b += slots * sizeof(oslamk_run);
    a->hit_key = (uint32_t *)b;
}

/* Parity tap: the sorted hit list of the pass that just ran in the pool with ONE reference point (oslam_run_votes_group,
 * waited for): per hit the key's number, theta_v (oslamk_pay.theta_t22) and the scene index, at most cap of each, *n_out
 * = the number of hits; *keep_out = the reference point's demand (k_scene_count).  The caller holds the pool. */
int oslam_pool_read_hits(const scratch_pool *p, uint32_t *numbers_out, uint32_t *theta_out, uint32_t *idx_out, size_t cap,
                         size_t *n_out, uint32_t *keep_out)
{
    int rc = OSLAM_OK;
    oslamk_vote_args a;
    oslamk_pay *pay = NULL;
    uint32_t n = 0;
    size_t i, m;
    *n_out = 0;
    if (keep_out) *keep_out = ((const uint32_t *)p->b[BUF_COUNTS].h)[0];
    if (p->plan.nb < 1) return OSLAM_OK;             /* no pair within reach: no batch, no list */
    carve_scratch(&a, p, p->plan.b[0].slots);
    HIPCHK(hipMemcpy(&n, (const uint32_t *)p->b[BUF_COUNTS].d + p->b[BUF_COUNTS].cap, sizeof n, hipMemcpyDeviceToHost));
    *n_out = n;
    m = n < cap ? n : cap;
    if (!m) return OSLAM_OK;
    pay = (oslamk_pay *)malloc(sizeof *pay * m);
    if (!pay) return fail(OSLAM_E_NOMEM, "host allocation failed");
    HIPCHK(hipMemcpy(pay, a.hit_sorted, sizeof *pay * m, hipMemcpyDeviceToHost));
    if (numbers_out) {
        HIPCHK(hipMemcpy(numbers_out, a.hit_key, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
        for (i = 0; i < m; i++) numbers_out[i] &= 0x7fffffffu;        /* bit 31: the run holds a marker */
    }
    for (i = 0; i < m; i++) {
        if (theta_out) theta_out[i] = pay[i].theta_t22;
        if (idx_out) idx_out[i] = pay[i].idx;
    }
done:
    free(pay);
    return rc;
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
 * batch scene keys -> hit sort -> votes, as the stages below.  What they share: */
typedef struct vote_pass {
    scratch_pool *pool;               /* held by the caller */
    oslam_model *const *ms;           /* ms[0..nm): models that share one union table and d_dist (a database group, or one) */
    int nm, n_ref;
    hipStream_t st;
    oslamk_vote_args a;               /* the scene's part, and the part of the member that voted last (ms[0] at first) */
    uint32_t *d_keep, *d_hitc, *d_runc, *d_off, *h_keep, *h_off;   /* the pool's counts, cut */
    size_t limit;                     /* of the hit lists, bytes */
    size_t widest;                    /* the largest n_slices of the members */
    size_t redo_stride;               /* places of one member's redo list */
    int ordered;                      /* heaviest reference points first (oslam_params.vote_order) */
    int one_grid;                     /* after pass_reserve: may; after pass_plan: does vote in one grid */
} vote_pass;

/* the part of the vote arguments that is a member's own: its buckets under the shared union slots, its outputs */
static void member_args(oslamk_vote_args *a, const oslam_model *m)
{
    a->table.uinfo = m->table.uinfo;
    a->table.n_slices = m->table.n_slices;
    a->table.slots = m->table.slots;
    a->table.cap = m->table.cap;
    a->ent = m->ent;
    a->thresh = m->params.vote_count_threshold;
    a->counters = m->d_counters;
    a->out = m->d_out;
    a->out_cap = m->out_cap;
    a->mode = (m->params.vote_mode == OSLAM_VOTE_FAST) ? 1 : 0;
}

static void pass_open(vote_pass *v, scratch_pool *pool, oslam_model *const *ms, int nm, const oslam_scene *s,
                      const uint32_t *d_ref_idx, const float *d_tsg, int n_ref, uint32_t fixed_gmax, uint32_t *acc_dump)
{
    int j;
    memset(v, 0, sizeof *v);
    v->pool = pool;
    v->ms = ms;
    v->nm = nm;
    v->n_ref = n_ref;
    v->st = (hipStream_t)oslam_stream();
    v->limit = scratch_limit(ms[0]);
    v->widest = 1;
    for (j = 0; j < nm; j++) if ((size_t)ms[j]->table.n_slices > v->widest) v->widest = (size_t)ms[j]->table.n_slices;
    /* the accumulator tap votes one reference point */
    v->ordered = (ms[0]->params.vote_order == 0 || ms[0]->params.vote_order == 3) && !acc_dump && n_ref > 1;
    /* A group whose frame is one batch (pass_plan) votes in ONE grid (k_vote_group): fifty small models are fifty grids
     * of little more than one round of workgroups otherwise, each with its own tail and its own three launches --
     * where it pays: members whose own grid is a few rounds of workgroups at most.  A member with tens of thousands of
     * workgroups fills the chip by itself, and the kernel that takes its arguments from memory keeps more of them in
     * registers than the one that gets them as kernel arguments (10 x 5000 points against 100k: 342 ms in one grid,
     * 313 ms in ten). */
    v->one_grid = nm > 1 && n_ref > 0 && !acc_dump && ((size_t)n_ref + 7) / 8 * 8 * v->widest <= 2048;
    for (j = 1; j < nm && v->one_grid; j++)
        if ((ms[j]->params.vote_mode == OSLAM_VOTE_FAST) != (ms[0]->params.vote_mode == OSLAM_VOTE_FAST)) v->one_grid = 0;
    v->a.scene = s->c.k;
    v->a.order = s->order;
    v->a.ref_idx = d_ref_idx;
    v->a.tsg = d_tsg;
    v->a.n_ref = n_ref;
    v->a.d_dist = ms[0]->d_dist;
    v->a.inv_d_dist = ms[0]->inv_d_dist;
    v->a.table = ms[0]->table;
    v->a.fixed_gmax = fixed_gmax;
    v->a.acc_dump = acc_dump;
    v->a.dump_ref = acc_dump ? 0 : -1;
    member_args(&v->a, ms[0]);
}

/* Stage 1: the pool's blocks that depend on the number of reference points and members */
static int pass_reserve(vote_pass *v)
{
    scratch_pool *pool = v->pool;
    const size_t n = (size_t)(v->n_ref > 0 ? v->n_ref : 1), nm = (size_t)v->nm;
    size_t need, cap;
    int rc = oslam_pool_reserve_counts(pool, n);
    if (rc != OSLAM_OK) return rc;
    /* one place per vote workgroup of the largest launch: (reference points padded to 8) x slices */
    need = v->redo_stride = (n + 7) / 8 * 8 * v->widest;
    if (nm > 1) need *= nm;                      /* a group voted in one grid: every member its own list */
    cap = need + need / 4;
    rc = pool_buf_grow(&pool->b[BUF_REDO], need, cap, sizeof(uint32_t) * cap, 0);
    if (rc != OSLAM_OK) return rc;
    if (v->ordered) {
        cap = n + n / 4 + 64;
        rc = pool_buf_grow(&pool->b[BUF_ORDER], n, cap, sizeof(uint32_t) * cap, sizeof(uint32_t) * cap);
        if (rc != OSLAM_OK) return rc;
    }
    if (v->one_grid) {
        cap = nm + nm / 2 + 8;
        rc = pool_buf_grow(&pool->b[BUF_VARGS], nm, cap, sizeof(oslamk_vote_args) * cap, sizeof(oslamk_vote_args) * cap);
        if (rc != OSLAM_OK) return rc;
    }
    cap = pool->b[BUF_COUNTS].cap;
    v->d_keep = (uint32_t *)pool->b[BUF_COUNTS].d;
    v->d_hitc = v->d_keep + cap;
    v->d_runc = v->d_hitc + cap;
    v->d_off = v->d_runc + cap;                  /* [2 * cap + 2] */
    v->h_keep = (uint32_t *)pool->b[BUF_COUNTS].h;
    v->h_off = v->h_keep + cap;
    return OSLAM_OK;
}

/* Stage 2, the demand: pairs within reach, per reference point, counted and brought to the host (which waits) */
static int pass_demand(vote_pass *v, oslam_vote_times *t)
{
    int rc = OSLAM_OK, i;
    hipEvent_t *ev = v->pool->ev;
    float k0 = 0.0f;
    uint64_t sum = 0;
    if (v->n_ref <= 0) return OSLAM_OK;
    HIPCHK(hipMemsetAsync(v->d_keep, 0, sizeof(uint32_t) * (size_t)v->n_ref, v->st));
    v->a.first_ref = 0;
    v->a.n_launch = v->n_ref;
    v->a.keep_count = v->d_keep;
    KCHK(oslamk_scene_count(&v->a, oslam_stream()));
    HIPCHK(hipEventRecord(ev[2], v->st));
    HIPCHK(hipMemcpyAsync(v->h_keep, v->d_keep, sizeof(uint32_t) * (size_t)v->n_ref, hipMemcpyDeviceToHost, v->st));
    HIPCHK(hipStreamSynchronize(v->st));
    HIPCHK(hipEventElapsedTime(&k0, ev[0], ev[2]));
    if (t) {
        for (i = 0; i < v->n_ref; i++) sum += v->h_keep[i];
        t->ms_key_kernel += k0;
        t->probed = sum;
    }
done:
    return rc;
}

/* Stage 3: the batches that fit the pool (the one walk of oslam_vote_plan.h), the hit lists for the largest of them,
 * the offsets of all of them to the device, and whether a group votes in one grid */
static int pass_plan(vote_pass *v)
{
    oslam_vote_plan *plan = &v->pool->plan;
    int rc = OSLAM_OK;
    if (oslam_vote_plan_build(plan, v->h_keep, v->n_ref, v->limit / SLOT_BYTES, v->h_off) != 0)
        return fail(OSLAM_E_NOMEM, "host allocation failed");
    rc = pool_reserve_slots(v->pool, plan->max_slots, v->limit);
    if (rc != OSLAM_OK) return rc;
    if (plan->n_off) HIPCHK(hipMemcpyAsync(v->d_off, v->h_off, sizeof(uint32_t) * plan->n_off, hipMemcpyHostToDevice, v->st));
    v->one_grid = v->one_grid && oslam_vote_plan_is_one_batch(plan);
done:
    return rc;
}

/* Stage 4, one batch: scene keys -> hit lists, their sort, the order of its reference points, and the votes of every
 * member from the same lists -- a launch each, or all in one grid */
static int pass_batch(vote_pass *v, int nb)
{
    scratch_pool *pool = v->pool;
    const oslam_vote_batch *b = &pool->plan.b[nb];
    oslamk_vote_args *a = &v->a, *d_vargs = (oslamk_vote_args *)pool->b[BUF_VARGS].d, *h_vargs = (oslamk_vote_args *)pool->b[BUF_VARGS].h;
    hipEvent_t *ev = nb < MAX_BATCH_EVENTS ? pool->ev + 4 + 3 * nb : NULL;       /* the first batches are timed */
    int rc = OSLAM_OK, j;
    a->first_ref = b->first;
    a->n_launch = b->n;
    a->keep_count = NULL;
    a->hit_off = v->d_off + b->off_at;
    a->hit_count = v->d_hitc;
    a->run_count = v->d_runc;
    carve_scratch(a, pool, b->slots);
    HIPCHK(hipMemsetAsync(v->d_hitc, 0, sizeof(uint32_t) * (size_t)b->n, v->st));
    if (ev) HIPCHK(hipEventRecord(ev[0], v->st));
    KCHK(oslamk_scene_hits(a, oslam_stream()));
    KCHK(oslamk_sort_hits(a, oslam_stream()));
    if (ev) HIPCHK(hipEventRecord(ev[1], v->st));
    a->ref_order = NULL;
    if (v->ordered) {
        /* made while the two kernels above run; every batch has its own piece of the pinned buffer, which
         * nothing writes again before the call's last wait */
        uint32_t *d_order = (uint32_t *)pool->b[BUF_ORDER].d + b->first, *h_order = (uint32_t *)pool->b[BUF_ORDER].h + b->first;
        oslam_ref_order(v->h_keep + b->first, (size_t)b->n, h_order);
        HIPCHK(hipMemcpyAsync(d_order, h_order, sizeof(uint32_t) * (size_t)b->n, hipMemcpyHostToDevice, v->st));
        a->ref_order = d_order;
    }
    for (j = 0; j < v->nm; j++) {
        member_args(a, v->ms[j]);
        if (v->one_grid) {
            a->redo = (uint32_t *)pool->b[BUF_REDO].d + (size_t)j * v->redo_stride;
            h_vargs[j] = *a;
            continue;
        }
        KCHK(oslamk_vote(a, oslam_stream()));
        /* the redo list belongs to this launch */
        HIPCHK(hipMemsetAsync(&v->ms[j]->d_counters->redo_count, 0, sizeof(uint32_t), v->st));
    }
    if (v->one_grid) {
        HIPCHK(hipMemcpyAsync(d_vargs, h_vargs, sizeof(oslamk_vote_args) * (size_t)v->nm, hipMemcpyHostToDevice, v->st));
        KCHK(oslamk_vote_group(d_vargs, h_vargs, v->nm, oslam_stream()));
    }
    if (ev) HIPCHK(hipEventRecord(ev[2], v->st));
done:
    return rc;
}

/* Stage 5: every member's counters on the host (which waits), the wide re-vote that a one-grid launch leaves to here,
 * the errors the kernels flagged, and the times of the pass */
static int pass_collect(vote_pass *v, oslamk_counters *cnt, oslam_vote_times *t)
{
    scratch_pool *pool = v->pool;
    const oslamk_vote_args *h_vargs = (const oslamk_vote_args *)pool->b[BUF_VARGS].h;
    hipEvent_t *ev = pool->ev;
    int rc = OSLAM_OK, i, j, again = 0;
    HIPCHK(hipEventRecord(ev[1], v->st));
    for (j = 0; j < v->nm; j++) HIPCHK(hipMemcpyAsync(&cnt[j], v->ms[j]->d_counters, sizeof *cnt, hipMemcpyDeviceToHost, v->st));
    HIPCHK(hipStreamSynchronize(v->st));
    /* a member of a one-grid launch with workgroups whose 16-bit counters overflowed (large planes in a small model:
     * next to never) gets its two passes now and its counters again */
    for (j = 0; j < v->nm && v->one_grid; j++)
        if (cnt[j].redo_count) {
            KCHK(oslamk_vote_wide(&h_vargs[j], oslam_stream()));
            HIPCHK(hipMemcpyAsync(&cnt[j], v->ms[j]->d_counters, sizeof *cnt, hipMemcpyDeviceToHost, v->st));
            again = 1;
        }
    if (again) HIPCHK(hipStreamSynchronize(v->st));
    for (j = 0; j < v->nm; j++)
        if (cnt[j].list_overflow)
            return fail(OSLAM_E_DEVICE, cnt[j].list_overflow & 1u
                            ? "a hit list overflowed: the counting pass and the hit pass disagreed on the pairs within reach"
                            : cnt[j].list_overflow & 2u ? "near-edge search: a hit's key number lies outside the model's bucket records"
                            : cnt[j].list_overflow & 4u ? "near-edge search: a bucket lies outside the model's entry arrays"
                                                        : "near-edge search: a directory place lies outside its bucket segment");
    if (!t) return OSLAM_OK;
    HIPCHK(hipEventElapsedTime(&t->ms, ev[0], ev[1]));
    for (i = 0; i < pool->plan.nb && i < MAX_BATCH_EVENTS; i++) {
        float k = 0.0f, vk = 0.0f;
        HIPCHK(hipEventElapsedTime(&k, ev[4 + 3 * i], ev[4 + 3 * i + 1]));
        HIPCHK(hipEventElapsedTime(&vk, ev[4 + 3 * i + 1], ev[4 + 3 * i + 2]));
        t->ms_key_kernel += k;
        t->ms_vote_kernel += vk;
    }
    t->launches += (uint32_t)pool->plan.nb;
done:
    return rc;
}

/* The scene pass -- count, keys, hit sort -- runs once for all of ms[0..nm), then each model votes with its own buckets.
 * d_ref_idx / d_tsg: the reference points and their frame rows.  cnt[nm]; t (may be NULL) receives what the pass
 * reports, its kernel times summed over the models.  The caller holds the pool of the device. */
int oslam_run_votes_group(scratch_pool *pool, oslam_model *const *ms, int nm, oslam_scene *s, const uint32_t *d_ref_idx,
                          const float *d_tsg, int n_ref, uint32_t fixed_gmax, uint32_t *acc_dump, oslamk_counters *cnt,
                          oslam_vote_times *t)
{
    vote_pass v;
    int rc = OSLAM_OK, j, nb;
    pass_open(&v, pool, ms, nm, s, d_ref_idx, d_tsg, n_ref, fixed_gmax, acc_dump);
    rc = pass_reserve(&v);
    if (rc != OSLAM_OK) return rc;
    for (j = 0; j < nm; j++) HIPCHK(hipMemsetAsync(ms[j]->d_counters, 0, sizeof(oslamk_counters), v.st));
    HIPCHK(hipEventRecord(pool->ev[0], v.st));
    rc = pass_demand(&v, t);
    if (rc == OSLAM_OK) rc = pass_plan(&v);
    for (nb = 0; rc == OSLAM_OK && nb < pool->plan.nb; nb++) rc = pass_batch(&v, nb);
    if (rc == OSLAM_OK) rc = pass_collect(&v, cnt, t);
done:
    return rc;
}

/* one pass of one model; fixed_gmax != 0: a further pass, exactly thresholded at the first one's maximum */
static int run_votes(scratch_pool *pool, oslam_model *m, oslam_scene *s, uint32_t fixed_gmax, oslamk_counters *cnt,
                     oslam_vote_times *t)
{
    const int rc = oslam_run_votes_group(pool, &m, 1, s, s->d_ref_idx, s->d_tsg, s->n_ref, fixed_gmax, NULL, cnt, t);
    if (rc == OSLAM_OK && fixed_gmax) cnt->gmax = fixed_gmax;
    return rc;
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
                      const oslamk_counters *cnt, const oslam_vote_times *t)
{
    st->num_scene_ppfs = (uint64_t)s->n_ref * (uint64_t)(s->c.n - 1);
    st->num_hits = cnt->hits;
    st->num_votes = cnt->votes;
    st->num_unique_votes = cnt->nonzero_cells;
    st->num_model_keys = m->num_model_keys;
    st->max_count = cnt->gmax;
    st->num_emitted = cnt->out_count;
    st->ms_vote = t->ms;
    st->ms_vote_kernel = t->ms_vote_kernel;
    st->ms_key_kernel = t->ms_key_kernel;
    st->vote_launches = t->launches;
    st->num_pairs_probed = t->probed;
    st->num_entries_streamed = cnt->entries;
    st->num_items = cnt->items;
    st->wide_workgroups = cnt->redo_total;
    st->scratch_bytes = pool->b[BUF_HITS].cap;
}

/* The votes of one model: *n_cells records in m->d_out, and in m->h_out too when to_host is set.  An overflowing
 * record buffer takes a second, exactly thresholded launch. */
int oslam_vote_records(scratch_pool *pool, oslam_model *m, oslam_scene *s, oslamk_counters *cnt, size_t *n_cells,
                       oslam_stats *st, int to_host)
{
    int rc = OSLAM_OK;
    oslam_vote_times t;
    float ms_first;
    memset(&t, 0, sizeof t);
    rc = run_votes(pool, m, s, 0, cnt, &t);
    if (rc != OSLAM_OK) return rc;
    /* a pass sets t.ms and adds to the rest: ms_vote is the first pass and the last */
    ms_first = t.ms;
    t.ms = 0.0f;
    if (cnt->out_count > m->out_cap) {
        const uint32_t g = cnt->gmax;
        rc = run_votes(pool, m, s, g, cnt, &t);
        if (rc != OSLAM_OK) return rc;
        if (cnt->out_count > m->out_cap) {
            /* even the exactly thresholded set is larger than the record buffer: the count is known now, so
             * the buffers grow to it (up to 2^28 records = 4 GiB) and the launch is repeated */
            rc = oslam_grow_records(m, (uint64_t)cnt->out_count + cnt->out_count / 8 + 1024);
            if (rc == OSLAM_OK) rc = run_votes(pool, m, s, g, cnt, &t);
            if (rc != OSLAM_OK) return rc;
            if (cnt->out_count > m->out_cap)
                return fail(OSLAM_E_LIMIT, "more accumulator peaks than the record buffer after growing it");
        }
    }
    t.ms += ms_first;
    if (getenv("OSLAM_PROF"))      /* only a -DVOTE_PROF build fills these */
        fprintf(stderr, "[oslam prof] k_vote wave cycles: pre-scan %llu, voting %llu, wait at the barrier behind it %llu, "
                        "of the voting: near-edge search %llu\n",
                cnt->prof[0], cnt->prof[1], cnt->prof[2], cnt->prof[3]);
    *n_cells = cnt->out_count;
    if (to_host && *n_cells) HIPCHK(hipMemcpy(m->h_out, m->d_out, sizeof(oslam_cell) * *n_cells, hipMemcpyDeviceToHost));
    if (st) oslam_vote_stats(st, pool, m, s, cnt, &t);
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
    rc = pool_buf_grow(&g_cur_pool->b[BUF_CLUSTER], total, total + total / 4, total + total / 4, 0);
    if (rc != OSLAM_OK) goto done;
    d = (char *)g_cur_pool->b[BUF_CLUSTER].d;
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
