/*
 * oslam_world.c -- the voxel store: a host-side map from global voxel coordinates to TSDF words that keeps what leaves a
 * volume's shifting window until the window returns (include/oslam.h at oslam_volume_shift_world; the shift that uses
 * it: oslam_volume.c; its view of the store: oslam_world.h).  Bricks of 8 x 8 x 8 words, keyed by floor(g / 8) per axis,
 * in a table with linear probing that doubles when half full; removal shifts the following entries back, so there are
 * no tombstones and a lookup that misses stops at the first empty slot.  Every stored word is seen (w > 0), so a zero
 * word in a brick means "nothing stored".  A colour store's bricks carry a second array of 512 colour words, each kept
 * under its g as it is whenever the TSDF word is stored and cleared with it.  The bricks' keys in ascending order, for the extraction of the whole map's
 * surface (oslam_world_surface.c), are made here too.  No device call and no HIP header: this file links alone.
 */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "oslam_world.h"

#define BRICK_SIDE 8
#define BRICK_WORDS (BRICK_SIDE * BRICK_SIDE * BRICK_SIDE)
#define TABLE_MIN 64                          /* slots of an empty store; a power of two */
#define WORLD_DEFAULT_BYTES ((uint64_t)1 << 30)
#define WORLD_BOX_MAX ((uint64_t)1 << 27)     /* voxels of one oslam_world_box */
#define WORLD_COORD_MAX (1 << 21)             /* |lo_a|, |hi_a| of a box: no difference of two leaves int */
#define NO_SLOT ((size_t)-1)

typedef struct brick {
    int32_t key[3];                           /* floor(g_a / 8) */
    uint32_t count;                           /* words != 0 */
    uint32_t words[BRICK_WORDS];              /* [z][y][x] */
    uint32_t colours[];                       /* [BRICK_WORDS] in a colour store, absent otherwise */
} brick;

struct oslam_world {
    pthread_mutex_t mu;
    float voxel, origin0[3];
    uint64_t max_bytes;
    int colour;                               /* the bricks carry colours[] */
    brick **slots;                            /* [cap], NULL = empty */
    size_t cap, n_bricks;                     /* cap a power of two, n_bricks * 2 <= cap */
    uint64_t n_voxels;
    oslam_world_stage stage[2];
};

static size_t slot_of(const int32_t key[3], size_t cap)
{
    uint64_t h = (uint64_t)(uint32_t)key[0] * 0x9e3779b97f4a7c15ull;
    h ^= (uint64_t)(uint32_t)key[1] * 0xc2b2ae3d27d4eb4full;
    h ^= (uint64_t)(uint32_t)key[2] * 0x165667b19e3779f9ull;
    h ^= h >> 29;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 32;
    return (size_t)h & (cap - 1);
}

static int same_key(const brick *b, const int32_t key[3]) { return b->key[0] == key[0] && b->key[1] == key[1] && b->key[2] == key[2]; }

static size_t brick_bytes(const oslam_world *w) { return sizeof(brick) + (w->colour ? BRICK_WORDS * sizeof(uint32_t) : 0); }

static uint64_t bytes_of(const oslam_world *w, size_t n_bricks, size_t cap)
{
    return (uint64_t)n_bricks * brick_bytes(w) + (uint64_t)cap * sizeof(brick *);
}

static size_t table_find(const oslam_world *w, const int32_t key[3])
{
    size_t s = slot_of(key, w->cap);
    while (w->slots[s]) {
        if (same_key(w->slots[s], key)) return s;
        s = (s + 1) & (w->cap - 1);
    }
    return NO_SLOT;
}

static void table_insert(brick **slots, size_t cap, brick *b)
{
    size_t s = slot_of(b->key, cap);
    while (slots[s]) s = (s + 1) & (cap - 1);
    slots[s] = b;
}

/* 0, or -1 when the new slots cannot be allocated (the table is then as it was); cap >= 2 * n_bricks */
static int table_resize(oslam_world *w, size_t cap)
{
    size_t s;
    brick **slots = (brick **)calloc(cap, sizeof *slots);
    if (!slots) return -1;
    for (s = 0; s < w->cap; s++)
        if (w->slots[s]) table_insert(slots, cap, w->slots[s]);
    free(w->slots);
    w->slots = slots;
    w->cap = cap;
    return 0;
}

/* frees the brick in slot s and moves the entries behind it back, so that every probe sequence stays gap-free */
static void table_remove(oslam_world *w, size_t s)
{
    size_t hole = s, j = s;
    free(w->slots[s]);
    w->slots[s] = NULL;
    w->n_bricks--;
    for (;;) {
        size_t home;
        j = (j + 1) & (w->cap - 1);
        if (!w->slots[j]) return;
        home = slot_of(w->slots[j]->key, w->cap);
        /* the entry at j may move into the hole iff its home is not cyclically inside (hole, j] */
        if (((j - home) & (w->cap - 1)) >= ((j - hole) & (w->cap - 1))) {
            w->slots[hole] = w->slots[j];
            w->slots[j] = NULL;
            hole = j;
        }
    }
}

/* frees every empty brick.  A removal moves entries only into slots at or behind the one examined (cyclically), and
 * the slot examined is examined again, so no empty brick is passed over */
static void sweep_empty(oslam_world *w)
{
    size_t s = 0;
    while (s < w->cap) {
        if (w->slots[s] && w->slots[s]->count == 0) table_remove(w, s);
        else s++;
    }
}

static void key_of(const int32_t g[3], int32_t key[3], unsigned *local)
{
    int a;
    unsigned l[3];
    for (a = 0; a < 3; a++) {
        key[a] = g[a] >> 3;                   /* arithmetic: floor for a negative g */
        l[a] = (unsigned)(g[a] - key[a] * BRICK_SIDE);
    }
    *local = (l[2] * BRICK_SIDE + l[1]) * BRICK_SIDE + l[0];
}

/* ---- what oslam_volume.c uses (oslam_world.h) ---- */
void oslam_world_lock(oslam_world *w) { pthread_mutex_lock(&w->mu); }
void oslam_world_unlock(oslam_world *w) { pthread_mutex_unlock(&w->mu); }

int oslam_world_compatible(const oslam_world *w, float voxel, const float origin0[3])
{
    return memcmp(&w->voxel, &voxel, sizeof voxel) == 0 && memcmp(w->origin0, origin0, sizeof w->origin0) == 0;
}

oslam_world_stage *oslam_world_stages(oslam_world *w) { return w->stage; }

size_t oslam_world_mark(const oslam_world *w) { return w->cap; }

int oslam_world_reserve(oslam_world *w, const int32_t g[3])
{
    int32_t key[3];
    unsigned local;
    size_t cap = w->cap;
    brick *b;
    key_of(g, key, &local);
    if (table_find(w, key) != NO_SLOT) return OSLAM_OK;
    if ((w->n_bricks + 1) * 2 > cap) cap *= 2;
    if (bytes_of(w, w->n_bricks + 1, cap) > w->max_bytes) return oslam_fail(OSLAM_E_LIMIT, "the voxel store's max_bytes is exceeded");
    b = (brick *)calloc(1, brick_bytes(w));
    if (!b || (cap != w->cap && table_resize(w, cap) != 0)) {
        free(b);
        return oslam_fail(OSLAM_E_NOMEM, "host allocation failed");
    }
    memcpy(b->key, key, sizeof key);
    table_insert(w->slots, w->cap, b);
    w->n_bricks++;
    return OSLAM_OK;
}

void oslam_world_rollback(oslam_world *w, size_t mark)
{
    sweep_empty(w);
    if (w->cap != mark && w->n_bricks * 2 <= mark) (void)table_resize(w, mark);
}

void oslam_world_store(oslam_world *w, const int32_t g[3], uint32_t word) { oslam_world_store_colour(w, g, word, 0u); }

int oslam_world_coloured(const oslam_world *w) { return w->colour; }

void oslam_world_store_colour(oslam_world *w, const int32_t g[3], uint32_t word, uint32_t colour)
{
    int32_t key[3];
    unsigned local;
    brick *b;
    key_of(g, key, &local);
    b = w->slots[table_find(w, key)];
    if (b->words[local] == 0u) {
        b->count++;
        w->n_voxels++;
    }
    b->words[local] = word;
    if (w->colour) b->colours[local] = colour;
}

static int imax(int a, int b) { return a > b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }

/* the words of b inside the box; -> how many */
static size_t visit_brick(oslam_world *w, brick *b, const int32_t lo[3], const int32_t hi[3], int take,
                          oslam_world_visit_colour_fn fn, void *ctx)
{
    int a, x, y, z, c0[3], c1[3];
    size_t n = 0;
    for (a = 0; a < 3; a++) {
        const int base = b->key[a] * BRICK_SIDE;
        c0[a] = imax(lo[a], base) - base;
        c1[a] = imin(hi[a], base + BRICK_SIDE) - base;
        if (c0[a] >= c1[a]) return 0;
    }
    for (z = c0[2]; z < c1[2]; z++)
        for (y = c0[1]; y < c1[1]; y++)
            for (x = c0[0]; x < c1[0]; x++) {
                const int local = (z * BRICK_SIDE + y) * BRICK_SIDE + x;
                uint32_t *p = &b->words[local];
                if (*p == 0u) continue;
                {
                    const int32_t g[3] = {b->key[0] * BRICK_SIDE + x, b->key[1] * BRICK_SIDE + y, b->key[2] * BRICK_SIDE + z};
                    if (fn) fn(ctx, g, *p, w->colour ? b->colours[local] : 0u);
                }
                n++;
                if (take) {
                    *p = 0u;
                    if (w->colour) b->colours[local] = 0u;
                    b->count--;
                    w->n_voxels--;
                }
            }
    return n;
}

typedef struct plain_visit {
    oslam_world_visit_fn fn;
    void *ctx;
} plain_visit;

static void visit_plain(void *ctx, const int32_t g[3], uint32_t word, uint32_t colour)
{
    const plain_visit *p = (const plain_visit *)ctx;
    (void)colour;
    p->fn(p->ctx, g, word);
}

size_t oslam_world_visit(oslam_world *w, const int32_t lo[3], const int32_t hi[3], int take, oslam_world_visit_fn fn, void *ctx)
{
    plain_visit p;
    p.fn = fn;
    p.ctx = ctx;
    return oslam_world_visit_colour(w, lo, hi, take, fn ? visit_plain : NULL, &p);
}

size_t oslam_world_visit_colour(oslam_world *w, const int32_t lo[3], const int32_t hi[3], int take, oslam_world_visit_colour_fn fn,
                                void *ctx)
{
    int a;
    int32_t k0[3], k1[3], key[3];
    uint64_t range = 1;
    size_t n = 0, s;
    if (w->n_bricks == 0) return 0;
    for (a = 0; a < 3; a++) {
        if (lo[a] >= hi[a]) return 0;
        k0[a] = lo[a] >> 3;
        k1[a] = (hi[a] - 1) >> 3;
        range *= (uint64_t)(k1[a] - k0[a] + 1);
    }
    if (range <= (uint64_t)w->cap) {
        /* fewer bricks in the box than slots in the table: look each one up */
        for (key[2] = k0[2]; key[2] <= k1[2]; key[2]++)
            for (key[1] = k0[1]; key[1] <= k1[1]; key[1]++)
                for (key[0] = k0[0]; key[0] <= k1[0]; key[0]++) {
                    s = table_find(w, key);
                    if (s == NO_SLOT) continue;
                    n += visit_brick(w, w->slots[s], lo, hi, take, fn, ctx);
                    if (take && w->slots[s]->count == 0) table_remove(w, s);
                }
    } else {
        int emptied = 0;
        for (s = 0; s < w->cap; s++)
            if (w->slots[s]) {
                n += visit_brick(w, w->slots[s], lo, hi, take, fn, ctx);
                emptied |= take && w->slots[s]->count == 0;
            }
        if (emptied) sweep_empty(w);
    }
    return n;
}

/* ---- the public calls (include/oslam.h) ---- */
int oslam_world_create(const oslam_world_params *p, oslam_world **out)
{
    oslam_world *w;
    if (out) *out = NULL;
    if (!p || !out) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    if (!isfinite(p->voxel) || !isfinite(p->origin0[0]) || !isfinite(p->origin0[1]) || !isfinite(p->origin0[2]))
        return oslam_fail(OSLAM_E_INVALID, "voxel and origin0 must be finite");
    if (!(p->voxel > 0.0f)) return oslam_fail(OSLAM_E_INVALID, "voxel must be > 0");
    if (p->colour != 0 && p->colour != 1) return oslam_fail(OSLAM_E_INVALID, "colour must be 0 or 1");
    w = (oslam_world *)calloc(1, sizeof *w);
    if (!w) return oslam_fail(OSLAM_E_NOMEM, "host allocation failed");
    w->slots = (brick **)calloc(TABLE_MIN, sizeof *w->slots);
    if (!w->slots) {
        free(w);
        return oslam_fail(OSLAM_E_NOMEM, "host allocation failed");
    }
    w->cap = TABLE_MIN;
    w->voxel = p->voxel;
    memcpy(w->origin0, p->origin0, sizeof w->origin0);
    w->max_bytes = p->max_bytes ? p->max_bytes : WORLD_DEFAULT_BYTES;
    w->colour = p->colour;
    pthread_mutex_init(&w->mu, NULL);
    *out = w;
    return OSLAM_OK;
}

static void drop_bricks(oslam_world *w)
{
    size_t s;
    for (s = 0; s < w->cap; s++) {
        free(w->slots[s]);
        w->slots[s] = NULL;
    }
    w->n_bricks = 0;
    w->n_voxels = 0;
}

int oslam_world_destroy(oslam_world *w)
{
    int k;
    if (!w) return oslam_fail(OSLAM_E_INVALID, "world is NULL");
    drop_bricks(w);
    free(w->slots);
    for (k = 0; k < 2; k++)
        if (w->stage[k].p && w->stage[k].release) w->stage[k].release(w->stage[k].p);
    pthread_mutex_destroy(&w->mu);
    free(w);
    return OSLAM_OK;
}

int oslam_world_clear(oslam_world *w)
{
    if (!w) return oslam_fail(OSLAM_E_INVALID, "world is NULL");
    pthread_mutex_lock(&w->mu);
    drop_bricks(w);
    if (w->cap != TABLE_MIN) (void)table_resize(w, TABLE_MIN);
    pthread_mutex_unlock(&w->mu);
    return OSLAM_OK;
}

int oslam_world_stats_get(oslam_world *w, oslam_world_stats *out)
{
    size_t s;
    int a, x, y, z, any = 0;
    if (!w || !out) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    memset(out, 0, sizeof *out);
    pthread_mutex_lock(&w->mu);
    out->voxels = w->n_voxels;
    out->bricks = w->n_bricks;
    out->bytes = bytes_of(w, w->n_bricks, w->cap);
    for (s = 0; s < w->cap; s++) {
        const brick *b = w->slots[s];
        if (!b) continue;
        for (z = 0; z < BRICK_SIDE; z++)
            for (y = 0; y < BRICK_SIDE; y++)
                for (x = 0; x < BRICK_SIDE; x++) {
                    const int32_t g[3] = {b->key[0] * BRICK_SIDE + x, b->key[1] * BRICK_SIDE + y, b->key[2] * BRICK_SIDE + z};
                    if (b->words[(z * BRICK_SIDE + y) * BRICK_SIDE + x] == 0u) continue;
                    for (a = 0; a < 3; a++) {
                        if (!any || g[a] < out->lo[a]) out->lo[a] = g[a];
                        if (!any || g[a] + 1 > out->hi[a]) out->hi[a] = g[a] + 1;
                    }
                    any = 1;
                }
    }
    pthread_mutex_unlock(&w->mu);
    return OSLAM_OK;
}

int oslam_world_has_colour(const oslam_world *w) { return w && w->colour; }

/* colours == NULL: colour 0 */
static int put(oslam_world *w, const int32_t *g, const uint32_t *words, const uint32_t *colours, size_t n)
{
    int rc = OSLAM_OK;
    size_t i, mark;
    for (i = 0; i < 3 * n; i++)
        if (g[i] < -OSLAM_WORLD_G_MAX || g[i] > OSLAM_WORLD_G_MAX)
            return oslam_fail(OSLAM_E_INVALID, "a global voxel coordinate is at most 2^20 + 512 in size");
    pthread_mutex_lock(&w->mu);
    mark = oslam_world_mark(w);
    for (i = 0; i < n && rc == OSLAM_OK; i++)
        if (words[i] >> 16) rc = oslam_world_reserve(w, g + 3 * i);
    if (rc != OSLAM_OK) oslam_world_rollback(w, mark);
    else
        for (i = 0; i < n; i++)
            if (words[i] >> 16) oslam_world_store_colour(w, g + 3 * i, words[i], colours ? colours[i] : 0u);
    pthread_mutex_unlock(&w->mu);
    return rc;
}

int oslam_world_put(oslam_world *w, const int32_t *g, const uint32_t *words, size_t n)
{
    if (!w || (n && (!g || !words))) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    return put(w, g, words, NULL, n);
}

int oslam_world_put_colour(oslam_world *w, const int32_t *g, const uint32_t *words, const uint32_t *colours, size_t n)
{
    if (!w || (n && (!g || !words || !colours))) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    if (!w->colour) return oslam_fail(OSLAM_E_INVALID, "the voxel store keeps no colour");
    return put(w, g, words, colours, n);
}

typedef struct dense_ctx {
    uint32_t *out, *colours;                  /* colours may be NULL */
    int32_t lo[3];
    size_t nx, ny;
} dense_ctx;

static void dense_write(void *ctx, const int32_t g[3], uint32_t word, uint32_t colour)
{
    const dense_ctx *d = (const dense_ctx *)ctx;
    const size_t at = ((size_t)(g[2] - d->lo[2]) * d->ny + (size_t)(g[1] - d->lo[1])) * d->nx + (size_t)(g[0] - d->lo[0]);
    d->out[at] = word;
    if (d->colours) d->colours[at] = colour;
}

static int box(oslam_world *w, const int32_t lo[3], const int32_t hi[3], uint32_t *words_out, uint32_t *colours_out, int want_colours,
               int take)
{
    int a;
    uint64_t n = 1;
    dense_ctx d;
    if (!w || !lo || !hi) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    for (a = 0; a < 3; a++) {
        if (lo[a] > hi[a] || lo[a] < -WORLD_COORD_MAX || hi[a] > WORLD_COORD_MAX)
            return oslam_fail(OSLAM_E_INVALID, "a box needs lo <= hi, both at most 2^21 in size");
        n *= (uint64_t)(hi[a] - lo[a]);       /* each factor below 2^23 */
        if (n > WORLD_BOX_MAX) return oslam_fail(OSLAM_E_LIMIT, "a box holds at most 2^27 voxels");
    }
    if (n == 0) return OSLAM_OK;
    if (!words_out || (want_colours && !colours_out)) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    memset(words_out, 0, (size_t)n * sizeof *words_out);
    if (want_colours) memset(colours_out, 0, (size_t)n * sizeof *colours_out);
    d.out = words_out;
    d.colours = want_colours ? colours_out : NULL;
    memcpy(d.lo, lo, sizeof d.lo);
    d.nx = (size_t)(hi[0] - lo[0]);
    d.ny = (size_t)(hi[1] - lo[1]);
    pthread_mutex_lock(&w->mu);
    (void)oslam_world_visit_colour(w, lo, hi, take, dense_write, &d);
    pthread_mutex_unlock(&w->mu);
    return OSLAM_OK;
}

int oslam_world_box(oslam_world *w, const int32_t lo[3], const int32_t hi[3], uint32_t *words_out, int take)
{
    return box(w, lo, hi, words_out, NULL, 0, take);
}

int oslam_world_box_colour(oslam_world *w, const int32_t lo[3], const int32_t hi[3], uint32_t *words_out, uint32_t *colours_out,
                           int take)
{
    if (!w) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    if (!w->colour) return oslam_fail(OSLAM_E_INVALID, "the voxel store keeps no colour");
    return box(w, lo, hi, words_out, colours_out, 1, take);
}

/* ---- brick enumeration (include/oslam.h at oslam_world_surface; its device side: oslam_world_surface.c) ---- */
static int key_cmp(const void *pa, const void *pb)
{
    const int32_t *a = (const int32_t *)pa, *b = (const int32_t *)pb;
    int c;
    for (c = 2; c >= 0; c--)
        if (a[c] != b[c]) return a[c] < b[c] ? -1 : 1;
    return 0;
}

void oslam_world_frame(const oslam_world *w, float *voxel, float origin0[3])
{
    *voxel = w->voxel;
    memcpy(origin0, w->origin0, sizeof w->origin0);
}

size_t oslam_world_brick_count(const oslam_world *w) { return w->n_bricks; }

void oslam_world_brick_keys(const oslam_world *w, int32_t *keys_out)
{
    size_t s, n = 0;
    for (s = 0; s < w->cap; s++)
        if (w->slots[s]) memcpy(keys_out + 3 * n++, w->slots[s]->key, sizeof w->slots[s]->key);
    qsort(keys_out, n, 3 * sizeof *keys_out, key_cmp);
}

const uint32_t *oslam_world_brick_words(const oslam_world *w, const int32_t key[3])
{
    const size_t s = table_find(w, key);
    return s == NO_SLOT ? NULL : w->slots[s]->words;
}

const uint32_t *oslam_world_brick_colours(const oslam_world *w, const int32_t key[3])
{
    const size_t s = table_find(w, key);
    return s == NO_SLOT || !w->colour ? NULL : w->slots[s]->colours;
}

int oslam_world_bricks(oslam_world *w, int32_t *keys_out, size_t cap, size_t *n_out)
{
    int rc = OSLAM_OK;
    if (!w || !n_out) return oslam_fail(OSLAM_E_INVALID, "NULL argument");
    if (!keys_out && cap != 0) return oslam_fail(OSLAM_E_INVALID, "cap must be 0 without an output");
    pthread_mutex_lock(&w->mu);
    *n_out = w->n_bricks;
    if (keys_out && w->n_bricks > cap) rc = oslam_fail(OSLAM_E_LIMIT, "output capacity too small");
    else if (keys_out) oslam_world_brick_keys(w, keys_out);
    pthread_mutex_unlock(&w->mu);
    return rc;
}
