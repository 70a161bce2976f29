/*
 * oslam_world.h -- the voxel store as oslam_window.c uses it (semantics: include/oslam.h at oslam_volume_shift_world;
 * the store itself: oslam_world.c).  Nothing here needs a device: the staging buffers are kept as plain pointers with
 * the function that frees them, both given by the caller that allocated them.
 */
#ifndef OSLAM_WORLD_H
#define OSLAM_WORLD_H

#include <stddef.h>
#include <stdint.h>

#include "oslam.h"

/* records the text for oslam_last_error and returns code (oslam_host.c) */
int oslam_fail(int code, const char *what);

#define OSLAM_WORLD_G_MAX ((1 << 20) + 512)   /* the largest |g_a| a window within the shift's limits can hold */

/* a pinned buffer the shift keeps with the store: bytes grows on demand, release frees p (set with it) */
typedef struct oslam_world_stage {
    void *p;
    size_t bytes;
    void (*release)(void *p);
} oslam_world_stage;

/* The calls below are made between oslam_world_lock and oslam_world_unlock, with the volume lock held. */
void oslam_world_lock(oslam_world *w);
void oslam_world_unlock(oslam_world *w);
/* the store was made for these float bits */
int oslam_world_compatible(const oslam_world *w, float voxel, const float origin0[3]);
/* the two staging buffers: [0] the records that leave, [1] the records that enter */
oslam_world_stage *oslam_world_stages(oslam_world *w);
/* the table's capacity, to be given to oslam_world_rollback */
size_t oslam_world_mark(const oslam_world *w);
/* makes the brick of g exist (empty when new): OSLAM_OK, OSLAM_E_LIMIT (max_bytes) or OSLAM_E_NOMEM */
int oslam_world_reserve(oslam_world *w, const int32_t g[3]);
/* frees every empty brick and takes the table back to the capacity it had at the mark */
void oslam_world_rollback(oslam_world *w, size_t mark);
/* stores a seen word under g, whose brick exists (oslam_world_reserve): cannot fail.  On a colour store the colour word
 * goes in next to it as it is (oslam_world_store: 0); a plain store drops it */
void oslam_world_store(oslam_world *w, const int32_t g[3], uint32_t word);
void oslam_world_store_colour(oslam_world *w, const int32_t g[3], uint32_t word, uint32_t colour);
/* the store's bricks carry colour words (oslam_world_params.colour) */
int oslam_world_coloured(const oslam_world *w);
/* calls fn(ctx, g, word) for every stored word with lo <= g < hi; take != 0 removes them and frees the bricks that
 * become empty.  -> the number of words visited */
typedef void (*oslam_world_visit_fn)(void *ctx, const int32_t g[3], uint32_t word);
size_t oslam_world_visit(oslam_world *w, const int32_t lo[3], const int32_t hi[3], int take, oslam_world_visit_fn fn, void *ctx);
/* the same visit, handing out the colour word stored with each word too (0 on a plain store) */
typedef void (*oslam_world_visit_colour_fn)(void *ctx, const int32_t g[3], uint32_t word, uint32_t colour);
size_t oslam_world_visit_colour(oslam_world *w, const int32_t lo[3], const int32_t hi[3], int take, oslam_world_visit_colour_fn fn,
                                void *ctx);
/* the float bits the store was made for */
void oslam_world_frame(const oslam_world *w, float *voxel, float origin0[3]);
/* the store's bricks for the extraction of the whole map (oslam_world_surface.c): how many; their keys floor(g / 8) as
 * keys_out [count][3], ascending by (bz, by, bx); the 512 words [z][y][x] of the brick with this key (NULL without one),
 * valid until the store changes */
size_t oslam_world_brick_count(const oslam_world *w);
void oslam_world_brick_keys(const oslam_world *w, int32_t *keys_out);
const uint32_t *oslam_world_brick_words(const oslam_world *w, const int32_t key[3]);
/* the 512 colour words of that brick, laid out as its words: NULL without the brick or on a plain store */
const uint32_t *oslam_world_brick_colours(const oslam_world *w, const int32_t key[3]);

#endif /* OSLAM_WORLD_H */
