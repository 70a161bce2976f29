/*
 * oslam_vote_plan.h -- how the reference points of one registration are cut into batches whose hit lists fit the
 * scratch pool: the rule, once, and the one walk that applies it.  Host only, static inline, no HIP and no error
 * text: tests/native/vote_plan_check.c includes it alone and holds the plan to a literal copy of the walk it replaced.
 *
 * keep[r] is the demand of reference point r (its pairs within reach, k_scene_count).  A list gets its count rounded
 * up to even, so that every list starts 8-byte aligned in the 4-byte key array too.  A batch takes reference points
 * while their lists fit limit_slots places and OSLAM_BATCH_SLOTS_MAX (offsets are 32 bits), and at least one: a
 * reference point that needs more than the limit is a batch of its own.
 */
#ifndef OSLAM_VOTE_PLAN_H
#define OSLAM_VOTE_PLAN_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#define OSLAM_BATCH_SLOTS_MAX 0xfffffff0u

typedef struct oslam_vote_batch {
    int first, n;                     /* reference points first .. first + n - 1 */
    size_t slots;                     /* places of its lists together */
    size_t off_at;                    /* its n + 1 offsets are off[off_at ..] */
} oslam_vote_batch;

typedef struct oslam_vote_plan {
    oslam_vote_batch *b;              /* [nb], in order; storage for cap batches that is kept between plans */
    int nb, cap;
    size_t n_off;                     /* offsets written: batch after batch the n + 1 of its n reference points, from 0 */
    size_t max_slots;                 /* the largest batch */
} oslam_vote_plan;

/* The rule: the batch that starts at reference point `first`.  off receives its n + 1 offsets, *slots its total. */
static inline int oslam_vote_batch_extent(const uint32_t *keep, int first, int n_ref, size_t limit_slots, uint32_t *off,
                                          size_t *slots)
{
    size_t t = 0;
    int n = 0;
    while (first + n < n_ref) {
        const size_t need = ((size_t)keep[first + n] + 1u) & ~(size_t)1u;
        if (n > 0 && (t + need > limit_slots || t + need > OSLAM_BATCH_SLOTS_MAX)) break;
        off[n] = (uint32_t)t;
        t += need;
        n++;
    }
    off[n] = (uint32_t)t;
    *slots = t;
    return n;
}

/* The walk: the batches of n_ref reference points into *p, their offsets into off[n_ref + batches] (at most 2 * n_ref).
 * 0, or -1 without memory for the batch records (the plan is empty then). */
static inline int oslam_vote_plan_build(oslam_vote_plan *p, const uint32_t *keep, int n_ref, size_t limit_slots, uint32_t *off)
{
    int first = 0;
    p->nb = 0;
    p->n_off = 0;
    p->max_slots = 0;
    while (first < n_ref) {
        oslam_vote_batch *b;
        if (p->nb == p->cap) {
            const int cap = p->cap ? 2 * p->cap : 4;
            oslam_vote_batch *grown = (oslam_vote_batch *)realloc(p->b, sizeof *grown * (size_t)cap);
            if (!grown) { p->nb = 0; p->n_off = 0; p->max_slots = 0; return -1; }
            p->b = grown;
            p->cap = cap;
        }
        b = &p->b[p->nb++];
        b->first = first;
        b->off_at = p->n_off;
        b->n = oslam_vote_batch_extent(keep, first, n_ref, limit_slots, off + p->n_off, &b->slots);
        if (b->slots > p->max_slots) p->max_slots = b->slots;
        p->n_off += (size_t)b->n + 1;
        first += b->n;
    }
    return 0;
}

/* the whole frame is one batch */
static inline int oslam_vote_plan_is_one_batch(const oslam_vote_plan *p) { return p->nb == 1; }

#endif /* OSLAM_VOTE_PLAN_H */
