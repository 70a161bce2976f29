/*
 * vote_plan_check.c -- csrc/oslam_vote_plan.h included alone and held to the walk it replaced.  Built and run by
 * tests/test_vote_plan_host.py, once with the library's flags and once under the address and undefined-behaviour
 * sanitizers.  old_batch_extent is a literal copy of oslam_vote.c's batch_extent before the header existed, and
 * old_walk the loop that oslam_run_votes_group ran over it; they are the statement of the contract, so they stay as
 * they are when the header changes.  Exit status 0 and "vote_plan_check ok" when every comparison holds.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oslam_vote_plan.h"

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "vote_plan_check: line %d: %s\n", __LINE__, #c);      \
            return 1;                                                             \
        }                                                                         \
    } while (0)

/* ---- the rule as it stood ---- */
static int old_batch_extent(const uint32_t *keep, int first, int n_ref, size_t limit_slots, uint32_t *off, size_t *slots)
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

typedef struct old_batch {
    int first, n;
    size_t slots, pos;
} old_batch;

/* the walk as it stood: batch after batch, the offsets of each at h_off + pos; the number of batches */
static int old_walk(const uint32_t *keep, int n_ref, size_t limit_slots, uint32_t *h_off, old_batch *b, size_t *n_off,
                    size_t *max_batch_slots)
{
    size_t pos = 0;
    int first, nb = 0;
    *max_batch_slots = 0;
    for (first = 0; first < n_ref; nb++) {
        size_t slots;
        const int n = old_batch_extent(keep, first, n_ref, limit_slots, h_off + pos, &slots);
        if (slots > *max_batch_slots) *max_batch_slots = slots;
        b[nb].first = first;
        b[nb].n = n;
        b[nb].slots = slots;
        b[nb].pos = pos;
        pos += (size_t)n + 1;
        first += n;
    }
    *n_off = pos;
    return nb;
}

/* ---- one demand vector: the plan against the old walk, and what holds of every plan ---- */
static oslam_vote_plan g_plan;            /* one plan for all the vectors, as the pool keeps one: its storage is reused */

static int check_vector(const uint32_t *keep, int n_ref, size_t limit)
{
    const size_t cap = 2 * (size_t)(n_ref > 0 ? n_ref : 1) + 2;
    uint32_t *off_old = (uint32_t *)malloc(sizeof(uint32_t) * cap), *off_new = (uint32_t *)malloc(sizeof(uint32_t) * cap);
    old_batch *ob = (old_batch *)malloc(sizeof *ob * (size_t)(n_ref > 0 ? n_ref : 1));
    size_t n_off = 0, max_slots = 0, slots0 = 0, i;
    int nb, k, next = 0, rc = 1;
    if (!off_old || !off_new || !ob) goto done;
    memset(off_old, 0xab, sizeof(uint32_t) * cap);
    memset(off_new, 0xab, sizeof(uint32_t) * cap);
    nb = old_walk(keep, n_ref, limit, off_old, ob, &n_off, &max_slots);
    if (oslam_vote_plan_build(&g_plan, keep, n_ref, limit, off_new) != 0) goto done;
    rc = 0;
#define VCHECK(c) do { if (!(c)) { fprintf(stderr, "vote_plan_check: line %d: %s (n_ref %d, limit %zu)\n", __LINE__, #c, n_ref, limit); rc = 1; goto done; } } while (0)
    VCHECK(g_plan.nb == nb);
    VCHECK(g_plan.n_off == n_off && n_off == (size_t)(n_ref > 0 ? n_ref : 0) + (size_t)nb);
    VCHECK(g_plan.max_slots == max_slots);
    /* all the offsets, in h_off's layout; nothing is written behind them */
    VCHECK(memcmp(off_old, off_new, sizeof(uint32_t) * cap) == 0);
    for (k = 0; k < nb; k++) {
        const oslam_vote_batch *b = &g_plan.b[k];
        VCHECK(b->first == ob[k].first && b->n == ob[k].n && b->slots == ob[k].slots && b->off_at == ob[k].pos);
        /* the batches tile [0, n_ref) in order without a gap, and hold at least one reference point */
        VCHECK(b->first == next && b->n >= 1);
        next += b->n;
        VCHECK(b->off_at == (size_t)b->first + (size_t)k);
        VCHECK(off_new[b->off_at] == 0 && off_new[b->off_at + (size_t)b->n] == (uint32_t)b->slots);
        /* a batch exceeds the limits only when it holds one reference point */
        VCHECK((b->slots <= limit && b->slots <= OSLAM_BATCH_SLOTS_MAX) || b->n == 1);
    }
    VCHECK(next == (n_ref > 0 ? n_ref : 0));
    for (i = 0; i < n_off; i++) VCHECK((off_new[i] & 1u) == 0);
    /* the one-grid test as it stood: the batch from 0 is the whole frame */
    VCHECK(oslam_vote_plan_is_one_batch(&g_plan) == (n_ref > 0 && old_batch_extent(keep, 0, n_ref, limit, NULL, &slots0) == n_ref));
done:
    free(off_old);
    free(off_new);
    free(ob);
    return rc;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

int main(void)
{
    static uint32_t keep[4096];
    int n, trial;
    size_t limit;
    /* no reference point, one, all-zero demands */
    CHECK(check_vector(keep, 0, 100) == 0);
    CHECK(g_plan.nb == 0 && g_plan.n_off == 0 && g_plan.max_slots == 0 && !oslam_vote_plan_is_one_batch(&g_plan));
    for (limit = 0; limit <= 3; limit++) {
        keep[0] = 0;
        CHECK(check_vector(keep, 1, limit) == 0);
        keep[0] = 7;
        CHECK(check_vector(keep, 1, limit) == 0);
        CHECK(g_plan.nb == 1 && g_plan.b[0].slots == 8);
    }
    memset(keep, 0, sizeof keep);
    CHECK(check_vector(keep, 4096, 0) == 0);
    CHECK(g_plan.nb == 1 && g_plan.max_slots == 0);           /* lists without places never break a batch */
    /* odd and even demands */
    for (n = 0; n < 64; n++) keep[n] = (uint32_t)n;
    for (limit = 0; limit < 200; limit++) CHECK(check_vector(keep, 64, limit) == 0);
    /* a demand of exactly the limit, and of the limit - 1 and + 1 after rounding, alone and behind a neighbour */
    {
        static const uint32_t edge[] = {100, 99, 98, 97, 101, 102, 103};
        size_t e, f;
        for (e = 0; e < sizeof edge / sizeof *edge; e++)
            for (f = 0; f < sizeof edge / sizeof *edge; f++) {
                keep[0] = edge[e]; keep[1] = 0; keep[2] = edge[f]; keep[3] = 2; keep[4] = edge[e]; keep[5] = 1;
                CHECK(check_vector(keep, 6, 100) == 0);
                keep[0] = 50; keep[1] = edge[e] - 50; keep[2] = 2;        /* a running total that lands on the limit's edge */
                CHECK(check_vector(keep, 3, 100) == 0);
            }
        keep[0] = 50; keep[1] = 50; keep[2] = 2;
        CHECK(check_vector(keep, 3, 100) == 0);
        CHECK(g_plan.nb == 2 && g_plan.b[0].n == 2 && g_plan.b[0].slots == 100);
        keep[1] = 51;                                                     /* rounds to 52: one place too many */
        CHECK(check_vector(keep, 3, 100) == 0);
        CHECK(g_plan.nb == 2 && g_plan.b[0].n == 1 && g_plan.b[1].slots == 54);
    }
    /* one reference point larger than the limit gets a batch of its own */
    keep[0] = 10; keep[1] = 5000; keep[2] = 10; keep[3] = 10;
    CHECK(check_vector(keep, 4, 100) == 0);
    CHECK(g_plan.nb == 3 && g_plan.b[1].first == 1 && g_plan.b[1].n == 1 && g_plan.b[1].slots == 5000 && g_plan.max_slots == 5000);
    /* a running total that reaches 0xfffffff0 before the limit */
    keep[0] = 0x7ffffff0u; keep[1] = 0x7ffffff0u; keep[2] = 0x10u; keep[3] = 2; keep[4] = 0xffffffffu; keep[5] = 4;
    CHECK(check_vector(keep, 6, (size_t)1 << 40) == 0);
    CHECK(g_plan.nb == 4 && g_plan.b[0].n == 3 && g_plan.b[0].slots == 0xfffffff0u && g_plan.b[2].slots == 0x100000000ull);
    keep[2] = 0x12u;
    CHECK(check_vector(keep, 6, (size_t)1 << 40) == 0);
    CHECK(g_plan.nb == 4 && g_plan.b[0].n == 2 && g_plan.b[1].n == 2);
    /* seeded random demands against small limits: most have several batches */
    for (trial = 0; trial < 10000; trial++) {
        const int n_ref = (int)(rnd() % 200u);
        const uint32_t top = 1u + rnd() % 300u;
        limit = rnd() % 2000u;
        for (n = 0; n < n_ref; n++) keep[n] = rnd() % 8u == 0 ? 0u : rnd() % top;
        CHECK(check_vector(keep, n_ref, limit) == 0);
    }
    free(g_plan.b);
    printf("vote_plan_check ok\n");
    return 0;
}
