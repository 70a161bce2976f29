/*
 * seg_union_check.c -- csrc/oslam_seg_union.h with host atomics, as a program of its own (tests/test_segments_host.py
 * builds and runs it, plain and under the address and undefined-behaviour sanitizers).
 *
 * Input file (text): the number of cases, then per case "n m", m lines "a b" (the joined pixel pairs) and n roots as the
 * restatement gives them (-1 = the pixel is not in).  Every case is run under SHUFFLES seeded orders of its edges, the
 * unions applied from OpenMP threads; L[i] <= i is checked at the entries a thread has just touched and at a moving
 * sample while the unions are in flight, over the whole array at the end, and every pixel's find must be the
 * restatement's root.
 */
#include <omp.h>
#include <stdio.h>
#include <stdlib.h>

#include "oslam_seg_union.h"

#define SHUFFLES 5

static uint64_t rng_state;
static uint32_t rng_next(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static int holds(const uint32_t *L, uint32_t i)
{
    const uint32_t p = OSLAM_SEG_LOAD(&L[i]);
    return p == OSLAM_SEG_NONE || p <= i;
}

int main(int argc, char **argv)
{
    FILE *f;
    int n_cases, c, checked = 0;
    if (argc != 2 || !(f = fopen(argv[1], "r"))) {
        fprintf(stderr, "usage: seg_union_check FILE\n");
        return 2;
    }
    if (fscanf(f, "%d", &n_cases) != 1) return 2;
    for (c = 0; c < n_cases; c++) {
        long n, m, e, i;
        int s, bad = 0;
        uint32_t *a, *b, *perm, *L;
        int32_t *want;
        if (fscanf(f, "%ld %ld", &n, &m) != 2 || n < 1 || m < 0) return 2;
        a = malloc(sizeof *a * (size_t)(m + 1));
        b = malloc(sizeof *b * (size_t)(m + 1));
        perm = malloc(sizeof *perm * (size_t)(m + 1));
        L = malloc(sizeof *L * (size_t)n);
        want = malloc(sizeof *want * (size_t)n);
        if (!a || !b || !perm || !L || !want) return 2;
        for (e = 0; e < m; e++)
            if (fscanf(f, "%u %u", &a[e], &b[e]) != 2) return 2;
        for (i = 0; i < n; i++)
            if (fscanf(f, "%d", &want[i]) != 1) return 2;
        for (s = 0; s < SHUFFLES; s++) {
            rng_state = 0x9e3779b97f4a7c15ull * (uint64_t)(s + 1) + (uint64_t)c;
            for (e = 0; e < m; e++) perm[e] = (uint32_t)e;
            if (s > 0)                               /* the first order is the list's own */
                for (e = m - 1; e > 0; e--) {
                    const long j = (long)(rng_next() % (uint32_t)(e + 1));
                    const uint32_t t = perm[e];
                    perm[e] = perm[j];
                    perm[j] = t;
                }
            for (i = 0; i < n; i++) L[i] = want[i] < 0 ? OSLAM_SEG_NONE : (uint32_t)i;
#pragma omp parallel for schedule(dynamic, 8) num_threads(8) reduction(+ : bad)
            for (e = 0; e < m; e++) {
                const uint32_t x = a[perm[e]], y = b[perm[e]];
                /* swapped in every other shuffle: the order of the arguments must not matter */
                if (s & 1) oslam_seg_union(L, y, x, (uint32_t)n);
                else oslam_seg_union(L, x, y, (uint32_t)n);
                bad += !holds(L, x) + !holds(L, y) + !holds(L, (uint32_t)((uint64_t)e * 7919u % (uint64_t)n));
            }
            for (i = 0; i < n; i++) {
                bad += !holds(L, (uint32_t)i);
                if (want[i] >= 0 && oslam_seg_find(L, (uint32_t)i, (uint32_t)n) != (uint32_t)want[i]) bad++;
                if (want[i] < 0 && L[i] != OSLAM_SEG_NONE) bad++;
            }
            if (bad) {
                fprintf(stderr, "case %d, shuffle %d: %d violations\n", c, s, bad);
                return 1;
            }
            checked++;
        }
        /* indices outside the array end the calls without a load or a store */
        oslam_seg_union(L, (uint32_t)n, 0, (uint32_t)n);
        oslam_seg_union(L, 0, (uint32_t)n + 5u, (uint32_t)n);
        if (oslam_seg_find(L, (uint32_t)n + 1u, (uint32_t)n) != (uint32_t)n + 1u) return 1;
        free(a);
        free(b);
        free(perm);
        free(L);
        free(want);
    }
    fclose(f);
    printf("seg_union_check ok: %d cases, %d runs\n", n_cases, checked);
    return 0;
}
