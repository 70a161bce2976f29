/*
 * world_check.c -- the voxel store (csrc/oslam_world.c) linked alone and run under the address and undefined-behaviour
 * sanitizers by tests/test_reload_host.py: put, read, take, clear and destroy over a table that grows and shrinks, with
 * negative coordinates and the limits.  Exit status 0 and "world_check ok" when every check holds.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oslam.h"

static char g_err[256];
int oslam_fail(int code, const char *what)          /* the library's is in oslam_host.c, which needs HIP */
{
    snprintf(g_err, sizeof g_err, "%s", what);
    return code;
}

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "world_check: line %d: %s (%s)\n", __LINE__, #c, g_err); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

#define G_MAX ((1 << 20) + 511)

int main(void)
{
    oslam_world_params p;
    oslam_world *w = NULL, *small = NULL;
    oslam_world_stats st, st2;
    enum { N = 48 * 40 * 24 };                      /* 6 x 6 x 4 bricks: the table of 64 slots doubles three times */
    int32_t *g = (int32_t *)malloc(sizeof(int32_t) * 3 * N), lo[3], hi[3];
    uint32_t *words = (uint32_t *)malloc(sizeof(uint32_t) * N), *out = (uint32_t *)malloc(sizeof(uint32_t) * N);
    size_t i, n = 0, seen = 0;
    int x, y, z;
    CHECK(g && words && out);
    memset(&p, 0, sizeof p);
    p.voxel = 0.05f;
    CHECK(oslam_world_create(&p, &w) == OSLAM_OK && w);
    for (z = -13; z < 11; z++)
        for (y = -7; y < 33; y++)
            for (x = -40; x < 8; x++) {
                g[3 * n] = x;
                g[3 * n + 1] = y;
                g[3 * n + 2] = z;
                words[n] = (uint32_t)(n * 2654435761u);
                if (n % 7 == 0) words[n] &= 0xffffu;                /* unseen: skipped */
                seen += (words[n] >> 16) != 0;
                n++;
            }
    CHECK(n == N);
    CHECK(oslam_world_put(w, g, words, n) == OSLAM_OK);
    CHECK(oslam_world_stats_get(w, &st) == OSLAM_OK && st.voxels == seen && st.bricks == 6 * 6 * 4);
    lo[0] = -40; lo[1] = -7; lo[2] = -13;
    hi[0] = 8; hi[1] = 33; hi[2] = 11;
    CHECK(oslam_world_box(w, lo, hi, out, 0) == OSLAM_OK);
    for (i = 0; i < n; i++) CHECK(out[i] == ((words[i] >> 16) ? words[i] : 0u));
    /* the far corners */
    {
        const int32_t far[6] = {G_MAX, -G_MAX, G_MAX, -G_MAX, G_MAX, -G_MAX};
        const uint32_t fw[2] = {0x00010000u, 0xffffffffu};
        const int32_t flo[3] = {G_MAX, -G_MAX, G_MAX}, fhi[3] = {G_MAX + 1, -G_MAX + 1, G_MAX + 1};
        uint32_t one = 7;
        CHECK(oslam_world_put(w, far, fw, 2) == OSLAM_OK);
        CHECK(oslam_world_box(w, flo, fhi, &one, 1) == OSLAM_OK && one == 0x00010000u);
        CHECK(oslam_world_box(w, flo, fhi, &one, 0) == OSLAM_OK && one == 0u);
        CHECK(oslam_world_stats_get(w, &st2) == OSLAM_OK && st2.voxels == seen + 1 && st2.bricks == st.bricks + 1);
    }
    /* take a box that cuts bricks on every axis, then everything */
    lo[0] = -35; lo[1] = 1; lo[2] = -9;
    hi[0] = 3; hi[1] = 18; hi[2] = 2;
    CHECK(oslam_world_box(w, lo, hi, out, 1) == OSLAM_OK);
    CHECK(oslam_world_box(w, lo, hi, out, 0) == OSLAM_OK);
    for (i = 0; i < (size_t)(38 * 17 * 11); i++) CHECK(out[i] == 0u);
    lo[0] = -(1 << 21); lo[1] = -64; lo[2] = -64;
    hi[0] = 1 << 21; hi[1] = 64; hi[2] = 64;
    CHECK(oslam_world_box(w, lo, hi, NULL, 1) == OSLAM_E_LIMIT);
    lo[0] = -64; hi[0] = 64;
    {
        uint32_t *big = (uint32_t *)malloc(sizeof(uint32_t) * 128 * 128 * 128);
        CHECK(big && oslam_world_box(w, lo, hi, big, 1) == OSLAM_OK);
        free(big);
    }
    CHECK(oslam_world_stats_get(w, &st) == OSLAM_OK && st.voxels == 1 && st.bricks == 1);
    CHECK(oslam_world_put(w, g, words, n) == OSLAM_OK && oslam_world_clear(w) == OSLAM_OK);
    CHECK(oslam_world_stats_get(w, &st) == OSLAM_OK && st.voxels == 0 && st.bricks == 0 && st.lo[0] == 0 && st.hi[2] == 0);
    /* a store too small for the put: nothing changes */
    p.max_bytes = 8192;
    CHECK(oslam_world_create(&p, &small) == OSLAM_OK);
    CHECK(oslam_world_put(small, g, words, 8) == OSLAM_OK && oslam_world_stats_get(small, &st) == OSLAM_OK);
    CHECK(oslam_world_put(small, g, words, n) == OSLAM_E_LIMIT);
    CHECK(oslam_world_stats_get(small, &st2) == OSLAM_OK && memcmp(&st, &st2, sizeof st) == 0);
    CHECK(oslam_world_destroy(small) == OSLAM_OK);
    CHECK(oslam_world_put(w, g, words, n) == OSLAM_OK);                      /* destroyed with bricks in it */
    CHECK(oslam_world_destroy(w) == OSLAM_OK);
    CHECK(oslam_world_destroy(NULL) == OSLAM_E_INVALID && oslam_world_create(NULL, &w) == OSLAM_E_INVALID);
    free(g);
    free(words);
    free(out);
    printf("world_check ok\n");
    return 0;
}
