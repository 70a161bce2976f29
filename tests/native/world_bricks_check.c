/*
 * world_bricks_check.c -- the brick enumeration of the voxel store (oslam_world_bricks, csrc/oslam_world.c) linked alone
 * and run under the address and undefined-behaviour sanitizers by tests/test_world_surface_host.py: the keys of a table
 * that grows and shrinks, with negative coordinates and the limits, are complete, distinct and ascending by
 * (bz, by, bx), and the output conventions hold.  Exit status 0 and "world_bricks_check ok" when every check holds.
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

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            fprintf(stderr, "world_bricks_check: line %d: %s (%s)\n", __LINE__, #c, g_err); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

#define G_MAX ((1 << 20) + 511)

/* the keys of w: as many as the store counts, ascending and distinct, and every brick holds something */
static int enumerate(oslam_world *w, size_t want)
{
    oslam_world_stats st;
    size_t n = 0, m = 0, i;
    int32_t *keys;
    CHECK(oslam_world_bricks(w, NULL, 0, &n) == OSLAM_OK && n == want);
    CHECK(oslam_world_stats_get(w, &st) == OSLAM_OK && st.bricks == n);
    keys = (int32_t *)malloc(sizeof(int32_t) * 3 * (n + 1));
    CHECK(keys);
    memset(keys, 0x55, sizeof(int32_t) * 3 * (n + 1));
    if (n > 0) {
        CHECK(oslam_world_bricks(w, keys, n - 1, &m) == OSLAM_E_LIMIT && m == n && keys[0] == 0x55555555);
    }
    CHECK(oslam_world_bricks(w, keys, n, &m) == OSLAM_OK && m == n && keys[3 * n] == 0x55555555);
    for (i = 0; i < n; i++) {
        const int32_t *k = keys + 3 * i;
        const int32_t lo[3] = {k[0] * 8, k[1] * 8, k[2] * 8}, hi[3] = {lo[0] + 8, lo[1] + 8, lo[2] + 8};
        uint32_t words[512];
        size_t v, seen = 0;
        if (i > 0) {
            const int32_t *p = k - 3;
            CHECK(p[2] < k[2] || (p[2] == k[2] && (p[1] < k[1] || (p[1] == k[1] && p[0] < k[0]))));
        }
        CHECK(oslam_world_box(w, lo, hi, words, 0) == OSLAM_OK);
        for (v = 0; v < 512; v++) seen += words[v] != 0u;
        CHECK(seen > 0);
    }
    free(keys);
    return 0;
}

int main(void)
{
    oslam_world_params p;
    oslam_world *w = NULL;
    size_t n = 9, total = 0;
    int32_t g[3], lo[3], hi[3];
    uint32_t word = 0x00030007u;
    int x, y, z, round;
    memset(&p, 0, sizeof p);
    p.voxel = 0.05f;
    CHECK(oslam_world_create(&p, &w) == OSLAM_OK && w);
    CHECK(oslam_world_bricks(NULL, NULL, 0, &n) == OSLAM_E_INVALID && oslam_world_bricks(w, NULL, 0, NULL) == OSLAM_E_INVALID);
    CHECK(oslam_world_bricks(w, NULL, 4, &n) == OSLAM_E_INVALID);
    CHECK(enumerate(w, 0) == 0);
    /* one voxel per brick over a growing table: 64 slots double at 33, 65, 129 and 257 bricks */
    for (z = -5; z < 3; z++)
        for (y = -2; y < 6; y++)
            for (x = -7; x < 1; x++) {
                g[0] = 8 * x + ((x + y) & 7);
                g[1] = 8 * y + ((y + z) & 7);
                g[2] = 8 * z + ((z + x) & 7);
                CHECK(oslam_world_put(w, g, &word, 1) == OSLAM_OK);
                total++;
                if (total == 1 || total == 32 || total == 33 || total == 65 || total == 130 || total == 512) CHECK(enumerate(w, total) == 0);
            }
    /* the limits of g, each in a brick of its own */
    for (round = 0; round < 2; round++) {
        g[0] = round ? -G_MAX : G_MAX;
        g[1] = round ? G_MAX : -G_MAX;
        g[2] = round ? -G_MAX : G_MAX;
        CHECK(oslam_world_put(w, g, &word, 1) == OSLAM_OK);
    }
    CHECK(enumerate(w, 514) == 0);
    /* shrink: slabs of bricks are taken until nothing is left */
    for (z = -5; z < 3; z++) {
        lo[0] = -64; lo[1] = -64; lo[2] = 8 * z;
        hi[0] = 64; hi[1] = 64; hi[2] = 8 * z + 8;
        CHECK(oslam_world_box(w, lo, hi, NULL, 1) == OSLAM_E_INVALID);      /* a box that holds voxels needs its output */
        {
            uint32_t *out = (uint32_t *)malloc(sizeof(uint32_t) * 128 * 128 * 8);
            CHECK(out && oslam_world_box(w, lo, hi, out, 1) == OSLAM_OK);
            free(out);
        }
        CHECK(enumerate(w, 2 + 64 * (size_t)(2 - z)) == 0);
    }
    CHECK(oslam_world_clear(w) == OSLAM_OK && enumerate(w, 0) == 0);
    CHECK(oslam_world_destroy(w) == OSLAM_OK);
    printf("world_bricks_check ok\n");
    return 0;
}
