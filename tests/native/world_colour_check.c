/*
 * world_colour_check.c -- the colour store (csrc/oslam_world.c with oslam_world_params.colour = 1) linked alone and run
 * under the address and undefined-behaviour sanitizers by tests/test_world_colour_host.py: put with colours, read, take,
 * a plain put over coloured records, clear and destroy over a table that grows and shrinks, and the refusals of a plain
 * store.  Exit status 0 and "world_colour_check ok" when every check holds.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oslam.h"
#include "oslam_world.h"

static char g_err[256];
int oslam_fail(int code, const char *what)          /* the library's is in oslam_host.c, which needs HIP */
{
    snprintf(g_err, sizeof g_err, "%s", what);
    return code;
}

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            fprintf(stderr, "world_colour_check: line %d: %s (%s)\n", __LINE__, #c, g_err); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

#define G_MAX ((1 << 20) + 511)
#define BRICK_BYTES 2064u
#define COLOUR_BRICK_BYTES 4112u

int main(void)
{
    oslam_world_params p;
    oslam_world *w = NULL, *plain = NULL, *small = NULL;
    oslam_world_stats st, st2;
    enum { N = 48 * 40 * 24 };                      /* 6 x 6 x 4 bricks: the table of 64 slots doubles three times */
    int32_t *g = (int32_t *)malloc(sizeof(int32_t) * 3 * N), lo[3], hi[3];
    uint32_t *words = (uint32_t *)malloc(sizeof(uint32_t) * N), *cols = (uint32_t *)malloc(sizeof(uint32_t) * N);
    uint32_t *out = (uint32_t *)malloc(sizeof(uint32_t) * N), *cout = (uint32_t *)malloc(sizeof(uint32_t) * N);
    size_t i, n = 0, seen = 0;
    int x, y, z;
    CHECK(g && words && cols && out && cout);
    memset(&p, 0, sizeof p);
    p.voxel = 0.05f;
    p.colour = 2;
    CHECK(oslam_world_create(&p, &w) == OSLAM_E_INVALID && !w);
    p.colour = 0;
    CHECK(oslam_world_create(&p, &plain) == OSLAM_OK && !oslam_world_has_colour(plain) && !oslam_world_has_colour(NULL));
    p.colour = 1;
    CHECK(oslam_world_create(&p, &w) == OSLAM_OK && w && oslam_world_has_colour(w));
    for (z = -13; z < 11; z++)
        for (y = -7; y < 33; y++)
            for (x = -40; x < 8; x++) {
                g[3 * n] = x;
                g[3 * n + 1] = y;
                g[3 * n + 2] = z;
                words[n] = (uint32_t)(n * 2654435761u);
                cols[n] = (uint32_t)(n * 40503u + 17u);
                if (n % 7 == 0) words[n] &= 0xffffu;                /* unseen: skipped, colour and all */
                if (n % 5 == 0) cols[n] &= 0xffffffu;               /* wc == 0: stored as it is */
                seen += (words[n] >> 16) != 0;
                n++;
            }
    CHECK(n == N);
    CHECK(oslam_world_put_colour(w, g, words, cols, n) == OSLAM_OK);
    CHECK(oslam_world_stats_get(w, &st) == OSLAM_OK && st.voxels == seen && st.bricks == 6 * 6 * 4);
    CHECK(st.bytes == st.bricks * COLOUR_BRICK_BYTES + 512u * sizeof(void *));
    CHECK(oslam_world_put(plain, g, words, n) == OSLAM_OK && oslam_world_stats_get(plain, &st2) == OSLAM_OK);
    CHECK(st2.voxels == seen && st2.bytes == st2.bricks * BRICK_BYTES + 512u * sizeof(void *));
    lo[0] = -40; lo[1] = -7; lo[2] = -13;
    hi[0] = 8; hi[1] = 33; hi[2] = 11;
    CHECK(oslam_world_box_colour(w, lo, hi, out, cout, 0) == OSLAM_OK);
    for (i = 0; i < n; i++) CHECK(out[i] == ((words[i] >> 16) ? words[i] : 0u) && cout[i] == ((words[i] >> 16) ? cols[i] : 0u));
    /* the internal accessors: a brick's colours lie next to its words */
    {
        const int32_t key[3] = {-5, -1, -2}, none[3] = {100, 100, 100};
        const uint32_t *bw = oslam_world_brick_words(w, key), *bc = oslam_world_brick_colours(w, key);
        CHECK(bw && bc && !oslam_world_brick_colours(w, none) && !oslam_world_brick_colours(plain, key));
        memset(out, 0, sizeof(uint32_t) * 512);
        lo[0] = -40; lo[1] = -8; lo[2] = -16;
        hi[0] = -32; hi[1] = 0; hi[2] = -8;
        CHECK(oslam_world_box_colour(w, lo, hi, out, cout, 0) == OSLAM_OK);
        CHECK(memcmp(out, bw, sizeof(uint32_t) * 512) == 0 && memcmp(cout, bc, sizeof(uint32_t) * 512) == 0);
    }
    /* a plain store refuses the colour calls; a plain put on a colour store stores colour 0; the plain box still reads */
    CHECK(oslam_world_put_colour(plain, g, words, cols, 1) == OSLAM_E_INVALID);
    CHECK(oslam_world_box_colour(plain, lo, hi, out, cout, 0) == OSLAM_E_INVALID);
    CHECK(oslam_world_put_colour(w, g, words, NULL, 1) == OSLAM_E_INVALID && oslam_world_put_colour(NULL, g, words, cols, 1) == OSLAM_E_INVALID);
    CHECK(oslam_world_box_colour(w, lo, hi, out, NULL, 0) == OSLAM_E_INVALID && oslam_world_box_colour(NULL, lo, hi, out, cout, 0) == OSLAM_E_INVALID);
    {
        const int32_t one_g[3] = {1, 1, 1}, olo[3] = {1, 1, 1}, ohi[3] = {2, 2, 2};
        const uint32_t w1 = 0x00050001u, c1 = 0x03112233u, w2 = 0x00060002u;
        uint32_t a = 9, b = 9;
        CHECK(oslam_world_put_colour(w, one_g, &w1, &c1, 1) == OSLAM_OK);
        CHECK(oslam_world_box_colour(w, olo, ohi, &a, &b, 0) == OSLAM_OK && a == w1 && b == c1);
        CHECK(oslam_world_put(w, one_g, &w2, 1) == OSLAM_OK);
        CHECK(oslam_world_box_colour(w, olo, ohi, &a, &b, 0) == OSLAM_OK && a == w2 && b == 0u);
        CHECK(oslam_world_box(w, olo, ohi, &a, 0) == OSLAM_OK && a == w2);
        CHECK(oslam_world_put_colour(w, one_g, &w1, &c1, 1) == OSLAM_OK);
        CHECK(oslam_world_box_colour(w, olo, ohi, &a, &b, 1) == OSLAM_OK && a == w1 && b == c1);      /* take */
        CHECK(oslam_world_box_colour(w, olo, ohi, &a, &b, 0) == OSLAM_OK && a == 0u && b == 0u);
        CHECK(oslam_world_put(w, one_g, &w2, 1) == OSLAM_OK);                                          /* no stale colour under a taken word */
        CHECK(oslam_world_box_colour(w, olo, ohi, &a, &b, 0) == OSLAM_OK && a == w2 && b == 0u);
    }
    /* the far corners */
    {
        const int32_t far[6] = {G_MAX, -G_MAX, G_MAX, -G_MAX, G_MAX, -G_MAX};
        const uint32_t fw[2] = {0x00010000u, 0xffffffffu}, fc[2] = {0xffffffffu, 0x01000000u};
        const int32_t flo[3] = {G_MAX, -G_MAX, G_MAX}, fhi[3] = {G_MAX + 1, -G_MAX + 1, G_MAX + 1};
        uint32_t one = 7, col = 7;
        CHECK(oslam_world_put_colour(w, far, fw, fc, 2) == OSLAM_OK);
        CHECK(oslam_world_box_colour(w, flo, fhi, &one, &col, 1) == OSLAM_OK && one == 0x00010000u && col == 0xffffffffu);
        CHECK(oslam_world_box_colour(w, flo, fhi, &one, &col, 0) == OSLAM_OK && one == 0u && col == 0u);
    }
    /* take a box that cuts bricks on every axis, then everything: the table shrinks */
    lo[0] = -35; lo[1] = 1; lo[2] = -9;
    hi[0] = 3; hi[1] = 18; hi[2] = 2;
    CHECK(oslam_world_box_colour(w, lo, hi, out, cout, 1) == OSLAM_OK);
    CHECK(oslam_world_box_colour(w, lo, hi, out, cout, 0) == OSLAM_OK);
    for (i = 0; i < (size_t)(38 * 17 * 11); i++) CHECK(out[i] == 0u && cout[i] == 0u);
    lo[0] = -64; lo[1] = -64; lo[2] = -64;
    hi[0] = 64; hi[1] = 64; hi[2] = 64;
    {
        uint32_t *big = (uint32_t *)malloc(sizeof(uint32_t) * 128 * 128 * 128), *bigc = (uint32_t *)malloc(sizeof(uint32_t) * 128 * 128 * 128);
        CHECK(big && bigc && oslam_world_box_colour(w, lo, hi, big, bigc, 1) == OSLAM_OK);
        free(big);
        free(bigc);
    }
    CHECK(oslam_world_stats_get(w, &st) == OSLAM_OK && st.voxels == 1 && st.bricks == 1);
    CHECK(oslam_world_put_colour(w, g, words, cols, n) == OSLAM_OK && oslam_world_clear(w) == OSLAM_OK);
    CHECK(oslam_world_stats_get(w, &st) == OSLAM_OK && st.voxels == 0 && st.bricks == 0 && st.bytes == 64u * sizeof(void *));
    /* max_bytes counts the larger brick: room for one colour brick and the empty table, where two plain bricks would fit */
    p.max_bytes = 2 * BRICK_BYTES + 64u * sizeof(void *);
    CHECK(oslam_world_create(&p, &small) == OSLAM_OK);
    CHECK(oslam_world_put_colour(small, g, words, cols, 8) == OSLAM_OK && oslam_world_stats_get(small, &st) == OSLAM_OK && st.bricks == 1);
    CHECK(oslam_world_put_colour(small, g, words, cols, n) == OSLAM_E_LIMIT);
    CHECK(oslam_world_stats_get(small, &st2) == OSLAM_OK && memcmp(&st, &st2, sizeof st) == 0);
    CHECK(oslam_world_destroy(small) == OSLAM_OK);
    CHECK(oslam_world_put_colour(w, g, words, cols, n) == OSLAM_OK);          /* destroyed with bricks in it */
    CHECK(oslam_world_destroy(w) == OSLAM_OK && oslam_world_destroy(plain) == OSLAM_OK);
    free(g);
    free(words);
    free(cols);
    free(out);
    free(cout);
    printf("world_colour_check ok\n");
    return 0;
}
