/*
 * window_check.c -- csrc/oslam_window.h included alone: the shifting window's arithmetic against brute force and against
 * the expressions it replaced.  Built and run by tests/test_window_host.py, once with the library's flags and once under
 * the address and undefined-behaviour sanitizers.  The functions named old_* are literal copies of the host code before
 * the header existed (oslam_volume.c and oslam_world_surface.c, over a stand-in for the volume's handle); they are the
 * statement of the contract (the GPU tests compare windows, stores and origins made with them word for word), so they
 * stay as they are when the header changes.  Exit status 0 and "window_check ok" when every comparison holds.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "oslam_window.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "window_check: line %d: %s\n", __LINE__, #c);     \
            return 1;                                                         \
        }                                                                     \
    } while (0)

/* ---- the expressions as they stood ---- */
typedef struct old_volume {                      /* what they read of struct oslam_volume */
    struct {
        unsigned nx, ny, nz;
        float voxel, origin[3];
    } p;
    int off[3];
} old_volume;

/* oslam_volume.c window_origin; the loop of oslam_world_map_open was the same text over (origin0, voxel, anchor) */
static void old_window_origin(const old_volume *vol, const int off[3], float origin[3])
{
    int a;
    for (a = 0; a < 3; a++) {
        origin[a] = vol->p.origin[a];
        if (off[a] != 0) {
            const float step = (float)off[a] * vol->p.voxel;
            origin[a] = vol->p.origin[a] + step;
        }
    }
}

/* oslam_volume.c global_of */
static void old_global_of(const old_volume *vol, uint32_t lin, int32_t g[3])
{
    const uint32_t row = lin / vol->p.nx;
    g[0] = (int32_t)(lin - row * vol->p.nx) + vol->off[0];
    g[1] = (int32_t)(row % vol->p.ny) + vol->off[1];
    g[2] = (int32_t)(row / vol->p.ny) + vol->off[2];
}

/* oslam_volume.c enter_record, the index it wrote */
typedef struct old_enter_ctx {
    int off[3];
    size_t nx, ny;
} old_enter_ctx;

static uint32_t old_enter_lin(const old_enter_ctx *e, const int32_t g[3])
{
    return (uint32_t)(((size_t)(g[2] - e->off[2]) * e->ny + (size_t)(g[1] - e->off[1])) * e->nx + (size_t)(g[0] - e->off[0]));
}

/* oslam_world_surface.c window_bricks */
static void old_window_bricks(const old_volume *vol, int kb0[3], int nb[3])
{
    const int n[3] = {(int)vol->p.nx, (int)vol->p.ny, (int)vol->p.nz};
    int a;
    for (a = 0; a < 3; a++) {
        kb0[a] = vol->off[a] >> 3;                                  /* arithmetic: floor for a negative offset */
        nb[a] = ((vol->off[a] + n[a] - 1) >> 3) - kb0[a] + 1;
    }
}

/* ---- the entering region ---- */
static int in_box(const int32_t g[3], const int32_t lo[3], const int32_t hi[3])
{
    return g[0] >= lo[0] && g[0] < hi[0] && g[1] >= lo[1] && g[1] < hi[1] && g[2] >= lo[2] && g[2] < hi[2];
}

/* what holds for windows of equal size whatever the check: no box for a zero shift, at most 3 boxes, none empty */
static int boxes_sane(const int off_old[3], const int off_new[3], int nb, int32_t lo[7][3], int32_t hi[7][3])
{
    int a, b;
    CHECK(nb >= 0 && nb <= 3);
    if (off_old[0] == off_new[0] && off_old[1] == off_new[1] && off_old[2] == off_new[2]) CHECK(nb == 0);
    for (b = 0; b < nb; b++)
        for (a = 0; a < 3; a++) CHECK(lo[b][a] < hi[b][a]);
    return 0;
}

/* every voxel of the new window's box plus a margin of 2 lies in exactly one box if it is in the new window and not in
 * the old one, and in none otherwise */
static int entering_by_voxels(const int off_old[3], const int shift[3], const unsigned n[3])
{
    int32_t lo[7][3], hi[7][3], g[3], old_lo[3], old_hi[3], new_lo[3], new_hi[3];
    int off_new[3], a, b, nb;
    for (a = 0; a < 3; a++) {
        off_new[a] = off_old[a] + shift[a];
        old_lo[a] = off_old[a];
        old_hi[a] = off_old[a] + (int)n[a];
        new_lo[a] = off_new[a];
        new_hi[a] = off_new[a] + (int)n[a];
    }
    nb = oslam_window_entering(off_old, off_new, n, lo, hi);
    if (boxes_sane(off_old, off_new, nb, lo, hi)) return 1;
    for (g[2] = new_lo[2] - 2; g[2] < new_hi[2] + 2; g[2]++)
        for (g[1] = new_lo[1] - 2; g[1] < new_hi[1] + 2; g[1]++)
            for (g[0] = new_lo[0] - 2; g[0] < new_hi[0] + 2; g[0]++) {
                int hits = 0;
                for (b = 0; b < nb; b++) hits += in_box(g, lo[b], hi[b]);
                CHECK(hits == (in_box(g, new_lo, new_hi) && !in_box(g, old_lo, old_hi) ? 1 : 0));
            }
    return 0;
}

/* the same by volumes and interval tests, for windows too large to mark: every box lies in the new window and outside the
 * old one, no two boxes meet, and the volumes sum to |new| - |overlap| */
static int entering_by_volumes(const int off_old[3], const int shift[3], const unsigned n[3])
{
    int32_t lo[7][3], hi[7][3];
    int off_new[3], a, b, c, nb;
    uint64_t sum = 0, whole = 1, overlap = 1;
    for (a = 0; a < 3; a++) {
        const int64_t ol = shift[a] > 0 ? shift[a] : -(int64_t)shift[a];
        off_new[a] = off_old[a] + shift[a];
        whole *= n[a];
        overlap *= ol < (int64_t)n[a] ? (uint64_t)((int64_t)n[a] - ol) : 0;
    }
    nb = oslam_window_entering(off_old, off_new, n, lo, hi);
    if (boxes_sane(off_old, off_new, nb, lo, hi)) return 1;
    for (b = 0; b < nb; b++) {
        int apart_old = 0;
        uint64_t v = 1;
        for (a = 0; a < 3; a++) {
            CHECK(lo[b][a] >= off_new[a] && hi[b][a] <= off_new[a] + (int)n[a]);
            if (hi[b][a] <= off_old[a] || lo[b][a] >= off_old[a] + (int)n[a]) apart_old = 1;
            v *= (uint64_t)(hi[b][a] - lo[b][a]);
        }
        CHECK(apart_old);
        sum += v;
        for (c = 0; c < b; c++) {
            int apart = 0;
            for (a = 0; a < 3; a++)
                if (hi[b][a] <= lo[c][a] || lo[b][a] >= hi[c][a]) apart = 1;
            CHECK(apart);
        }
    }
    CHECK(sum == whole - overlap);
    return 0;
}

static int check_entering(void)
{
    static const int olds[3][3] = {{0, 0, 0}, {-7, 2, 1}, {3, -2, -9}};
    static const unsigned ragged[3] = {5, 3, 4}, cube[3] = {256, 256, 256};
    static const int big[][3] = {{0, 0, 0}, {8, 0, 0}, {-8, 16, 0}, {3, -5, 2}, {255, 255, 255}, {256, 0, 0}, {-256, 1, -1},
                                 {257, -255, 8}, {0, 0, -300}, {-1, -1, -1}, {64, 64, -64}};
    enum { LIM = (1 << 20) - 8 };
    static const int far_off[4][3] = {{LIM, -LIM, LIM}, {-LIM, LIM, -LIM}, {LIM - 8, -LIM + 8, 0}, {-LIM + 264, LIM - 256, -LIM}};
    static const int far_shift[4][3] = {{-8, 8, -24}, {264, -256, 8}, {8, -8, 3}, {-264, 256, 0}};     /* from +-(2^20 - 8), and to it */
    int shift[3], cases = 0;
    size_t k, o;
    for (o = 0; o < 3; o++)
        for (shift[2] = -5; shift[2] <= 5; shift[2]++)
            for (shift[1] = -4; shift[1] <= 4; shift[1]++)
                for (shift[0] = -6; shift[0] <= 6; shift[0]++, cases++)
                    if (entering_by_voxels(olds[o], shift, ragged) || entering_by_volumes(olds[o], shift, ragged)) return 1;
    CHECK(cases == 3861);
    for (o = 0; o < 3; o++)
        for (k = 0; k < sizeof big / sizeof big[0]; k++)
            if (entering_by_volumes(olds[o], big[k], cube)) return 1;
    for (k = 0; k < 4; k++)
        if (entering_by_volumes(far_off[k], far_shift[k], cube)) return 1;
    return 0;
}

/* ---- the origin ---- */
static int check_origin(void)
{
    static const int offs[] = {0, 1, -1, 8, -8, 1 << 20, -(1 << 20)};
    static const float origins[] = {-0.0f, 0.0f, 1e-42f, -1.25f, 2.0f, 0.1f, -2.56f};
    static const float voxels[] = {0.0625f, 0.02f};
    const size_t n_off = sizeof offs / sizeof offs[0], n_org = sizeof origins / sizeof origins[0];
    size_t i, j, k, v;
    for (v = 0; v < 2; v++)
        for (i = 0; i < n_off; i++)
            for (j = 0; j < n_off; j++)
                for (k = 0; k < n_org; k++) {
                    old_volume vol;
                    const int off[3] = {offs[i], offs[j], offs[(i + j + k) % n_off]};
                    float want[3], got[3];
                    vol.p.voxel = voxels[v];
                    vol.p.origin[0] = origins[k];
                    vol.p.origin[1] = origins[(k + i) % n_org];
                    vol.p.origin[2] = origins[(k + j) % n_org];
                    old_window_origin(&vol, off, want);
                    oslam_window_origin(vol.p.origin, vol.p.voxel, off, got);
                    CHECK(memcmp(want, got, sizeof want) == 0);
                }
    {                                               /* an offset of 0 keeps -0.0f: an addition of +0.0f would not */
        const float origin0[3] = {-0.0f, -0.0f, -0.0f}, minus_zero = -0.0f;
        const int off[3] = {0, 8, 0};
        float got[3];
        oslam_window_origin(origin0, 0.02f, off, got);
        CHECK(memcmp(&got[0], &minus_zero, sizeof minus_zero) == 0 && memcmp(&got[2], &minus_zero, sizeof minus_zero) == 0);
        CHECK(got[1] == 8.0f * 0.02f);
    }
    return 0;
}

/* ---- global coordinate and linear index ---- */
static int check_index(void)
{
    static const int offs[2][3] = {{-1048568, -24, -3}, {1048568, 7, 40}};
    const unsigned n[3] = {16, 24, 8};
    size_t o;
    for (o = 0; o < 2; o++) {
        old_volume vol;
        old_enter_ctx e;
        uint32_t lin;
        vol.p.nx = n[0];
        vol.p.ny = n[1];
        vol.p.nz = n[2];
        memcpy(vol.off, offs[o], sizeof vol.off);
        memcpy(e.off, offs[o], sizeof e.off);
        e.nx = n[0];
        e.ny = n[1];
        for (lin = 0; lin < n[0] * n[1] * n[2]; lin++) {
            int32_t want[3], g[3];
            old_global_of(&vol, lin, want);
            oslam_window_global(n, offs[o], lin, g);
            CHECK(memcmp(want, g, sizeof g) == 0);
            CHECK(g[0] - offs[o][0] == (int32_t)(lin % 16) && g[1] - offs[o][1] == (int32_t)(lin / 16 % 24) &&
                  g[2] - offs[o][2] == (int32_t)(lin / (16 * 24)));
            CHECK(oslam_window_lin(n, offs[o], g) == lin && old_enter_lin(&e, g) == lin);
        }
    }
    return 0;
}

/* ---- the bricks a window overlaps ---- */
static int floor_div8(int x) { return x >= 0 ? x / 8 : -((-x + 7) / 8); }

static int check_bricks(void)
{
    static const unsigned sides[2] = {16, 24};
    int off, a;
    size_t s;
    for (s = 0; s < 2; s++)
        for (off = -17; off <= 17; off++) {
            old_volume vol;
            const unsigned n[3] = {sides[s], sides[1 - s], sides[s]};
            const int offs[3] = {off, -off, off + 3};
            int kb0[3], nb[3], kb0_old[3], nb_old[3];
            vol.p.nx = n[0];
            vol.p.ny = n[1];
            vol.p.nz = n[2];
            memcpy(vol.off, offs, sizeof vol.off);
            old_window_bricks(&vol, kb0_old, nb_old);
            oslam_window_bricks(n, offs, kb0, nb);
            CHECK(memcmp(kb0, kb0_old, sizeof kb0) == 0 && memcmp(nb, nb_old, sizeof nb) == 0);
            for (a = 0; a < 3; a++) {
                CHECK(kb0[a] == floor_div8(offs[a]));
                CHECK(kb0[a] + nb[a] - 1 == floor_div8(offs[a] + (int)n[a] - 1));
            }
        }
    return 0;
}

/* ---- the layout of a batch of records ---- */
static int check_records(void)
{
    static const size_t counts[3] = {0, 1, 2147483647u};
    size_t k;
    CHECK(sizeof(size_t) >= 8);                    /* the largest batch has 12 * (2^31 - 1) bytes */
    for (k = 0; k < 3; k++) {
        CHECK(oslam_records_bytes(counts[k], 0) == (size_t)8 * counts[k]);
        CHECK(oslam_records_bytes(counts[k], 1) == (size_t)12 * counts[k]);
        CHECK(oslam_records_colours(counts[k]) == (size_t)2 * counts[k]);
        /* the colours follow the pairs and end with the batch */
        CHECK(sizeof(uint32_t) * (oslam_records_colours(counts[k]) + counts[k]) == oslam_records_bytes(counts[k], 1));
        CHECK(sizeof(uint32_t) * oslam_records_colours(counts[k]) == oslam_records_bytes(counts[k], 0));
    }
    return 0;
}

int main(void)
{
    if (check_entering() || check_origin() || check_index() || check_bricks() || check_records()) return 1;
    printf("window_check ok\n");
    return 0;
}
