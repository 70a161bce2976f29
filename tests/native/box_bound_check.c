/*
 * box_bound_check.c -- pc_box_bin_range (csrc/ppf_core.h), the bound that lets phase 1 of the scene-key kernels drop a
 * (reference point, group of 64 scene points) with one test: for random boxes and points -- degenerate boxes (a plane,
 * a line, one point), points inside the box, on its faces and far away, several bin widths -- the range it gives holds
 * pc_pair_dist_bin of the pair (point, q) for every q of the box that is tried: the corners, the point of the box
 * nearest to the point, and random points of the box.  It gives no range for coordinates that are not finite and for
 * a box that is the point itself, and where it gives one the range is no wider than the box's diagonal plus two bins and the slack.
 * Built and run by tests/test_box_bound_host.py, with the library's flags and under the address and
 * undefined-behaviour sanitizers.  Exit status 0 and "box_bound_check ok" when every comparison holds.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "ppf_core.h"

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "box_bound_check: line %d: %s\n", __LINE__, #c);      \
            return 1;                                                             \
        }                                                                         \
    } while (0)

static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void)
{
    g_s ^= g_s << 13;
    g_s ^= g_s >> 7;
    g_s ^= g_s << 17;
    return (uint32_t)(g_s >> 32);
}
static float unit(void) { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }           /* [0, 1) */

/* the bin of the pair (p, q) as the kernels take it, inside the range? */
static int holds(const float *p, const float *q, float d, int kmin, int kmax)
{
    const int k = pc_pair_dist_bin(q[0] - p[0], q[1] - p[1], q[2] - p[2], d, 1.0f / d);
    return k >= kmin && k <= kmax;
}

static int one_case(const float *box, const float *p, float d, int *given)
{
    int kmin = 0, kmax = 0, c, a, t;
    float q[3], diag = 0.0f;
    *given = pc_box_bin_range(box, p[0], p[1], p[2], 1.0f / d, &kmin, &kmax);
    if (!*given) return 0;
    CHECK(kmin >= 0 && kmin <= kmax);
    for (a = 0; a < 3; a++) diag += (box[3 + a] - box[a]) * (box[3 + a] - box[a]);
    /* farthest - nearest <= the diagonal; the slack widens either end by its share of the bin number */
    CHECK((double)(kmax - kmin) <= sqrt((double)diag) / (double)d + 2.0 + 2.0 * (double)PC_BOX_SLACK * (double)kmax);
    for (c = 0; c < 8; c++) {
        for (a = 0; a < 3; a++) q[a] = box[((c >> a) & 1) * 3 + a];
        CHECK(holds(p, q, d, kmin, kmax));
    }
    for (a = 0; a < 3; a++) q[a] = p[a] < box[a] ? box[a] : p[a] > box[3 + a] ? box[3 + a] : p[a];
    CHECK(holds(p, q, d, kmin, kmax));
    for (t = 0; t < 24; t++) {
        for (a = 0; a < 3; a++) {
            const uint32_t m = rnd() & 7u;                 /* a face now and then */
            q[a] = m == 0 ? box[a] : m == 1 ? box[3 + a] : box[a] + (box[3 + a] - box[a]) * unit();
            if (q[a] > box[3 + a]) q[a] = box[3 + a];
        }
        CHECK(holds(p, q, d, kmin, kmax));
    }
    return 0;
}

int main(void)
{
    static const float widths[] = {0.0993f, 0.01f, 1.0f, 3.7e-4f, 25.0f};
    long n_given = 0, n = 0;
    int i, a, given;
    for (i = 0; i < 200000; i++) {
        float box[6], p[3];
        const float d = widths[rnd() % 5u];
        const float size = (rnd() & 3u) == 0 ? 8.0f : 0.7f;
        const uint32_t flat = rnd() & 7u;                  /* bit a: the box has no extent on axis a (half of the cases) */
        const uint32_t where = rnd() & 3u;
        for (a = 0; a < 3; a++) {
            const float c = (unit() - 0.5f) * 20.0f, half = ((rnd() & 1u) && ((flat >> a) & 1u)) ? 0.0f : unit() * size;
            box[a] = c - half;
            box[3 + a] = c + half;
            /* the point: inside the box, near it, or anywhere */
            p[a] = where == 0 ? box[a] + (box[3 + a] - box[a]) * unit()
                 : where == 1 ? c + (unit() - 0.5f) * 4.0f * (half + d)
                              : (unit() - 0.5f) * 60.0f;
        }
        if (one_case(box, p, d, &given)) return 1;
        /* a box that is more than the point alone always gets a range */
        if (box[0] < box[3] || box[1] < box[4] || box[2] < box[5]) CHECK(given);
        n_given += given;
        n++;
    }
    CHECK(n_given > n / 2);
    {
        /* no range: the box is the point; a coordinate of the box or of the point that is not finite; too many bins */
        float box[6] = {1.0f, 2.0f, 3.0f, 1.0f, 2.0f, 3.0f}, nanbox[6], p[3] = {1.0f, 2.0f, 3.0f};
        int kmin, kmax;
        CHECK(!pc_box_bin_range(box, p[0], p[1], p[2], 10.0f, &kmin, &kmax));
        for (a = 0; a < 6; a++) nanbox[a] = NAN;
        CHECK(!pc_box_bin_range(nanbox, 0.0f, 0.0f, 0.0f, 10.0f, &kmin, &kmax));
        box[3] = 2.0f;
        CHECK(pc_box_bin_range(box, p[0], p[1], p[2], 10.0f, &kmin, &kmax) && kmin == 0 && kmax >= 10);
        CHECK(!pc_box_bin_range(box, NAN, p[1], p[2], 10.0f, &kmin, &kmax));
        CHECK(!pc_box_bin_range(box, p[0], INFINITY, p[2], 10.0f, &kmin, &kmax));
        CHECK(!pc_box_bin_range(box, p[0], p[1], -INFINITY, 10.0f, &kmin, &kmax));
        box[3] = INFINITY;
        CHECK(!pc_box_bin_range(box, p[0], p[1], p[2], 10.0f, &kmin, &kmax));
        box[3] = 2.0f;
        box[0] = NAN;
        CHECK(!pc_box_bin_range(box, p[0], p[1], p[2], 10.0f, &kmin, &kmax));
        box[0] = 1.0f;
        CHECK(!pc_box_bin_range(box, p[0], p[1], p[2], 4.0e6f, &kmin, &kmax));
    }
    printf("box_bound_check ok: %ld of %ld cases with a range\n", n_given, n);
    return 0;
}
