/*
 * oslam_window.h -- the arithmetic of the shifting window, each rule stated once: the origin of a window at an offset,
 * the region that enters under a shift, a window voxel's global coordinate and back, the aligned bricks a window's box
 * overlaps, and the layout of a batch of records on its way between the window and the voxel store.  Host only, no HIP,
 * no error text: tests/native/window_check.c includes it alone.  Users: oslam_window.c, oslam_volume.c (reset) and
 * oslam_world_surface.c.  A window is its sides n[3] in voxels and its offset off[3]; global coordinates g are voxels
 * of the created volume's lattice (include/oslam.h at oslam_volume_shift).
 */
#ifndef OSLAM_WINDOW_H
#define OSLAM_WINDOW_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* the origin of the window at off, derived from the created origin and never accumulated (include/oslam.h at
 * oslam_volume_shift): one float multiply, then one float add.  An axis with off 0 keeps origin0's bits, -0.0f too */
static inline void oslam_window_origin(const float origin0[3], float voxel, const int off[3], float origin[3])
{
    int a;
    for (a = 0; a < 3; a++) {
        origin[a] = origin0[a];
        if (off[a] != 0) {
            const float step = (float)off[a] * voxel;
            origin[a] = origin0[a] + step;
        }
    }
}

/* The entering region, the window at off_new minus the window at off_old in global coordinates, as at most 7 disjoint
 * boxes lo <= g < hi: axis by axis, the slabs of what remains that lie outside the old window, then the rest restricted
 * to the overlap; all of what remains as soon as an axis has no overlap.  -> the number of boxes */
static inline int oslam_window_entering(const int off_old[3], const int off_new[3], const unsigned n[3], int32_t lo[7][3],
                                        int32_t hi[7][3])
{
    int a, nb = 0;
    int32_t cl[3], ch[3];
    for (a = 0; a < 3; a++) {
        cl[a] = off_new[a];
        ch[a] = off_new[a] + (int)n[a];
    }
    for (a = 0; a < 3; a++) {
        const int32_t ol = cl[a] > off_old[a] ? cl[a] : off_old[a];
        const int32_t oh = ch[a] < off_old[a] + (int)n[a] ? ch[a] : off_old[a] + (int)n[a];
        if (ol >= oh) {
            memcpy(lo[nb], cl, sizeof cl);
            memcpy(hi[nb], ch, sizeof ch);
            return nb + 1;
        }
        if (cl[a] < ol) {
            memcpy(lo[nb], cl, sizeof cl);
            memcpy(hi[nb], ch, sizeof ch);
            hi[nb++][a] = ol;
        }
        if (oh < ch[a]) {
            memcpy(lo[nb], cl, sizeof cl);
            memcpy(hi[nb], ch, sizeof ch);
            lo[nb++][a] = oh;
        }
        cl[a] = ol;
        ch[a] = oh;
    }
    return nb;                                                      /* what remains is the overlap: it does not enter */
}

/* the global coordinate of the voxel with linear index lin (x fastest) in the window n at off */
static inline void oslam_window_global(const unsigned n[3], const int off[3], uint32_t lin, int32_t g[3])
{
    const uint32_t row = lin / n[0];
    g[0] = (int32_t)(lin - row * n[0]) + off[0];
    g[1] = (int32_t)(row % n[1]) + off[1];
    g[2] = (int32_t)(row / n[1]) + off[2];
}

/* its inverse: the linear index of g, which lies in the window n at off */
static inline uint32_t oslam_window_lin(const unsigned n[3], const int off[3], const int32_t g[3])
{
    return (uint32_t)(((size_t)(g[2] - off[2]) * n[1] + (size_t)(g[1] - off[1])) * n[0] + (size_t)(g[0] - off[0]));
}

/* the aligned bricks of 8 x 8 x 8 voxels that the window's box overlaps: the first key and the number of keys per axis */
static inline void oslam_window_bricks(const unsigned n[3], const int off[3], int kb0[3], int nb[3])
{
    int a;
    for (a = 0; a < 3; a++) {
        kb0[a] = off[a] >> 3;                                       /* arithmetic: floor for a negative offset */
        nb[a] = ((off[a] + (int)n[a] - 1) >> 3) - kb0[a] + 1;
    }
}

/* A batch of n records, in HBM, in pinned memory and on the host link alike: [n][2] words {linear index, TSDF word}, then
 * [n] colour words when the batch is coloured: one buffer, so one copy moves both.  Its bytes, and the word at which
 * its colours start */
static inline size_t oslam_records_bytes(size_t n, int coloured) { return sizeof(uint32_t) * (coloured ? 3 : 2) * n; }
static inline size_t oslam_records_colours(size_t n) { return 2 * n; }

#endif /* OSLAM_WINDOW_H */
