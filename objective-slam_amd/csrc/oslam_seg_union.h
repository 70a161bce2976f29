/*
 * oslam_seg_union.h -- the lock-free union-find of the segments stage (include/oslam.h at oslam_view_segments): find and
 * union over an array L of n parents, for k_seg_tile (L in LDS, local indices), k_seg_seam and k_seg_flatten (L in HBM,
 * pixel indices) and, with host atomics, for tests/native/seg_union_check.c.
 *
 * Invariant.  An entry is either OSLAM_SEG_NONE (the pixel is not in: it is never passed to find or union and never
 * changes) or a parent L[i] <= i, at all times.  It holds at the start (L[i] = i) and every store while unions are in
 * flight is atomicMin(&L[hi], lo) with lo < hi, which can only lower an entry: L[hi] stays <= hi.  i is a root iff
 * L[i] == i.  A root can only stop being one, never become one again, and since parents only point downwards the
 * smallest index of a component is always a root: when all unions have ended, find(i) is the component's smallest index.
 *
 * Termination.  find follows i -> L[i] while L[i] < i: a strictly decreasing chain of indices, at most i steps, whatever
 * other threads store meanwhile.  union(a, b) holds a pair (hi, lo) of indices that were roots when read, lo < hi, and
 * does old = atomicMin(&L[hi], lo).  old == hi: hi was still a root and now hangs under lo; done.  Otherwise another
 * thread had hung hi under old < hi first.  The entry now holds min(old, lo): the link hi -> lo or hi -> old that was
 * not stored is owed, and union(old, lo) pays it: the loop goes on with find(old), find(lo).  The larger index of the
 * pair is at most max(old, lo) < hi: it strictly decreases from one round to the next and is bounded below by 0, so the
 * loop ends after at most hi rounds; it also ends when the two roots meet.  No thread waits for another: there is no
 * lock and no spin on a value someone else must write, so a wave that is never scheduled again cannot hold up the rest.
 *
 * Bounds.  Every index is checked against n before any load or store; an index outside ends the call.
 */
#ifndef OSLAM_SEG_UNION_H
#define OSLAM_SEG_UNION_H

#include <stdint.h>

#define OSLAM_SEG_NONE 0xffffffffu

#if defined(__HIPCC__)
#define OSLAM_SEG_FN __device__ __forceinline__
#ifndef OSLAM_SEG_ATOMIC_MIN
#define OSLAM_SEG_ATOMIC_MIN(p, v) atomicMin((p), (v))
#endif
#else
#define OSLAM_SEG_FN static inline
#ifndef OSLAM_SEG_ATOMIC_MIN
/* the host's: a compare-and-swap loop that returns the value before, as atomicMin does */
static inline uint32_t oslam_seg_host_min(uint32_t *p, uint32_t v)
{
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
    return old;
}
#define OSLAM_SEG_ATOMIC_MIN(p, v) oslam_seg_host_min((p), (v))
#endif
#endif
/* a load that the compiler may not merge with an earlier one: other threads lower entries meanwhile */
#define OSLAM_SEG_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)

/* the root above i as the array stands: i itself when i >= n or its entry is OSLAM_SEG_NONE */
OSLAM_SEG_FN uint32_t oslam_seg_find(const uint32_t *L, uint32_t i, uint32_t n)
{
    while (i < n) {
        const uint32_t p = OSLAM_SEG_LOAD(&L[i]);
        if (p >= i) break;
        i = p;
    }
    return i;
}

/* joins the components of a and b */
OSLAM_SEG_FN void oslam_seg_union(uint32_t *L, uint32_t a, uint32_t b, uint32_t n)
{
    while (a < n && b < n) {
        a = oslam_seg_find(L, a, n);
        b = oslam_seg_find(L, b, n);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = OSLAM_SEG_ATOMIC_MIN(&L[hi], lo);
        if (old >= hi) return;          /* hi was a root (old == hi) and hangs under lo now; old > hi: not an in pixel */
        a = old;
        b = lo;
    }
}

#endif /* OSLAM_SEG_UNION_H */
