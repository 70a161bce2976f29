/*
 * oslam_segments.hip -- the segments stage's kernels (semantics: include/oslam.h at oslam_view_segments; host side:
 * oslam_segments.c; the union-find and its termination argument: oslam_seg_union.h).  A call enqueues six kernels,
 * whatever the image holds:
 *
 *   k_seg_tile     one workgroup of 256 threads per 32 x 32 pixel tile, four pixels a thread (rows ly, ly + 8, ..).  z and
 *                  the in flag are staged in LDS (a pixel that is not in holds z = 0), then a union-find over the tile's
 *                  1024 local indices in LDS: every in pixel is joined with its right and its lower neighbour inside the
 *                  tile when the gate passes, by atomicMin on LDS.  After a barrier every pixel finds its local root and
 *                  the pixels per local root are counted in LDS (one atomic per wave when all its in pixels share a root,
 *                  the usual case; one per pixel otherwise).  L[i] = the pixel index of the local root, tcount[i] = the
 *                  count at a local root and 0 elsewhere.  LDS 12 KiB.
 *   k_seg_seam     one thread per pixel pair across a tile border, first the vertical borders (x = 32, 64, ..), then the
 *                  horizontal ones.  A joined pair is merged by oslam_seg_union on L in HBM.
 *   k_seg_flatten  one thread per pixel: L[i] = find(i).  Unions have ended with the kernel before, so the plain store
 *                  only shortens a chain that other threads may be walking: every value an entry takes is an ancestor.
 *                  A tile-local root adds its count to count[final root]: one integer atomic per tile and local component,
 *                  not one per pixel.  The in pixels are counted by ballot.
 *   k_seg_collect  one thread per pixel: a root (L[i] == i) is counted; with count >= min_pixels it takes the next place
 *                  of the candidate list (places past OSLAMK_SEG_CAND are counted and not written).
 *   k_seg_rank     one workgroup of 1024 threads.  The keys pixels << 32 | ~root go into LDS (32 KiB); a candidate's rank
 *                  is the number of larger keys.  The keys are distinct, so the ranks are a permutation and the order in
 *                  which the list was filled cannot matter.  Ranks below max_segments preset their record and leave
 *                  1 << 31 | rank in count[root] (a count is at most 2^28).  More than OSLAMK_SEG_CAND candidates set
 *                  `overflow` instead, and k_seg_label leaves at once.
 *   k_seg_label    one thread per pixel in 32 x 8 tiles: the label is the rank in count[L[i]] or -1.  Bounding boxes and
 *                  centroid sums are reduced per wave over the lanes with equal labels (a loop over the distinct labels of
 *                  the wave, six shuffle steps each) before one lane adds them with integer atomicMin, atomicMax and
 *                  atomicAdd.
 *
 * The shape is the issue's; the counts go through a second array (tcount) rather than staying in LDS between k_seg_tile
 * and k_seg_flatten, because LDS does not outlive a kernel.
 *
 * No float atomics, no scratch.  Every result is an integer, so nothing depends on the order of pixels, waves or
 * workgroups; the gate is one float32 expression and -ffp-contract=off keeps its operations apart: the results equal
 * tests/segments_ref.py byte for byte.
 *
 * Bounds.  w, h <= 16384, so a pixel index is below 2^28 and fits the uint32 entries of L.  (u, v) is checked against
 * (w, h), or i against w * h, before any load or store; a local index is below 1024 by construction (lx < 31 before
 * li + 1, ly < 31 before li + 32); a root read from L or a candidate's root is checked against w * h before it indexes
 * count; a rank below max_segments <= OSLAMK_SEG_MAX indexes acc; a candidate place is checked against OSLAMK_SEG_CAND.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam.h"
#include "oslam_depth_normal.h"
#include "oslam_kernels.h"
#include "oslam_seg_union.h"

#define SEG_THREADS 256
#define SEG_TILE OSLAMK_SEG_TILE
#define SEG_TILE_PIX (SEG_TILE * SEG_TILE)
#define SEG_RANK_THREADS 1024
#define SEG_RANKED 0x80000000u

/* the edge rule, float32 with this grouping */
__device__ __forceinline__ bool seg_joined(float za, float zb, float max_step, float rel_step)
{
    return fabsf(za - zb) <= max_step + rel_step * fminf(za, zb);
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_tile(const oslamk_seg_args a)
{
    __shared__ float sz[SEG_TILE_PIX];
    __shared__ uint32_t sp[SEG_TILE_PIX], sc[SEG_TILE_PIX];
    const int x0 = (int)blockIdx.x * SEG_TILE, y0 = (int)blockIdx.y * SEG_TILE;
    const int lx = (int)threadIdx.x & 31, ly0 = (int)threadIdx.x >> 5;
    const int u = x0 + lx;

#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int li = (int)threadIdx.x + SEG_THREADS * k, v = y0 + ly0 + 8 * k;
        float z = 0.0f;
        if (u < a.v.w && v < a.v.h) {
            const size_t i = (size_t)v * a.v.w + u;
            z = a.v.z[i];
            if (!(z > 0.0f) || (a.plane_labels && a.plane_labels[i] >= 0)) z = 0.0f;
        }
        sz[li] = z;
        sp[li] = z > 0.0f ? (uint32_t)li : OSLAM_SEG_NONE;
        sc[li] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int li = (int)threadIdx.x + SEG_THREADS * k, ly = ly0 + 8 * k;
        const float z = sz[li];
        if (z > 0.0f) {
            if (lx < SEG_TILE - 1) {
                const float zr = sz[li + 1];
                if (zr > 0.0f && seg_joined(z, zr, a.max_step, a.rel_step)) oslam_seg_union(sp, (uint32_t)li, (uint32_t)li + 1, SEG_TILE_PIX);
            }
            if (ly < SEG_TILE - 1) {
                const float zd = sz[li + SEG_TILE];
                if (zd > 0.0f && seg_joined(z, zd, a.max_step, a.rel_step)) oslam_seg_union(sp, (uint32_t)li, (uint32_t)li + SEG_TILE, SEG_TILE_PIX);
            }
        }
    }
    __syncthreads();
    uint32_t r[4];
    const int lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int li = (int)threadIdx.x + SEG_THREADS * k;
        const bool on = sz[li] > 0.0f;
        r[k] = on ? oslam_seg_find(sp, (uint32_t)li, SEG_TILE_PIX) : OSLAM_SEG_NONE;
        const unsigned long long m = __ballot(on);
        if (m) {
            const int first = __ffsll((long long)m) - 1;
            const uint32_t r0 = (uint32_t)__shfl((int)r[k], first);
            if (__ballot(on && r[k] == r0) == m) {
                if (lane == first) atomicAdd(&sc[r0], (uint32_t)__popcll(m));
            } else if (on) {
                atomicAdd(&sc[r[k]], 1u);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int li = (int)threadIdx.x + SEG_THREADS * k, v = y0 + ly0 + 8 * k;
        if (u < a.v.w && v < a.v.h) {
            const size_t i = (size_t)v * a.v.w + u;
            uint32_t g = OSLAM_SEG_NONE, c = 0;
            if (r[k] != OSLAM_SEG_NONE) {
                g = (uint32_t)(y0 + (int)(r[k] >> 5)) * (uint32_t)a.v.w + (uint32_t)(x0 + (int)(r[k] & 31));
                c = r[k] == (uint32_t)li ? sc[li] : 0u;
            }
            a.L[i] = g;
            a.tcount[i] = c;
        }
    }
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_seam(const oslamk_seg_args a, uint32_t n_vert, uint32_t n_pairs)
{
    uint32_t t = blockIdx.x * SEG_THREADS + threadIdx.x;
    if (t >= n_pairs) return;
    const uint32_t w = (uint32_t)a.v.w, h = (uint32_t)a.v.h, n_pix = w * h;
    uint32_t i, j;
    if (t < n_vert) {                               /* (x - 1, y) | (x, y) at x = 32 (b + 1) */
        const uint32_t b = t / h, y = t - b * h, x = (b + 1) * SEG_TILE;
        if (x >= w) return;
        j = y * w + x;
        i = j - 1;
    } else {                                        /* (x, y - 1) | (x, y) at y = 32 (b + 1) */
        t -= n_vert;
        const uint32_t b = t / w, x = t - b * w, y = (b + 1) * SEG_TILE;
        if (y >= h) return;
        j = y * w + x;
        i = j - w;
    }
    if (j >= n_pix) return;
    if (OSLAM_SEG_LOAD(&a.L[i]) == OSLAM_SEG_NONE || OSLAM_SEG_LOAD(&a.L[j]) == OSLAM_SEG_NONE) return;
    if (seg_joined(a.v.z[i], a.v.z[j], a.max_step, a.rel_step)) oslam_seg_union(a.L, i, j, n_pix);
}

/* adds the popcount of a wave's ballot over the workgroup's four waves into *dst: one atomic per workgroup */
__device__ __forceinline__ void seg_count(bool flag, uint32_t *sh, uint32_t *dst)
{
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (s) atomicAdd(dst, s);
    }
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_flatten(const oslamk_seg_args a)
{
    __shared__ uint32_t sh[SEG_THREADS / 64];
    const uint32_t n_pix = (uint32_t)a.v.w * (uint32_t)a.v.h, i = blockIdx.x * SEG_THREADS + threadIdx.x;
    bool in = false;
    if (i < n_pix) {
        in = OSLAM_SEG_LOAD(&a.L[i]) != OSLAM_SEG_NONE;
        if (in) {
            const uint32_t r = oslam_seg_find(a.L, i, n_pix);
            a.L[i] = r;
            const uint32_t c = a.tcount[i];
            if (c) atomicAdd(&a.count[r], c);
        }
    }
    seg_count(in, sh, &a.blk->valid_in);
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_collect(const oslamk_seg_args a)
{
    __shared__ uint32_t sh[SEG_THREADS / 64];
    const uint32_t n_pix = (uint32_t)a.v.w * (uint32_t)a.v.h, i = blockIdx.x * SEG_THREADS + threadIdx.x;
    bool root = false;
    if (i < n_pix) {
        root = a.L[i] == i;
        if (root) {
            const uint32_t c = a.count[i];
            if (c >= a.min_pixels) {
                const uint32_t slot = atomicAdd(&a.blk->n_candidates, 1u);
                if (slot < OSLAMK_SEG_CAND) {
                    a.blk->cand[slot][0] = c;
                    a.blk->cand[slot][1] = i;
                }
            }
        }
    }
    seg_count(root, sh, &a.blk->n_components);
}

__global__ __launch_bounds__(SEG_RANK_THREADS) void k_seg_rank(const oslamk_seg_args a)
{
    __shared__ unsigned long long key[OSLAMK_SEG_CAND];
    const uint32_t nc = a.blk->n_candidates, n_pix = (uint32_t)a.v.w * (uint32_t)a.v.h;
    if (nc > OSLAMK_SEG_CAND) {                     /* the same in every thread */
        if (threadIdx.x == 0) a.blk->overflow = 1;
        return;
    }
    for (uint32_t j = threadIdx.x; j < nc; j += SEG_RANK_THREADS)
        key[j] = ((unsigned long long)a.blk->cand[j][0] << 32) | (unsigned long long)(0xffffffffu - a.blk->cand[j][1]);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nc; j += SEG_RANK_THREADS) {
        const unsigned long long k = key[j];
        uint32_t rank = 0;
        for (uint32_t m = 0; m < nc; m++) rank += key[m] > k ? 1u : 0u;   /* the same address in every lane: a broadcast */
        const uint32_t root = 0xffffffffu - (uint32_t)k;
        if (rank < a.max_segments && rank < OSLAMK_SEG_MAX && root < n_pix) {
            oslamk_seg_acc *o = &a.blk->acc[rank];
            o->pixels = (uint32_t)(k >> 32);
            o->root = root;
            o->u0 = 0xffffffffu;
            o->v0 = 0xffffffffu;
            o->u1 = 0;
            o->v1 = 0;
            o->n = 0;
            o->pad = 0;
            o->s[0] = 0;
            o->s[1] = 0;
            o->s[2] = 0;
            a.count[root] = SEG_RANKED | rank;
        }
    }
}

__global__ __launch_bounds__(SEG_THREADS) void k_seg_label(const oslamk_seg_args a)
{
    if (a.blk->overflow) return;                    /* the whole grid leaves together */
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), vv = blockIdx.y * 8 + (threadIdx.x >> 5);
    const uint32_t n_pix = (uint32_t)a.v.w * (uint32_t)a.v.h;
    int32_t lab = -1;
    bool ok = false;
    long long qx = 0, qy = 0, qz = 0;
    if (u < a.v.w && vv < a.v.h) {
        const size_t i = (size_t)vv * a.v.w + u;
        const uint32_t r = a.L[i];
        if (r < n_pix) {
            const uint32_t c = a.count[r];
            if (c & SEG_RANKED) lab = (int32_t)(c & ~SEG_RANKED);
        }
        a.labels[i] = lab;
        if (lab >= 0) {
            const depth_cam cam = {a.v.fx, a.v.fy, a.v.cx, a.v.cy, 1.0f, a.v.z_min, a.v.z_max, 0.0f};
            float p[3];
            back_project(u, vv, a.v.z[i], cam, p);
            const float fx = p[0] * OSLAMK_SEG_SCALE, fy = p[1] * OSLAMK_SEG_SCALE, fz = p[2] * OSLAMK_SEG_SCALE;
            /* the range test in float before the conversion: |q_a| <= 2^30, a sum over 2^28 pixels <= 2^58 */
            ok = fabsf(fx) <= OSLAMK_SEG_BOUND && fabsf(fy) <= OSLAMK_SEG_BOUND && fabsf(fz) <= OSLAMK_SEG_BOUND;
            if (ok) {
                qx = (long long)(int32_t)rintf(fx);
                qy = (long long)(int32_t)rintf(fy);
                qz = (long long)(int32_t)rintf(fz);
            }
        }
    }
    const int lane = (int)threadIdx.x & 63;
    unsigned long long todo = __ballot(lab >= 0);
    while (todo) {                                  /* one round per distinct label of the wave */
        const int first = __ffsll((long long)todo) - 1;
        const int32_t l0 = __shfl(lab, first);
        const bool mine = lab == l0;
        uint32_t u0 = mine ? (uint32_t)u : 0xffffffffu, v0 = mine ? (uint32_t)vv : 0xffffffffu;
        uint32_t u1 = mine ? (uint32_t)u : 0u, v1 = mine ? (uint32_t)vv : 0u;
        uint32_t n = mine && ok ? 1u : 0u;
        long long sx = mine ? qx : 0, sy = mine ? qy : 0, sz = mine ? qz : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            u0 = min(u0, (uint32_t)__shfl_xor((int)u0, off));
            v0 = min(v0, (uint32_t)__shfl_xor((int)v0, off));
            u1 = max(u1, (uint32_t)__shfl_xor((int)u1, off));
            v1 = max(v1, (uint32_t)__shfl_xor((int)v1, off));
            n += (uint32_t)__shfl_xor((int)n, off);
            sx += __shfl_xor(sx, off);
            sy += __shfl_xor(sy, off);
            sz += __shfl_xor(sz, off);
        }
        if (lane == first && (uint32_t)l0 < OSLAMK_SEG_MAX) {
            oslamk_seg_acc *o = &a.blk->acc[l0];
            atomicMin(&o->u0, u0);
            atomicMin(&o->v0, v0);
            atomicMax(&o->u1, u1);
            atomicMax(&o->v1, v1);
            if (n) {
                atomicAdd(&o->n, n);
                atomicAdd(&o->s[0], (unsigned long long)sx);
                atomicAdd(&o->s[1], (unsigned long long)sy);
                atomicAdd(&o->s[2], (unsigned long long)sz);
            }
        }
        todo &= ~__ballot(mine);
    }
}

extern "C" int oslamk_segments_find(const oslamk_seg_args *a, void *stream)
{
    if (a->v.w <= 0 || a->v.h <= 0 || a->v.w > 16384 || a->v.h > 16384 || !a->v.z || !a->L || !a->tcount || !a->count ||
        !a->labels || !a->blk || a->max_segments < 1 || a->max_segments > OSLAMK_SEG_MAX || a->min_pixels < 1)
        return (int)hipErrorInvalidValue;
    const uint32_t w = (uint32_t)a->v.w, h = (uint32_t)a->v.h, n_pix = w * h;
    const uint32_t tx = (w + SEG_TILE - 1) / SEG_TILE, ty = (h + SEG_TILE - 1) / SEG_TILE;
    const uint32_t n_vert = (tx - 1) * h, n_pairs = n_vert + (ty - 1) * w;
    const uint32_t seam_groups = n_pairs ? (n_pairs + SEG_THREADS - 1) / SEG_THREADS : 1u;   /* the count of launches is constant */
    const uint32_t pix_groups = (n_pix + SEG_THREADS - 1) / SEG_THREADS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_seg_tile, dim3(tx, ty), dim3(SEG_THREADS), 0, s, *a);
    hipLaunchKernelGGL(k_seg_seam, dim3(seam_groups), dim3(SEG_THREADS), 0, s, *a, n_vert, n_pairs);
    hipLaunchKernelGGL(k_seg_flatten, dim3(pix_groups), dim3(SEG_THREADS), 0, s, *a);
    hipLaunchKernelGGL(k_seg_collect, dim3(pix_groups), dim3(SEG_THREADS), 0, s, *a);
    hipLaunchKernelGGL(k_seg_rank, dim3(1), dim3(SEG_RANK_THREADS), 0, s, *a);
    hipLaunchKernelGGL(k_seg_label, dim3((w + 31) / 32, (h + 7) / 8), dim3(SEG_THREADS), 0, s, *a);
    return (int)hipGetLastError();
}
