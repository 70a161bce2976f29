/*
 * oslam_explain.hip -- the explain stage's kernels (semantics: include/oslam.h at oslam_explain; host side:
 * oslam_explain.c).
 *
 *   k_explain_splat   k_render_splat into private z-buffers: one thread per model point, every hypothesis of the call in
 *                     one grid (y = hypothesis, x = block of 256 model points, k_verify's grid over k_verify's
 *                     descriptors): transform, BACK, OUT (oslam_icp_core.h's, unchanged), the half-width k, then one
 *                     32-bit unsigned atomicMin of the bits of p'z into every pixel of the clipped window, inside the
 *                     hypothesis's own rectangle of the pool.  Alone in its buffer a hypothesis needs no label in the key.
 *                     The atomics return nothing and compile to global_atomic_umin, at most 17 x 17 a point.  A window
 *                     that leaves the rectangle is not written and counted in `clipped` (the host fails the call).
 *                     drawn and clipped: wave ballots + popcount, the four waves summed in LDS (32 bytes, the only LDS),
 *                     one integer atomicAdd per counter and workgroup.  No scratch.
 *   k_explain_score   one thread per pixel of a rectangle, a 32 x 8 block per workgroup (x, y = block of the largest
 *                     rectangle, z = hypothesis; the blocks beyond their own rectangle leave at once): Z_h against the
 *                     observed z, the class, the quantised residual.  Class counters by ballot + popcount and the
 *                     residuals by a wave shuffle tree, the four waves summed in LDS, one integer atomicAdd per counter
 *                     and workgroup.  Claims: one 64-bit atomicAdd per (wave, tile); the lanes of a wave that share a tile
 *                     are found by ballots, as k_render_resolve finds the lanes that share a label.
 *   k_explain_claims  one thread per table entry: cnt -> cnt << 40 | cnt * conflict_q of its hypothesis, from the
 *                     finished counters: the word k_arbitrate reads.
 *
 * Bounds.  k_explain_splat reads point i < m.n of its hypothesis only; the centre pixel is range-checked in float before
 * it becomes an int (oslam_icp_project), 0 <= k <= 8, the window is clipped to the image and then required to lie inside
 * the rectangle [x0, x0 + w) x [y0, y0 + h) before any write, so every atomic goes to a word in [off, off + w * h) of the
 * pool, which the host sized as the sum of w * h.  k_explain_score touches pixel (lx, ly) of a rectangle only when lx < w
 * and ly < h, reads the view at (x0 + lx, y0 + ly) only when that lies inside the image, and checks the tile index
 * against n_tiles before the atomic; the table index is < n_mem * n_tiles.  k_explain_claims touches entry e < n_mem *
 * n_tiles and rec[e / n_tiles], e / n_tiles < n_mem.  Pixel and table indices are size_t: a pool may reach 2^26 words
 * and a table 2^25 entries.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_icp_core.h"
#include "oslam_kernels.h"

typedef unsigned long long u64;
#define EXPLAIN_EMPTY 0xffffffffu
#define EXPLAIN_WAVES (OSLAMK_VERIFY_THREADS / 64)

__global__ __launch_bounds__(OSLAMK_VERIFY_THREADS) void k_explain_splat(const oslamk_view v, const oslamk_verify_member *mem,
                                                                         const float *rho, const oslamk_explain_rect *rect,
                                                                         int max_splat, int keep_back, uint32_t *pool,
                                                                         oslamk_explain_rec *rec)
{
    __shared__ uint32_t sh[EXPLAIN_WAVES][2];
    const uint32_t j = blockIdx.y;
    const oslamk_verify_member *d = &mem[j];
    if (blockIdx.x >= d->n_blocks) return;     /* the whole workgroup leaves together */
    const int i = (int)(blockIdx.x * OSLAMK_VERIFY_THREADS + threadIdx.x);
    bool draw = false, clip = false;

    if (i < d->m.n) {
        float q[3], m[3];
        int u, vv;
        oslam_icp_transform(d->T, d->m.px[i], d->m.py[i], d->m.pz[i], d->m.nx[i], d->m.ny[i], d->m.nz[i], q, m);
        const bool back = (m[0] * q[0] + m[1] * q[1]) + m[2] * q[2] >= 0.0f;
        if ((keep_back || !back) && oslam_icp_project(v, q, &u, &vv)) {
            const oslamk_explain_rect r = rect[j];
            const float kf = floorf((rho[j] * v.fx) / q[2] + 0.5f);
            const int k = kf < (float)max_splat ? (int)kf : max_splat;
            const int u0 = max(u - k, 0), u1 = min(u + k, v.w - 1);
            const int v0 = max(vv - k, 0), v1 = min(vv + k, v.h - 1);
            draw = true;
            if (r.w > 0 && r.h > 0 && u0 >= r.x0 && u1 - r.x0 < r.w && v0 >= r.y0 && v1 - r.y0 < r.h) {
                const uint32_t key = __float_as_uint(q[2]);
                for (int y = v0; y <= v1; y++) {
                    uint32_t *row = pool + (size_t)r.off + (size_t)(y - r.y0) * (size_t)r.w;
                    for (int x = u0; x <= u1; x++) atomicMin(&row[x - r.x0], key);
                }
            } else {
                clip = true;
            }
        }
    }

    const u64 b0 = __ballot(draw), b1 = __ballot(clip);
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6][0] = (uint32_t)__popcll(b0);
        sh[threadIdx.x >> 6][1] = (uint32_t)__popcll(b1);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t s = 0;
#pragma unroll
        for (int ww = 0; ww < EXPLAIN_WAVES; ww++) s += sh[ww][threadIdx.x];
        if (s) atomicAdd(threadIdx.x == 0 ? &rec[j].drawn : &rec[j].clipped, s);
    }
}

__global__ __launch_bounds__(256) void k_explain_score(const oslamk_view v, const oslamk_verify_member *mem,
                                                       const oslamk_explain_rect *rect, const uint32_t *pool,
                                                       const oslamk_arb_grid g, u64 *cnt, oslamk_explain_rec *rec)
{
    __shared__ uint32_t sh[4][5];
    const uint32_t j = blockIdx.z;
    const oslamk_explain_rect r = rect[j];
    /* uniform over the workgroup: a skipped hypothesis, or a block beyond this hypothesis's rectangle */
    if (mem[j].n_blocks == 0 || (int)(blockIdx.x * 32) >= r.w || (int)(blockIdx.y * 8) >= r.h) return;
    const int lx = (int)(blockIdx.x * 32) + (int)(threadIdx.x & 31), ly = (int)(blockIdx.y * 8) + (int)(threadIdx.x >> 5);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int cls = -1;                               /* 0 AGREE, 1 OCCLUDED, 2 THROUGH, 3 UNKNOWN; -1: nothing drawn here */
    uint32_t q = 0, tile = 0;

    if (lx < r.w && ly < r.h) {
        const uint32_t zb = pool[(size_t)r.off + (size_t)ly * (size_t)r.w + (size_t)lx];
        const int x = r.x0 + lx, y = r.y0 + ly;
        if (zb != EXPLAIN_EMPTY && x >= 0 && x < v.w && y >= 0 && y < v.h) {
            const float zh = __uint_as_float(zb), zo = v.z[(size_t)y * v.w + x];
            const float tol = mem[j].tol;
            const float dz = fabsf(zo - zh);
            if (zo == 0.0f) {
                cls = 3;
            } else if (dz <= tol) {
                const float xq = dz * (65535.0f / tol);
                cls = 0;
                q = xq < 65535.0f ? (uint32_t)xq : 65535u;
                tile = (uint32_t)(y / g.tile) * (uint32_t)g.tiles_x + (uint32_t)(x / g.tile);
            } else {
                cls = zo < zh ? 1 : 2;
            }
        }
    }

    /* every lane of the wave takes part in the ballots and shuffles, the ones without a pixel with nothing to count */
    const u64 b0 = __ballot(cls == 0), b1 = __ballot(cls == 1), b2 = __ballot(cls == 2), b3 = __ballot(cls == 3);
    uint32_t qs = q;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) qs += __shfl_down(qs, off);
    if (lane == 0) {
        sh[wv][0] = (uint32_t)__popcll(b0);
        sh[wv][1] = (uint32_t)__popcll(b1);
        sh[wv][2] = (uint32_t)__popcll(b2);
        sh[wv][3] = (uint32_t)__popcll(b3);
        sh[wv][4] = qs;                         /* at most 64 * 65535 */
    }

    bool pending = cls == 0 && tile < g.n_tiles;
    for (;;) {
        const u64 todo = __ballot(pending);
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t t0 = (uint32_t)__shfl((int)tile, leader);
        const u64 same = __ballot(pending && tile == t0);
        if (lane == leader) atomicAdd(&cnt[(size_t)j * g.n_tiles + t0], (u64)__popcll(same));
        if (tile == t0) pending = false;
    }

    __syncthreads();
    if (threadIdx.x < 5) {
        const uint32_t s = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
        if (s) {
            if (threadIdx.x < 4) atomicAdd(&rec[j].agree + threadIdx.x, s);   /* agree, occluded, through, unknown */
            else atomicAdd(&rec[j].resid_sum, (u64)s);
        }
    }
}

__global__ __launch_bounds__(256) void k_explain_claims(const oslamk_explain_rec *rec, uint32_t n_tiles, size_t n_ent, u64 *cnt)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    const u64 c = cnt[e];
    if (!c) return;
    const oslamk_explain_rec *r = &rec[e / n_tiles];
    const u64 a = r->agree, t = r->through;
    const u64 q = a ? (65535ull * t) / (a + t) : 0ull;
    cnt[e] = (c << OSLAMK_ARB_CNT_SHIFT) | (c * q);
}

static bool explain_grid_ok(const oslamk_view *v, oslamk_arb_grid g)
{
    return v->w > 0 && v->h > 0 && g.tile >= 4 && g.tile <= 128 && g.tiles_x >= 1 &&
           (uint32_t)g.tiles_x == (uint32_t)((v->w + g.tile - 1) / g.tile) &&
           g.n_tiles == (uint32_t)g.tiles_x * (uint32_t)((v->h + g.tile - 1) / g.tile);
}

extern "C" int oslamk_explain_splat(const oslamk_view *v, const oslamk_verify_member *d_mem, const float *d_rho,
                                    const oslamk_explain_rect *d_rect, uint32_t n_mem, uint32_t max_blocks, int max_splat,
                                    int keep_back, uint32_t *pool, oslamk_explain_rec *rec, void *stream)
{
    if (n_mem == 0 || max_blocks == 0) return 0;
    if (n_mem > OSLAMK_ARB_MAX_HYP || max_splat < 0 || max_splat > OSLAMK_RENDER_MAX_SPLAT || v->w <= 0 || v->h <= 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_explain_splat, dim3(max_blocks, n_mem), dim3(OSLAMK_VERIFY_THREADS), 0, (hipStream_t)stream, *v,
                       d_mem, d_rho, d_rect, max_splat, keep_back != 0, pool, rec);
    return (int)hipGetLastError();
}

extern "C" int oslamk_explain_score(const oslamk_view *v, const oslamk_verify_member *d_mem,
                                    const oslamk_explain_rect *d_rect, uint32_t n_mem, int max_w, int max_h,
                                    const uint32_t *pool, oslamk_arb_grid g, unsigned long long *cnt,
                                    oslamk_explain_rec *rec, void *stream)
{
    if (n_mem == 0 || n_mem > OSLAMK_ARB_MAX_HYP || max_w < 0 || max_h < 0 || max_w > v->w || max_h > v->h ||
        !explain_grid_ok(v, g))
        return (int)hipErrorInvalidValue;
    /* every rectangle empty: one block per hypothesis, which leaves at once */
    hipLaunchKernelGGL(k_explain_score, dim3(max_w ? (max_w + 31) / 32 : 1, max_h ? (max_h + 7) / 8 : 1, n_mem), dim3(256),
                       0, (hipStream_t)stream, *v, d_mem, d_rect, pool, g, cnt, rec);
    return (int)hipGetLastError();
}

extern "C" int oslamk_explain_claims(const oslamk_explain_rec *rec, uint32_t n_mem, uint32_t n_tiles,
                                     unsigned long long *cnt, void *stream)
{
    if (n_mem == 0 || n_mem > OSLAMK_ARB_MAX_HYP || n_tiles == 0) return (int)hipErrorInvalidValue;
    const size_t n_ent = (size_t)n_mem * n_tiles;
    hipLaunchKernelGGL(k_explain_claims, dim3((unsigned)((n_ent + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rec,
                       n_tiles, n_ent, cnt);
    return (int)hipGetLastError();
}
