/*
 * oslam_refine.hip -- the refinement stage's kernels (semantics: include/oslam.h at oslam_refine; host side:
 * oslam_refine.c).
 *
 *   scene grid     k_grid_count (cell and rank of every scene point, integer atomics), k_scan_local +
 *                  k_scan_top (exclusive scan of the cell counts: 4096 cells per workgroup, then the block
 *                  totals in one workgroup; the scan over a workgroup is oslam_block_scan.h's), k_grid_scatter
 *                  (cell starts, points in cell order)
 *   correspond     k_refine_corr: one thread per model point, every member of the call in one grid (y = member,
 *                  x = block of 256 model points); the transform (oslam_icp_core.h), the 27-cell walk, then the 29
 *                  (step) or 2 (score) partial sums through the fixed wave64 shuffle tree and the fixed LDS order of
 *                  oslam_icp_block_sums into a (member, workgroup) slab.  No float atomics: the sums are bitwise
 *                  reproducible
 *   solve          k_refine_solve: one wave per member sums its slab in double in workgroup order, solves the 6x6
 *                  system by Cholesky and updates the double pose
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_block_scan.h"
#include "oslam_icp_core.h"
#include "oslam_kernels.h"
#include "oslam_refine_step.h"

/* ---------------------------------------------------------------- scene grid */
__device__ __forceinline__ int grid_axis(float x, double lo, double inv, int dim)
{
    double f = floor(((double)x - lo) * inv);
    f = fmin(fmax(f, -2.0), (double)dim + 1.0);       /* far outside (or NaN): a cell the walk clamps away */
    return (int)f;
}

__global__ __launch_bounds__(256) void k_grid_count(const oslamk_grid g, oslamk_cloud c)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    int cx = grid_axis(c.px[i], g.lo[0], g.inv_edge, g.dim[0]);
    int cy = grid_axis(c.py[i], g.lo[1], g.inv_edge, g.dim[1]);
    int cz = grid_axis(c.pz[i], g.lo[2], g.inv_edge, g.dim[2]);
    cx = min(max(cx, 0), g.dim[0] - 1);
    cy = min(max(cy, 0), g.dim[1] - 1);
    cz = min(max(cz, 0), g.dim[2] - 1);
    const uint32_t cell = ((uint32_t)cz * (uint32_t)g.dim[1] + (uint32_t)cy) * (uint32_t)g.dim[0] + (uint32_t)cx;
    g.cell_of[i] = cell;
    g.rank[i] = atomicAdd(&g.local[cell], 1u);
}

/* local[0 .. n_items): exclusive scan inside each block of 4096 items, in place; bsum[block] = the block's total */
__global__ __launch_bounds__(256) void k_scan_local(uint32_t *local, uint32_t n_items, uint32_t *bsum)
{
    __shared__ uint32_t sh[4];
    const uint32_t base = blockIdx.x * OSLAMK_SCAN_ITEMS + threadIdx.x * 16u;
    uint32_t v[16], s = 0, tot;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        v[k] = base + k < n_items ? local[base + k] : 0u;
        s += v[k];
    }
    uint32_t run = block_excl_scan<4>(s, sh, &tot);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (base + k < n_items) local[base + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

/* bsum[0 .. nb): exclusive scan in place, one workgroup of 1024 threads (nb <= 1024 * 8) */
__global__ __launch_bounds__(1024) void k_scan_top(uint32_t *bsum, uint32_t nb)
{
    __shared__ uint32_t sh[16];
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t base = threadIdx.x * per;
    uint32_t s = 0, tot;
    for (uint32_t k = 0; k < per; k++)
        if (base + k < nb) s += bsum[base + k];
    uint32_t run = block_excl_scan<16>(s, sh, &tot);
    for (uint32_t k = 0; k < per; k++)
        if (base + k < nb) {
            const uint32_t x = bsum[base + k];
            bsum[base + k] = run;
            run += x;
        }
}

__global__ __launch_bounds__(256) void k_grid_scatter(const oslamk_grid g, oslamk_cloud c)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= g.n_cells) g.start[i] = g.local[i] + g.bsum[i / OSLAMK_SCAN_ITEMS];
    if (i < (uint32_t)c.n) {
        const uint32_t cell = g.cell_of[i];
        const uint32_t pos = g.local[cell] + g.bsum[cell / OSLAMK_SCAN_ITEMS] + g.rank[i];
        float4 *dst = reinterpret_cast<float4 *>(g.pts) + 2 * (size_t)pos;
        dst[0] = make_float4(c.px[i], c.py[i], c.pz[i], __int_as_float((int)i));
        dst[1] = make_float4(c.nx[i], c.ny[i], c.nz[i], 0.0f);
    }
}

/* ---------------------------------------------------------------- correspondences + partial sums */
template <int MODE>
__global__ __launch_bounds__(OSLAMK_REFINE_THREADS) void k_refine_corr(const oslamk_grid g, const oslamk_refine_member *mem,
                                                                      uint32_t max_blocks, float *slab, int32_t *idx_out)
{
    constexpr int NS = MODE == OSLAMK_REFINE_STEP ? OSLAMK_REFINE_SUMS : 2;
    constexpr int STRIDE = MODE == OSLAMK_REFINE_STEP ? OSLAMK_REFINE_STRIDE : 2;
    __shared__ float sh[OSLAMK_REFINE_THREADS / 64][NS];
    const uint32_t j = blockIdx.y;
    const oslamk_refine_member *d = &mem[j];
    /* whole workgroups leave together: the conditions depend on the block only */
    if (MODE == OSLAMK_REFINE_STEP && d->done) return;
    if (MODE == OSLAMK_REFINE_SCORE && !d->active) return;
    if (blockIdx.x >= d->n_blocks) return;
    const int i = (int)(blockIdx.x * OSLAMK_REFINE_THREADS + threadIdx.x);
    const float4 *pts = reinterpret_cast<const float4 *>(g.pts);

    float s[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) s[k] = 0.0f;

    if (i < d->m.n) {
        const float r2 = MODE == OSLAMK_REFINE_SCORE ? d->r2_score : d->r2_corr;
        const float min_dot = d->min_dot;
        float q[3], m[3];
        oslam_icp_transform(d->Tf, d->m.px[i], d->m.py[i], d->m.pz[i], d->m.nx[i], d->m.ny[i], d->m.nz[i], q, m);
        const float qx = q[0], qy = q[1], qz = q[2], mx = m[0], my = m[1], mz = m[2];

        const int cx = grid_axis(qx, g.lo[0], g.inv_edge, g.dim[0]);
        const int cy = grid_axis(qy, g.lo[1], g.inv_edge, g.dim[1]);
        const int cz = grid_axis(qz, g.lo[2], g.inv_edge, g.dim[2]);
        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dim[0] - 1);
        const int y0 = max(cy - 1, 0), y1 = min(cy + 1, g.dim[1] - 1);
        const int z0 = max(cz - 1, 0), z1 = min(cz + 1, g.dim[2] - 1);
        float best = INFINITY;
        int best_idx = 0x7fffffff;
        uint32_t best_pos = 0;
        if (x0 <= x1 && y0 <= y1 && z0 <= z1) {
            for (int zz = z0; zz <= z1; zz++)
                for (int yy = y0; yy <= y1; yy++) {
                    const uint32_t row = ((uint32_t)zz * (uint32_t)g.dim[1] + (uint32_t)yy) * (uint32_t)g.dim[0];
                    const uint32_t e = g.start[row + (uint32_t)x1 + 1u];
                    for (uint32_t k = g.start[row + (uint32_t)x0]; k < e; k++) {
                        const float4 a = pts[2 * (size_t)k];
                        const float dx = a.x - qx, dy = a.y - qy, dz = a.z - qz;
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        if (!(d2 <= r2)) continue;
                        const float4 b = pts[2 * (size_t)k + 1];
                        const float dot = (mx * b.x + my * b.y) + mz * b.z;
                        const int idx = __float_as_int(a.w);
                        if (dot >= min_dot && (d2 < best || (d2 == best && idx < best_idx))) {
                            best = d2;
                            best_idx = idx;
                            best_pos = k;
                        }
                    }
                }
        }
        const bool found = best_idx != 0x7fffffff;
        if (MODE == OSLAMK_REFINE_TAP) {
            idx_out[i] = found ? best_idx : -1;
        } else if (MODE == OSLAMK_REFINE_SCORE) {
            if (found) {
                s[0] = 1.0f;
                s[1] = best;
            }
        } else if (found) {
            const float4 a = pts[2 * (size_t)best_pos];
            const float4 b = pts[2 * (size_t)best_pos + 1];
            oslam_refine_point_sums(qx, qy, qz, a, b, d->c, s);
        }
    }
    if (MODE == OSLAMK_REFINE_TAP) return;

    /* fixed-order reduction: shuffle tree inside each wave, then the waves in index order */
    const float sum = oslam_icp_block_sums<NS>(s, sh);
    if (threadIdx.x < NS) slab[((size_t)j * max_blocks + blockIdx.x) * STRIDE + threadIdx.x] = sum;
}

/* ---------------------------------------------------------------- solve */
__device__ void member_stop(oslamk_refine_member *d, uint32_t *n_done)
{
    d->done = 1;
    atomicAdd(n_done, 1u);
}

__global__ __launch_bounds__(64) void k_refine_solve(oslamk_refine_member *mem, uint32_t max_blocks, const float *slab,
                                                     uint32_t *n_done)
{
    __shared__ double S[OSLAMK_REFINE_SUMS];
    oslamk_refine_member *d = &mem[blockIdx.x];
    if (d->done) return;
    const int lane = threadIdx.x;
    if (lane < OSLAMK_REFINE_SUMS) {
        const float *p = slab + (size_t)blockIdx.x * max_blocks * OSLAMK_REFINE_STRIDE + lane;
        double acc = 0.0;
        for (uint32_t b = 0; b < d->n_blocks; b++) acc += (double)p[(size_t)b * OSLAMK_REFINE_STRIDE];
        S[lane] = acc;
    }
    __syncthreads();
    if (lane != 0) return;

    d->n_corr = (int32_t)S[27];
    double th, vn;
    if (!oslam_refine_step(S, d->T, d->cm, d->Tf, d->c, &th, &vn)) { member_stop(d, n_done); return; }
    d->iterations += 1;
    if (th < (double)d->stop_rot && vn < (double)d->stop_trans) {
        d->converged = 1;
        member_stop(d, n_done);
    } else if ((uint32_t)d->iterations >= d->max_iter) {
        member_stop(d, n_done);
    }
}

/* ---------------------------------------------------------------- launchers */
extern "C" int oslamk_refine_grid_build(const oslamk_grid *g, oslamk_cloud c, void *stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t n_items = g->n_cells + 1u;
    const uint32_t nb = (n_items + OSLAMK_SCAN_ITEMS - 1) / OSLAMK_SCAN_ITEMS;
    const uint32_t n_threads = (n_items > (uint32_t)c.n ? n_items : (uint32_t)c.n);
    hipError_t e;
    if (c.n <= 0 || g->n_cells == 0 || g->n_cells > OSLAMK_GRID_MAX_CELLS || nb > 1024u * 8u) return (int)hipErrorInvalidValue;
    e = hipMemsetAsync(g->local, 0, sizeof(uint32_t) * n_items, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_grid_count, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, stream, *g, c);
    hipLaunchKernelGGL(k_scan_local, dim3(nb), dim3(256), 0, stream, g->local, n_items, g->bsum);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, stream, g->bsum, nb);
    hipLaunchKernelGGL(k_grid_scatter, dim3((n_threads + 255) / 256), dim3(256), 0, stream, *g, c);
    return (int)hipGetLastError();
}

extern "C" int oslamk_refine_corr(int mode, const oslamk_grid *g, const oslamk_refine_member *d_mem, uint32_t n_mem,
                                  uint32_t max_blocks, float *slab, int32_t *idx_out, void *stream)
{
    if (n_mem == 0 || max_blocks == 0) return 0;
    if (n_mem > 65535u) return (int)hipErrorInvalidValue;
    const dim3 grid(max_blocks, n_mem);
    if (mode == OSLAMK_REFINE_STEP)
        hipLaunchKernelGGL(k_refine_corr<OSLAMK_REFINE_STEP>, grid, dim3(OSLAMK_REFINE_THREADS), 0, (hipStream_t)stream, *g,
                           d_mem, max_blocks, slab, idx_out);
    else if (mode == OSLAMK_REFINE_SCORE)
        hipLaunchKernelGGL(k_refine_corr<OSLAMK_REFINE_SCORE>, grid, dim3(OSLAMK_REFINE_THREADS), 0, (hipStream_t)stream, *g,
                           d_mem, max_blocks, slab, idx_out);
    else
        hipLaunchKernelGGL(k_refine_corr<OSLAMK_REFINE_TAP>, grid, dim3(OSLAMK_REFINE_THREADS), 0, (hipStream_t)stream, *g,
                           d_mem, max_blocks, slab, idx_out);
    return (int)hipGetLastError();
}

extern "C" int oslamk_refine_solve(oslamk_refine_member *d_mem, uint32_t n_mem, uint32_t max_blocks, const float *slab,
                                   uint32_t *n_done, void *stream)
{
    if (n_mem == 0) return 0;
    hipLaunchKernelGGL(k_refine_solve, dim3(n_mem), dim3(64), 0, (hipStream_t)stream, d_mem, max_blocks, slab, n_done);
    return (int)hipGetLastError();
}
