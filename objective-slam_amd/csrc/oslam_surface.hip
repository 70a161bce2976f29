/*
 * oslam_surface.hip -- the fused surface of a TSDF volume as points with normals, all of it or the part that a shift of
 * the volume's window loses (semantics: include/oslam.h at oslam_volume_surface and oslam_volume_leaving; host side:
 * oslam_surface.c; sums and scans over a workgroup: oslam_block_scan.h; the edges and points: oslam_surf_edge.h).  The
 * volume is large and the surface small, so the volume is read twice and nothing proportional to the number of voxels is
 * stored.  The two passes are written once (surface_count, surface_emit) and compiled twice:
 *
 *   k_surface_count   a workgroup of 256 threads owns OSLAMK_SURF_RUN consecutive linear voxel indices, as
 *                     OSLAMK_SURF_ITEMS chunks of 256 (a wave reads 64 consecutive words per chunk).  A thread loads its
 *                     own words first; a wave none of whose words is seen does nothing more.  A seen voxel loads its
 *                     three neighbour words at +1, +nx and +nx*ny (only those that exist), tests the signs and, at a
 *                     crossing, makes the point and the six trilinear reads of its normal.  The workgroup's number of
 *                     points goes to counts[blockIdx.x] (block_sum, no atomic), the crossings are added as integers to
 *                     totals[0] (one integer atomic per wave: a count does not depend on the order).
 *   k_surface_scan    one workgroup turns counts[] into exclusive offsets in place, 256 at a time with a carry, and
 *                     leaves their sum in *total_out (oslamk_surface_scan runs it alone, for oslam_mesh.hip).
 *   k_surface_emit    recomputes.  The rank of a point is its rank in the chunk (surf_chunk_rank: voxel order, then
 *                     axis), plus the points of the earlier chunks, plus the workgroup's offset: ascending
 *                     3 * voxel + axis.  A workgroup none of whose words is seen returns after its loads.
 *   k_leave_count     the same two bodies with LEAVING set: the mask of a voxel's crossings is ANDed with the mask of its
 *   k_leave_emit      edges that have an end outside the window after the shift, before anything is counted or ranked.
 *                     That mask comes from the voxel's index alone, so a workgroup none of whose 1024 voxels has such an
 *                     edge returns before it loads a word (k_leave_count stores its zero count first: the scan reads it).
 * Bounds.  A voxel index is checked against nx*ny*nz before its word is loaded (the last workgroup's run is ragged); a
 * neighbour is loaded only when its coordinate is below n_a, which keeps idx + stride inside the volume and stops a row's
 * last voxel from reading the next row's first; the trilinear read checks its base corner in float before it becomes an
 * index (oslam_tsdf_read.h); a record's rank is checked against the number of points before it is stored.  The
 * launchers check the volume's sizes, the number of workgroups and the shift (at most 2^20 in size, so no coordinate
 * difference leaves int).  No scratch; 96 / 22 / 118 / 98 / 120 VGPRs, LDS 16 / 16 / 320 / 272 / 320 bytes
 * (profiles/r16_kernel_resources_surface_merged.txt).
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"
#include "oslam_surf_edge.h"

__device__ __forceinline__ bool leave_in(int c, int n) { return (unsigned)c < (unsigned)n; }

/* the edges of voxel idx (< n_vox) that leave under the shift, as a mask of axes: the edge exists and the voxel or the
 * edge's other end lies outside the window afterwards */
__device__ __forceinline__ uint32_t leave_edges(const oslamk_volume &vol, uint32_t idx, const oslamk_shift3 &sh)
{
    const uint32_t nx = (uint32_t)vol.nx, ny = (uint32_t)vol.ny, row = idx / nx;
    const int n[3] = {vol.nx, vol.ny, vol.nz};
    const int c[3] = {(int)(idx - row * nx), (int)(row % ny), (int)(row / ny)};
    const bool stays = leave_in(c[0] - sh.s[0], n[0]) && leave_in(c[1] - sh.s[1], n[1]) && leave_in(c[2] - sh.s[2], n[2]);
    uint32_t mask = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (c[a] + 1 < n[a] && !(stays && leave_in(c[a] + 1 - sh.s[a], n[a]))) mask |= 1u << a;
    return mask;
}

/* the leaving edges of a thread's voxels, three bits per chunk of its workgroup's run */
__device__ __forceinline__ uint32_t leave_load(const oslamk_volume &vol, uint32_t n_vox, const oslamk_shift3 &sh)
{
    uint32_t lv = 0;
#pragma unroll
    for (int it = 0; it < SURF_ITEMS; it++) {
        const uint32_t idx = surf_idx(it);
        if (idx < n_vox) lv |= leave_edges(vol, idx, sh) << (3 * it);
    }
    return lv;
}

/* The count pass.  LEAVING: only the crossings that the shift sh loses (lv: leave_load's mask; a workgroup without a
 * leaving edge stores its zero count and returns before any load); otherwise sh is not read and lv is all ones, which
 * the compiler folds away */
template <bool LEAVING>
__device__ __forceinline__ void surface_count(const oslamk_volume &vol, const oslamk_shift3 &sh, uint32_t min_w, uint32_t n_vox,
                                              uint32_t *counts, uint32_t *totals)
{
    __shared__ uint32_t s_pts[SURF_WAVES];
    uint32_t lv = ~0u;
    if (LEAVING) {
        lv = leave_load(vol, n_vox, sh);
        if (!__syncthreads_or(lv != 0u)) {
            if (threadIdx.x == 0) counts[blockIdx.x] = 0u;
            return;
        }
    }
    uint32_t w0[SURF_ITEMS], pts = 0, cross = 0;
    const bool any = surf_load(vol, n_vox, min_w, w0);
    if (__ballot(any && lv != 0u)) {
        for (int it = 0; it < SURF_ITEMS; it++) {
            const uint32_t lm = lv >> (3 * it) & 7u;
            if (!surf_seen(w0[it], min_w) || !lm) continue;
            int ijk[3];
            uint32_t nb[3];
            float rec[6];
            const uint32_t mask = surf_crossings(vol, surf_idx(it), w0[it], min_w, ijk, nb) & lm;
            cross += (uint32_t)__popc(mask);
#pragma unroll 1
            for (int a = 0; a < 3; a++)
                if ((mask >> a & 1u) && surf_point(vol, ijk, a, w0[it], surf_pick(nb, a), rec)) pts++;
        }
        cross = wave_sum(cross);
    }
    if ((threadIdx.x & 63u) == 0 && cross) atomicAdd(totals, cross);
    pts = block_sum<SURF_WAVES>(pts, s_pts);
    if (threadIdx.x == 0) counts[blockIdx.x] = pts;
}

/* The emit pass; LEAVING, sh and lv as in surface_count (a workgroup without a leaving edge returns before any load) */
template <bool LEAVING>
__device__ __forceinline__ void surface_emit(const oslamk_volume &vol, const oslamk_shift3 &sh, uint32_t min_w, uint32_t n_vox,
                                             const uint32_t *offsets, uint32_t n_points, float *out6)
{
    __shared__ uint32_t s_cnt[SURF_ITEMS][SURF_WAVES];
    uint32_t lv = ~0u;
    if (LEAVING) {
        lv = leave_load(vol, n_vox, sh);
        if (!__syncthreads_or(lv != 0u)) return;
    }
    uint32_t w0[SURF_ITEMS];
    const bool any = surf_load(vol, n_vox, min_w, w0) && lv != 0u;
    if (!__syncthreads_or(any)) return;
    const bool wave_any = __ballot(any) != 0ull;
    uint32_t run = offsets[blockIdx.x];
    for (int it = 0; it < SURF_ITEMS; it++) {
        float rec[3][6] = {};
        uint32_t has = 0, all;
        const uint32_t lm = lv >> (3 * it) & 7u;
        if (wave_any && surf_seen(w0[it], min_w) && lm) {
            int ijk[3];
            uint32_t nb[3];
            const uint32_t mask = surf_crossings(vol, surf_idx(it), w0[it], min_w, ijk, nb) & lm;
            /* one axis at a time (the three together cost 200 registers); the record goes to its row by selects */
#pragma unroll 1
            for (int a = 0; a < 3; a++) {
                float r[6];
                if (!((mask >> a & 1u) && surf_point(vol, ijk, a, w0[it], surf_pick(nb, a), r))) continue;
                has |= 1u << a;
#pragma unroll
                for (int c = 0; c < 6; c++) {
                    rec[0][c] = a == 0 ? r[c] : rec[0][c];
                    rec[1][c] = a == 1 ? r[c] : rec[1][c];
                    rec[2][c] = a == 2 ? r[c] : rec[2][c];
                }
            }
        }
        uint32_t rank = run + surf_chunk_rank(has, s_cnt[it], &all);
#pragma unroll
        for (int a = 0; a < 3; a++)
            if (has >> a & 1u) {
                if (rank < n_points) {
                    float2 *dst = reinterpret_cast<float2 *>(out6 + (size_t)rank * 6);
                    dst[0] = make_float2(rec[a][0], rec[a][1]);
                    dst[1] = make_float2(rec[a][2], rec[a][3]);
                    dst[2] = make_float2(rec[a][4], rec[a][5]);
                }
                rank++;
            }
        run += all;
    }
}

__global__ __launch_bounds__(SURF_T) void k_surface_count(const oslamk_volume vol, uint32_t min_w, uint32_t n_vox, uint32_t *counts,
                                                          uint32_t *totals)
{
    surface_count<false>(vol, oslamk_shift3{}, min_w, n_vox, counts, totals);
}

__global__ __launch_bounds__(SURF_T) void k_leave_count(const oslamk_volume vol, const oslamk_shift3 sh, uint32_t min_w, uint32_t n_vox,
                                                        uint32_t *counts, uint32_t *totals)
{
    surface_count<true>(vol, sh, min_w, n_vox, counts, totals);
}

__global__ __launch_bounds__(SURF_T) void k_surface_scan(uint32_t *counts, uint32_t n, uint32_t *total_out)
{
    __shared__ uint32_t s_wave[SURF_WAVES];
    uint32_t carry = 0;
    for (uint32_t tile = 0; tile < n; tile += SURF_T) {
        const uint32_t i = tile + threadIdx.x;
        uint32_t all;
        const uint32_t excl = block_excl_scan<SURF_WAVES>(i < n ? counts[i] : 0u, s_wave, &all);
        if (i < n) counts[i] = carry + excl;
        carry += all;
        __syncthreads();                                        /* the next tile stores to s_wave again */
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(SURF_T) void k_surface_emit(const oslamk_volume vol, uint32_t min_w, uint32_t n_vox,
                                                         const uint32_t *offsets, uint32_t n_points, float *out6)
{
    surface_emit<false>(vol, oslamk_shift3{}, min_w, n_vox, offsets, n_points, out6);
}

__global__ __launch_bounds__(SURF_T) void k_leave_emit(const oslamk_volume vol, const oslamk_shift3 sh, uint32_t min_w, uint32_t n_vox,
                                                       const uint32_t *offsets, uint32_t n_points, float *out6)
{
    surface_emit<true>(vol, sh, min_w, n_vox, offsets, n_points, out6);
}

extern "C" uint32_t oslamk_surface_groups(const oslamk_volume *vol)
{
    const uint32_t n_vox = (uint32_t)vol->nx * (uint32_t)vol->ny * (uint32_t)vol->nz;
    return (n_vox + OSLAMK_SURF_RUN - 1u) / OSLAMK_SURF_RUN;
}

extern "C" int oslamk_surface_count(const oslamk_volume *vol, const int *shift, uint32_t min_weight, uint32_t n_groups,
                                    uint32_t *counts, uint32_t *totals, void *stream)
{
    uint32_t n_vox;
    if (!surf_launch_ok(vol, min_weight, n_groups, &n_vox) || (shift && !oslamk_shift_ok(shift)) || !counts || !totals)
        return (int)hipErrorInvalidValue;
    if (shift) {
        const oslamk_shift3 sh = {{shift[0], shift[1], shift[2]}};
        hipLaunchKernelGGL(k_leave_count, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, sh, min_weight, n_vox, counts, totals);
    } else
        hipLaunchKernelGGL(k_surface_count, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, counts, totals);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : oslamk_surface_scan(counts, n_groups, totals + 1, stream);
}

extern "C" int oslamk_surface_scan(uint32_t *counts, uint32_t n, uint32_t *total_out, void *stream)
{
    if (!counts || !total_out || n == 0 || n > (1u << 17)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_surface_scan, dim3(1), dim3(SURF_T), 0, (hipStream_t)stream, counts, n, total_out);
    return (int)hipGetLastError();
}

extern "C" int oslamk_surface_emit(const oslamk_volume *vol, const int *shift, uint32_t min_weight, uint32_t n_groups,
                                   const uint32_t *offsets, uint32_t n_points, float *out6, void *stream)
{
    uint32_t n_vox;
    if (!surf_launch_ok(vol, min_weight, n_groups, &n_vox) || (shift && !oslamk_shift_ok(shift)) || !offsets || !out6 || n_points == 0)
        return (int)hipErrorInvalidValue;
    if (shift) {
        const oslamk_shift3 sh = {{shift[0], shift[1], shift[2]}};
        hipLaunchKernelGGL(k_leave_emit, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, sh, min_weight, n_vox, offsets,
                           n_points, out6);
    } else
        hipLaunchKernelGGL(k_surface_emit, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, offsets,
                           n_points, out6);
    return (int)hipGetLastError();
}
