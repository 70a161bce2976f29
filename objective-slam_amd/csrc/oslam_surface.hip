/*
 * oslam_surface.hip -- the fused surface of a TSDF volume as points with normals (semantics: include/oslam.h at
 * oslam_volume_surface; host side: oslam_volume.c).  The volume is large and the surface small, so the volume is read
 * twice and nothing proportional to the number of voxels is stored:
 *
 *   k_surface_count   a workgroup of 256 threads owns OSLAMK_SURF_RUN consecutive linear voxel indices, as
 *                     OSLAMK_SURF_ITEMS chunks of 256 (a wave reads 64 consecutive words per chunk).  A thread loads its
 *                     own words first; a wave none of whose words is seen does nothing more.  A seen voxel loads its
 *                     three neighbour words at +1, +nx and +nx*ny (only those that exist), tests the signs and, at a
 *                     crossing, makes the point and the six trilinear reads of its normal.  The workgroup's number of
 *                     points goes to counts[blockIdx.x] (a sum over the waves in LDS, no atomic), the crossings are
 *                     added as integers to totals[0] (one integer atomic per wave: a count does not depend on the order).
 *   k_surface_scan    one workgroup turns counts[] into exclusive offsets in place, 256 at a time with a carry, and
 *                     leaves the number of points in totals[1] (oslamk_surface_scan runs it alone, for oslam_mesh.hip).
 *   k_surface_emit    recomputes.  Per chunk the rank of a point is the points of the lower lanes (three ballots, one
 *                     per axis, and popcounts: voxel order, then axis), plus the points of the lower waves (LDS), plus
 *                     the points of the earlier chunks, plus the workgroup's offset: ascending 3 * voxel + axis.
 *                     A workgroup none of whose words is seen returns after its loads.
 * Bounds.  A voxel index is checked against nx*ny*nz before its word is loaded (the last workgroup's run is ragged); a
 * neighbour is loaded only when its coordinate is below n_a, which keeps idx + stride inside the volume and stops a row's
 * last voxel from reading the next row's first; the trilinear read checks its base corner in float before it becomes an
 * index (oslam_tsdf_read.h); a record's rank is checked against the number of points before it is stored.  The
 * launchers check the volume's sizes and the number of workgroups.  No scratch; 96 / 21 / 118 VGPRs, LDS 16 / 16 / 320
 * bytes (profiles/r09_kernel_resources_surface.txt).
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"
#include "oslam_surf_edge.h"

__global__ __launch_bounds__(SURF_T) void k_surface_count(const oslamk_volume vol, uint32_t min_w, uint32_t n_vox, uint32_t *counts,
                                                          uint32_t *totals)
{
    __shared__ uint32_t s_pts[SURF_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t w0[SURF_ITEMS], pts = 0, cross = 0;
    const bool any = surf_load(vol, n_vox, min_w, w0);
    if (__ballot(any)) {
        for (int it = 0; it < SURF_ITEMS; it++) {
            if (!surf_seen(w0[it], min_w)) continue;
            const uint32_t idx = blockIdx.x * (uint32_t)OSLAMK_SURF_RUN + (uint32_t)it * SURF_T + threadIdx.x;
            int ijk[3];
            uint32_t nb[3];
            float rec[6];
            const uint32_t mask = surf_crossings(vol, idx, w0[it], min_w, ijk, nb);
            cross += (uint32_t)__popc(mask);
#pragma unroll 1
            for (int a = 0; a < 3; a++)
                if ((mask >> a & 1u) && surf_point(vol, ijk, a, w0[it], surf_pick(nb, a), rec)) pts++;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            pts += __shfl_down(pts, off, 64);
            cross += __shfl_down(cross, off, 64);
        }
    }
    if (lane == 0) {
        s_pts[wave] = pts;
        if (cross) atomicAdd(totals, cross);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < SURF_WAVES; w++) s += s_pts[w];
        counts[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(SURF_T) void k_surface_scan(uint32_t *counts, uint32_t n, uint32_t *totals)
{
    __shared__ uint32_t s_wave[SURF_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t tile = 0; tile < n; tile += SURF_T) {
        const uint32_t i = tile + threadIdx.x;
        const uint32_t v = i < n ? counts[i] : 0u;
        uint32_t x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, 64);
            if (lane >= (uint32_t)off) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < SURF_WAVES; w++) {
            const uint32_t c = s_wave[w];
            if (w < wave) before += c;
            all += c;
        }
        if (i < n) counts[i] = carry + before + (x - v);
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[1] = carry;
}

__global__ __launch_bounds__(SURF_T) void k_surface_emit(const oslamk_volume vol, uint32_t min_w, uint32_t n_vox,
                                                         const uint32_t *offsets, uint32_t n_points, float *out6)
{
    __shared__ uint32_t s_cnt[SURF_ITEMS][SURF_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t w0[SURF_ITEMS];
    const bool any = surf_load(vol, n_vox, min_w, w0);
    if (!__syncthreads_or(any)) return;
    const bool wave_any = __ballot(any) != 0ull;
    uint32_t run = offsets[blockIdx.x];
    for (int it = 0; it < SURF_ITEMS; it++) {
        float rec[3][6] = {};
        uint32_t has = 0;
        if (wave_any && surf_seen(w0[it], min_w)) {
            const uint32_t idx = blockIdx.x * (uint32_t)OSLAMK_SURF_RUN + (uint32_t)it * SURF_T + threadIdx.x;
            int ijk[3];
            uint32_t nb[3];
            const uint32_t mask = surf_crossings(vol, idx, w0[it], min_w, ijk, nb);
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
        const uint64_t bx = __ballot(has & 1u), by = __ballot(has & 2u), bz = __ballot(has & 4u);
        if (lane == 0) s_cnt[it][wave] = (uint32_t)(__popcll(bx) + __popcll(by) + __popcll(bz));
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < SURF_WAVES; w++) {
            const uint32_t c = s_cnt[it][w];
            if (w < wave) before += c;
            all += c;
        }
        uint32_t rank = run + before + (uint32_t)(__popcll(bx & below) + __popcll(by & below) + __popcll(bz & below));
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

static bool surface_ok(const oslamk_volume *vol, uint32_t min_w, uint32_t n_groups, uint32_t *n_vox)
{
    if (!(vol->words && vol->nx >= 16 && vol->ny >= 16 && vol->nz >= 16 && vol->nx <= 512 && vol->ny <= 512 && vol->nz <= 512 &&
          vol->voxel > 0.0f && min_w >= 1u && min_w <= 65535u))
        return false;
    *n_vox = (uint32_t)vol->nx * (uint32_t)vol->ny * (uint32_t)vol->nz;          /* at most 2^27 */
    return n_groups == oslamk_surface_groups(vol);
}

extern "C" uint32_t oslamk_surface_groups(const oslamk_volume *vol)
{
    const uint32_t n_vox = (uint32_t)vol->nx * (uint32_t)vol->ny * (uint32_t)vol->nz;
    return (n_vox + OSLAMK_SURF_RUN - 1u) / OSLAMK_SURF_RUN;
}

extern "C" int oslamk_surface_count(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, uint32_t *counts,
                                    uint32_t *totals, void *stream)
{
    uint32_t n_vox;
    hipError_t e;
    if (!surface_ok(vol, min_weight, n_groups, &n_vox) || !counts || !totals) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_surface_count, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, counts, totals);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_surface_scan, dim3(1), dim3(SURF_T), 0, (hipStream_t)stream, counts, n_groups, totals);
    return (int)hipGetLastError();
}

extern "C" int oslamk_surface_scan(uint32_t *counts, uint32_t n, uint32_t *totals, void *stream)
{
    if (!counts || !totals || n == 0 || n > (1u << 17)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_surface_scan, dim3(1), dim3(SURF_T), 0, (hipStream_t)stream, counts, n, totals);
    return (int)hipGetLastError();
}

extern "C" int oslamk_surface_emit(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, const uint32_t *offsets,
                                   uint32_t n_points, float *out6, void *stream)
{
    uint32_t n_vox;
    if (!surface_ok(vol, min_weight, n_groups, &n_vox) || !offsets || !out6 || n_points == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_surface_emit, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, offsets,
                       n_points, out6);
    return (int)hipGetLastError();
}
