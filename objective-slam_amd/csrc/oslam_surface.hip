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
 *                     leaves the number of points in totals[1].
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
#include "oslam_tsdf_read.h"
#include "ppf_math.h"

#define SURF_T OSLAMK_SURF_THREADS
#define SURF_ITEMS OSLAMK_SURF_ITEMS
#define SURF_WAVES (OSLAMK_SURF_THREADS / 64)

static_assert(OSLAMK_SURF_RUN == SURF_T * SURF_ITEMS && SURF_T % 64 == 0, "a run is whole chunks of whole waves");

__device__ __forceinline__ bool surf_seen(uint32_t word, uint32_t min_w) { return (word >> 16) >= min_w; }
__device__ __forceinline__ bool surf_neg(uint32_t word) { return (int16_t)(word & 0xffffu) < 0; }

/* the crossings of the seen voxel idx (word w0) as a mask of axes; ijk = its coordinates, nb[a] = the neighbour's word
 * where bit a is set */
__device__ __forceinline__ uint32_t surf_crossings(const oslamk_volume &vol, uint32_t idx, uint32_t w0, uint32_t min_w, int ijk[3],
                                                   uint32_t nb[3])
{
    const uint32_t nx = (uint32_t)vol.nx, ny = (uint32_t)vol.ny, row = idx / nx;
    const uint32_t stride[3] = {1u, nx, nx * ny};
    const int n[3] = {vol.nx, vol.ny, vol.nz};
    uint32_t mask = 0;
    ijk[0] = (int)(idx - row * nx);
    ijk[1] = (int)(row % ny);
    ijk[2] = (int)(row / ny);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        nb[a] = 0u;
        if (ijk[a] + 1 < n[a]) {
            nb[a] = vol.words[(size_t)idx + stride[a]];
            if (surf_seen(nb[a], min_w) && surf_neg(w0) != surf_neg(nb[a])) mask |= 1u << a;
        }
    }
    return mask;
}

__device__ __forceinline__ uint32_t surf_pick(const uint32_t nb[3], int a) { return a == 0 ? nb[0] : a == 1 ? nb[1] : nb[2]; }

/* the point of the crossing on axis a of voxel ijk and its normal into rec (x y z nx ny nz); false without a normal */
__device__ __forceinline__ bool surf_point(const oslamk_volume &vol, const int ijk[3], int a, uint32_t w0, uint32_t w1, float rec[6])
{
    const float F0 = tsdf_of(w0), F1 = tsdf_of(w1);
    const float t = F0 / (F0 - F1);
    const float h = vol.voxel;
    float P[3];
#pragma unroll
    for (int b = 0; b < 3; b++) {
        P[b] = vol.origin[b] + ((float)ijk[b] + 0.5f) * h;
        if (b == a) P[b] = P[b] + t * h;
    }
    float x0, x1, y0, y1, z0, z1;
    if (!(tsdf_trilinear(vol, P[0] + h, P[1], P[2], &x1) && tsdf_trilinear(vol, P[0] - h, P[1], P[2], &x0) &&
          tsdf_trilinear(vol, P[0], P[1] + h, P[2], &y1) && tsdf_trilinear(vol, P[0], P[1] - h, P[2], &y0) &&
          tsdf_trilinear(vol, P[0], P[1], P[2] + h, &z1) && tsdf_trilinear(vol, P[0], P[1], P[2] - h, &z0)))
        return false;
    const float gx = x1 - x0, gy = y1 - y0, gz = z1 - z0;
    const float len = pm_sqrtf((gx * gx + gy * gy) + gz * gz);
    if (!(len > 0.0f && len <= 3.0e38f)) return false;
    rec[0] = P[0];
    rec[1] = P[1];
    rec[2] = P[2];
    rec[3] = gx / len;
    rec[4] = gy / len;
    rec[5] = gz / len;
    return true;
}

/* a thread's own words of its workgroup's run (0 = unseen past the end of the volume); true when one of them is seen */
__device__ __forceinline__ bool surf_load(const oslamk_volume &vol, uint32_t n_vox, uint32_t min_w, uint32_t w0[SURF_ITEMS])
{
    const uint32_t base = blockIdx.x * (uint32_t)OSLAMK_SURF_RUN + threadIdx.x;
    bool any = false;
#pragma unroll
    for (int it = 0; it < SURF_ITEMS; it++) {
        const uint32_t idx = base + (uint32_t)it * SURF_T;
        w0[it] = idx < n_vox ? vol.words[idx] : 0u;
        any |= surf_seen(w0[it], min_w);
    }
    return any;
}

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

extern "C" int oslamk_surface_emit(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, const uint32_t *offsets,
                                   uint32_t n_points, float *out6, void *stream)
{
    uint32_t n_vox;
    if (!surface_ok(vol, min_weight, n_groups, &n_vox) || !offsets || !out6 || n_points == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_surface_emit, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, offsets,
                       n_points, out6);
    return (int)hipGetLastError();
}
