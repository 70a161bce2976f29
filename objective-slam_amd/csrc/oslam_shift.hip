/*
 * oslam_shift.hip -- the window of voxels a TSDF volume holds, moved by whole voxels, and the part of the fused surface
 * that such a move loses (semantics: include/oslam.h at oslam_volume_shift; host side: oslam_volume.c and
 * oslam_surface.c; sums over a wave and a workgroup: oslam_block_scan.h; the edges and points: oslam_surf_edge.h).
 *
 *   k_tsdf_shift      copies from the live buffer into a second buffer of the same size (the host swaps the two after
 *                     the launch: a shift in place would read words another workgroup has already overwritten).  A
 *                     thread owns four consecutive destination words of one row and stores them with one 16-byte
 *                     store.  A row whose source row does not exist stores zeros without loading; otherwise the four
 *                     source words are loaded one by one, each with its x range-checked, or with one 16-byte load when
 *                     the x shift is a multiple of 4 (the source quad is then aligned and lies wholly inside its row or
 *                     wholly outside).  The words with w > 0 are counted: a popcount, wave_sum, one integer atomic per
 *                     wave.
 *   k_leave_count     k_surface_count and k_surface_emit again, over the same workgroups and runs, with the mask of a
 *   k_leave_emit      voxel's crossings ANDed with the mask of its edges that have an end outside the window after the
 *                     shift, before anything is counted or ranked.  That mask comes from the voxel's index alone, so a
 *                     workgroup none of whose 1024 voxels has such an edge returns before it loads a word
 *                     (k_leave_count stores its zero count first: the scan reads it).
 * Bounds.  k_tsdf_shift checks the quad's index against the number of quads before anything else, forms the source's
 * linear index only after the three source coordinates passed their integer range checks (a row's end does not read the
 * next row's start), and stores inside the destination by the first check alone.  The shifts are at most 2^20 in size
 * (checked by the launchers), so no coordinate sum leaves int.  The extraction's bounds are oslam_surface.hip's, the
 * rank check before every store included.  The resources are in profiles/r15_kernel_resources_shift.txt.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"
#include "oslam_surf_edge.h"

#define SHIFT_T 256

struct shift3 {
    int s[3];
};

__device__ __forceinline__ bool shift_in(int c, int n) { return (unsigned)c < (unsigned)n; }

__global__ __launch_bounds__(SHIFT_T) void k_tsdf_shift(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int nx, int ny,
                                                        int nz, const shift3 sh, uint32_t n_quads, uint32_t *kept)
{
    const uint32_t q = blockIdx.x * (uint32_t)SHIFT_T + threadIdx.x;
    uint32_t cnt = 0;
    if (q < n_quads) {
        const uint32_t qpr = (uint32_t)nx >> 2, row = q / qpr;
        const int i0 = (int)((q - row * qpr) << 2), j = (int)(row % (uint32_t)ny), k = (int)(row / (uint32_t)ny);
        const int si = i0 + sh.s[0], sj = j + sh.s[1], sk = k + sh.s[2];
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (shift_in(sj, ny) && shift_in(sk, nz)) {
            const size_t base = ((size_t)sk * (size_t)ny + (size_t)sj) * (size_t)nx;
            if ((sh.s[0] & 3) == 0) {
                if (shift_in(si, nx)) w = *reinterpret_cast<const uint4 *>(src + base + (size_t)si);
            } else {
                if (shift_in(si, nx)) w.x = src[base + (size_t)si];
                if (shift_in(si + 1, nx)) w.y = src[base + (size_t)(si + 1)];
                if (shift_in(si + 2, nx)) w.z = src[base + (size_t)(si + 2)];
                if (shift_in(si + 3, nx)) w.w = src[base + (size_t)(si + 3)];
            }
        }
        *reinterpret_cast<uint4 *>(dst + (size_t)q * 4) = w;
        cnt = (uint32_t)((w.x >> 16 != 0u) + (w.y >> 16 != 0u) + (w.z >> 16 != 0u) + (w.w >> 16 != 0u));
    }
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63u) == 0 && cnt) atomicAdd(kept, cnt);
}

/* the edges of voxel idx (< n_vox) that leave under the shift, as a mask of axes: the edge exists and the voxel or the
 * edge's other end lies outside the window afterwards */
__device__ __forceinline__ uint32_t leave_edges(const oslamk_volume &vol, uint32_t idx, const shift3 &sh)
{
    const uint32_t nx = (uint32_t)vol.nx, ny = (uint32_t)vol.ny, row = idx / nx;
    const int n[3] = {vol.nx, vol.ny, vol.nz};
    const int c[3] = {(int)(idx - row * nx), (int)(row % ny), (int)(row / ny)};
    const bool stays = shift_in(c[0] - sh.s[0], n[0]) && shift_in(c[1] - sh.s[1], n[1]) && shift_in(c[2] - sh.s[2], n[2]);
    uint32_t mask = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        if (c[a] + 1 < n[a] && !(stays && shift_in(c[a] + 1 - sh.s[a], n[a]))) mask |= 1u << a;
    return mask;
}

/* the leaving edges of a thread's voxels, three bits per chunk of its workgroup's run */
__device__ __forceinline__ uint32_t leave_load(const oslamk_volume &vol, uint32_t n_vox, const shift3 &sh)
{
    uint32_t lv = 0;
#pragma unroll
    for (int it = 0; it < SURF_ITEMS; it++) {
        const uint32_t idx = surf_idx(it);
        if (idx < n_vox) lv |= leave_edges(vol, idx, sh) << (3 * it);
    }
    return lv;
}

__global__ __launch_bounds__(SURF_T) void k_leave_count(const oslamk_volume vol, const shift3 sh, uint32_t min_w, uint32_t n_vox,
                                                        uint32_t *counts, uint32_t *totals)
{
    __shared__ uint32_t s_pts[SURF_WAVES];
    const uint32_t lv = leave_load(vol, n_vox, sh);
    if (!__syncthreads_or(lv != 0u)) {
        if (threadIdx.x == 0) counts[blockIdx.x] = 0u;
        return;
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

__global__ __launch_bounds__(SURF_T) void k_leave_emit(const oslamk_volume vol, const shift3 sh, uint32_t min_w, uint32_t n_vox,
                                                       const uint32_t *offsets, uint32_t n_points, float *out6)
{
    __shared__ uint32_t s_cnt[SURF_ITEMS][SURF_WAVES];
    const uint32_t lv = leave_load(vol, n_vox, sh);
    if (!__syncthreads_or(lv != 0u)) return;
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
            /* one axis at a time, the record to its row by selects, as in k_surface_emit */
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

static bool shift_ok(const int shift[3], shift3 *sh)
{
    if (!shift) return false;
    for (int a = 0; a < 3; a++) {
        if (shift[a] < -OSLAMK_SHIFT_MAX || shift[a] > OSLAMK_SHIFT_MAX) return false;
        sh->s[a] = shift[a];
    }
    return true;
}

extern "C" int oslamk_tsdf_shift(const oslamk_volume *vol, uint32_t *dst, const int shift[3], uint32_t *kept, void *stream)
{
    shift3 sh;
    if (!(vol && vol->words && dst && dst != vol->words && kept && shift_ok(shift, &sh) && vol->nx >= 16 && vol->ny >= 16 &&
          vol->nz >= 16 && vol->nx <= 512 && vol->ny <= 512 && vol->nz <= 512 && vol->nx % 8 == 0))
        return (int)hipErrorInvalidValue;
    const uint32_t n_quads = (uint32_t)(vol->nx / 4) * (uint32_t)vol->ny * (uint32_t)vol->nz;       /* at most 2^25 */
    hipLaunchKernelGGL(k_tsdf_shift, dim3((n_quads + SHIFT_T - 1u) / SHIFT_T), dim3(SHIFT_T), 0, (hipStream_t)stream, vol->words, dst,
                       vol->nx, vol->ny, vol->nz, sh, n_quads, kept);
    return (int)hipGetLastError();
}

extern "C" int oslamk_leave_count(const oslamk_volume *vol, const int shift[3], uint32_t min_weight, uint32_t n_groups,
                                  uint32_t *counts, uint32_t *totals, void *stream)
{
    uint32_t n_vox;
    shift3 sh;
    if (!surf_launch_ok(vol, min_weight, n_groups, &n_vox) || !shift_ok(shift, &sh) || !counts || !totals) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_leave_count, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, sh, min_weight, n_vox, counts, totals);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : oslamk_surface_scan(counts, n_groups, totals + 1, stream);
}

extern "C" int oslamk_leave_emit(const oslamk_volume *vol, const int shift[3], uint32_t min_weight, uint32_t n_groups,
                                 const uint32_t *offsets, uint32_t n_points, float *out6, void *stream)
{
    uint32_t n_vox;
    shift3 sh;
    if (!surf_launch_ok(vol, min_weight, n_groups, &n_vox) || !shift_ok(shift, &sh) || !offsets || !out6 || n_points == 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_leave_emit, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, sh, min_weight, n_vox, offsets,
                       n_points, out6);
    return (int)hipGetLastError();
}
