/*
 * oslam_reload.hip -- the voxels that a shift of a TSDF volume's window moves out, packed into records for the voxel
 * store, and the records the store gives back, scattered into the moved window (semantics: include/oslam.h at
 * oslam_volume_shift_world; host side: oslam_volume.c and oslam_world.c; sums and scans: oslam_block_scan.h).  No float
 * operation anywhere: words are copied, never read as numbers beyond "weight != 0".
 *
 *   k_tsdf_pack_count   a workgroup of 256 threads owns OSLAMK_PACK_RUN consecutive linear voxel indices of the old
 *                       window, as OSLAMK_PACK_ITEMS chunks of 256 (the runs of the surface extraction).  Whether a voxel
 *                       leaves comes from its index alone; a workgroup none of whose voxels leaves stores its zero count
 *                       (the scan reads it) and returns before it loads a word.  Otherwise a thread loads the words of
 *                       its leaving voxels only, and the number of seen ones goes to counts[blockIdx.x] (block_sum).
 *   (scan)              oslamk_surface_scan of oslam_surface.hip turns counts[] into offsets and leaves the total.
 *   k_tsdf_pack_emit    recomputes.  The rank of a record is its rank in the chunk (block_excl_scan), plus the records of
 *                       the earlier chunks, plus the workgroup's offset: ascending linear index.  A record {lin, word}
 *                       goes out with one 8-byte store.
 *   k_tsdf_unpack       one thread per record {lin in the new window, word}: one 4-byte store.  The host gives distinct
 *                       lin, and launches it in stream order behind k_tsdf_shift into the buffer that shift wrote.
 * Bounds.  An index is checked against nx*ny*nz before it is split into coordinates and before its word is loaded (the
 * last run is ragged); a record's rank is checked against the counted total before the store; k_tsdf_unpack checks the
 * record's number against the number of records before the load and its lin against nx*ny*nz before the store.  The
 * launchers check the sides, the shift (at most 2^20 in size, so no coordinate difference leaves int), the number of
 * workgroups and that there are no more records than voxels.  No scratch; the resources are in
 * profiles/r17_kernel_resources_reload.txt.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "oslam_block_scan.h"
#include "oslam_kernels.h"

#define PACK_T OSLAMK_PACK_THREADS
#define PACK_ITEMS OSLAMK_PACK_ITEMS
#define PACK_WAVES (OSLAMK_PACK_THREADS / 64)

static_assert(OSLAMK_PACK_RUN == PACK_T * PACK_ITEMS && PACK_T % 64 == 0, "a run is whole chunks of whole waves");

struct pack_dims {
    int nx, ny, nz;
};

__device__ __forceinline__ bool pack_in(int c, int n) { return (unsigned)c < (unsigned)n; }

__device__ __forceinline__ uint32_t pack_idx(int it) { return blockIdx.x * (uint32_t)OSLAMK_PACK_RUN + (uint32_t)it * PACK_T + threadIdx.x; }

/* bit it: the thread's voxel of chunk it exists and lies outside the window after the shift */
__device__ __forceinline__ uint32_t pack_leaving(const pack_dims &d, uint32_t n_vox, const oslamk_shift3 &sh)
{
    uint32_t lv = 0;
#pragma unroll
    for (int it = 0; it < PACK_ITEMS; it++) {
        const uint32_t idx = pack_idx(it);
        if (idx < n_vox) {
            const uint32_t row = idx / (uint32_t)d.nx;
            const int i = (int)(idx - row * (uint32_t)d.nx), j = (int)(row % (uint32_t)d.ny), k = (int)(row / (uint32_t)d.ny);
            const bool stays = pack_in(i - sh.s[0], d.nx) && pack_in(j - sh.s[1], d.ny) && pack_in(k - sh.s[2], d.nz);
            lv |= (stays ? 0u : 1u) << it;
        }
    }
    return lv;
}

__global__ __launch_bounds__(PACK_T) void k_tsdf_pack_count(const uint32_t *__restrict__ words, const pack_dims d, const oslamk_shift3 sh,
                                                            uint32_t n_vox, uint32_t *counts)
{
    __shared__ uint32_t s_sum[PACK_WAVES];
    const uint32_t lv = pack_leaving(d, n_vox, sh);
    if (!__syncthreads_or(lv != 0u)) {
        if (threadIdx.x == 0) counts[blockIdx.x] = 0u;
        return;
    }
    uint32_t cnt = 0;
#pragma unroll
    for (int it = 0; it < PACK_ITEMS; it++)
        if (lv >> it & 1u) cnt += (words[pack_idx(it)] >> 16) != 0u;      /* the bit is set only below n_vox */
    cnt = block_sum<PACK_WAVES>(cnt, s_sum);
    if (threadIdx.x == 0) counts[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(PACK_T) void k_tsdf_pack_emit(const uint32_t *__restrict__ words, const pack_dims d, const oslamk_shift3 sh,
                                                           uint32_t n_vox, const uint32_t *__restrict__ offsets, uint32_t n_rec,
                                                           uint2 *__restrict__ out)
{
    __shared__ uint32_t s_cnt[PACK_ITEMS][PACK_WAVES];
    const uint32_t lv = pack_leaving(d, n_vox, sh);
    if (!__syncthreads_or(lv != 0u)) return;
    uint32_t w[PACK_ITEMS];
#pragma unroll
    for (int it = 0; it < PACK_ITEMS; it++) w[it] = (lv >> it & 1u) ? words[pack_idx(it)] : 0u;
    uint32_t run = offsets[blockIdx.x];
#pragma unroll
    for (int it = 0; it < PACK_ITEMS; it++) {
        const uint32_t has = (w[it] >> 16) != 0u ? 1u : 0u;
        uint32_t all;
        const uint32_t rank = run + block_excl_scan<PACK_WAVES>(has, s_cnt[it], &all);
        if (has && rank < n_rec) out[rank] = make_uint2(pack_idx(it), w[it]);
        run += all;
    }
}

__global__ __launch_bounds__(PACK_T) void k_tsdf_unpack(uint32_t *__restrict__ dst, uint32_t n_vox, const uint2 *__restrict__ recs,
                                                        uint32_t n_rec)
{
    const uint32_t r = blockIdx.x * (uint32_t)PACK_T + threadIdx.x;
    if (r >= n_rec) return;
    const uint2 rec = recs[r];
    if (rec.x < n_vox) dst[rec.x] = rec.y;
}

static bool pack_launch_ok(const oslamk_volume *vol, const int shift[3], uint32_t n_groups, uint32_t *n_vox)
{
    if (!(vol && vol->words && shift && oslamk_shift_ok(shift) && oslamk_sides_ok(vol->nx, vol->ny, vol->nz, 1))) return false;
    *n_vox = (uint32_t)vol->nx * (uint32_t)vol->ny * (uint32_t)vol->nz;          /* at most 2^27 */
    return n_groups == oslamk_pack_groups(vol);
}

extern "C" uint32_t oslamk_pack_groups(const oslamk_volume *vol)
{
    const uint32_t n_vox = (uint32_t)vol->nx * (uint32_t)vol->ny * (uint32_t)vol->nz;
    return (n_vox + OSLAMK_PACK_RUN - 1u) / OSLAMK_PACK_RUN;
}

extern "C" int oslamk_tsdf_pack_count(const oslamk_volume *vol, const int shift[3], uint32_t n_groups, uint32_t *counts,
                                      uint32_t *total_out, void *stream)
{
    uint32_t n_vox;
    if (!pack_launch_ok(vol, shift, n_groups, &n_vox) || !counts || !total_out) return (int)hipErrorInvalidValue;
    const pack_dims d = {vol->nx, vol->ny, vol->nz};
    const oslamk_shift3 sh = {{shift[0], shift[1], shift[2]}};
    hipLaunchKernelGGL(k_tsdf_pack_count, dim3(n_groups), dim3(PACK_T), 0, (hipStream_t)stream, vol->words, d, sh, n_vox, counts);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : oslamk_surface_scan(counts, n_groups, total_out, stream);
}

extern "C" int oslamk_tsdf_pack_emit(const oslamk_volume *vol, const int shift[3], uint32_t n_groups, const uint32_t *offsets,
                                     uint32_t n_rec, uint32_t *rec_out, void *stream)
{
    uint32_t n_vox;
    if (!pack_launch_ok(vol, shift, n_groups, &n_vox) || !offsets || !rec_out || n_rec == 0 || n_rec > n_vox ||
        ((uintptr_t)rec_out & 7u))
        return (int)hipErrorInvalidValue;
    const pack_dims d = {vol->nx, vol->ny, vol->nz};
    const oslamk_shift3 sh = {{shift[0], shift[1], shift[2]}};
    hipLaunchKernelGGL(k_tsdf_pack_emit, dim3(n_groups), dim3(PACK_T), 0, (hipStream_t)stream, vol->words, d, sh, n_vox, offsets, n_rec,
                       reinterpret_cast<uint2 *>(rec_out));
    return (int)hipGetLastError();
}

extern "C" int oslamk_tsdf_unpack(uint32_t *dst, int nx, int ny, int nz, const uint32_t *recs, uint32_t n_rec, void *stream)
{
    if (!dst || !recs || !oslamk_sides_ok(nx, ny, nz, 1) || ((uintptr_t)recs & 7u)) return (int)hipErrorInvalidValue;
    const uint32_t n_vox = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;
    if (n_rec == 0 || n_rec > n_vox) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tsdf_unpack, dim3((n_rec + PACK_T - 1u) / PACK_T), dim3(PACK_T), 0, (hipStream_t)stream, dst, n_vox,
                       reinterpret_cast<const uint2 *>(recs), n_rec);
    return (int)hipGetLastError();
}
