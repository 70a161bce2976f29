/*
 * oslam_shift.hip -- the window of voxels a TSDF volume holds, moved by whole voxels (semantics: include/oslam.h at
 * oslam_volume_shift; host side: oslam_volume.c; sums over a wave: oslam_block_scan.h).  The part of the fused surface
 * that such a move loses is extracted by k_leave_count and k_leave_emit of oslam_surface.hip.
 *
 *   k_tsdf_shift      copies from the live buffer into a second buffer of the same size (the host swaps the two after
 *                     the launch: a shift in place would read words another workgroup has already overwritten).  A
 *                     thread owns four consecutive destination words of one row and stores them with one 16-byte
 *                     store.  A row whose source row does not exist stores zeros without loading; otherwise the four
 *                     source words are loaded one by one, each with its x range-checked, or with one 16-byte load when
 *                     the x shift is a multiple of 4 (the source quad is then aligned and lies wholly inside its row or
 *                     wholly outside).  The words with w > 0 are counted: a popcount, wave_sum, one integer atomic per
 *                     wave.
 * Bounds.  k_tsdf_shift checks the quad's index against the number of quads before anything else, forms the source's
 * linear index only after the three source coordinates passed their integer range checks (a row's end does not read the
 * next row's start), and stores inside the destination by the first check alone.  The shifts are at most 2^20 in size
 * (checked by the launcher), so no coordinate sum leaves int.  The resources are in
 * profiles/r16_kernel_resources_surface_merged.txt.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_block_scan.h"
#include "oslam_kernels.h"

#define SHIFT_T 256

__device__ __forceinline__ bool shift_in(int c, int n) { return (unsigned)c < (unsigned)n; }

__global__ __launch_bounds__(SHIFT_T) void k_tsdf_shift(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int nx, int ny,
                                                        int nz, const oslamk_shift3 sh, uint32_t n_quads, uint32_t *kept)
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

extern "C" int oslamk_tsdf_shift(const oslamk_volume *vol, uint32_t *dst, const int shift[3], uint32_t *kept, void *stream)
{
    if (!(vol && vol->words && dst && dst != vol->words && kept && shift && oslamk_shift_ok(shift) &&
          oslamk_sides_ok(vol->nx, vol->ny, vol->nz, 1)))
        return (int)hipErrorInvalidValue;
    const oslamk_shift3 sh = {{shift[0], shift[1], shift[2]}};
    const uint32_t n_quads = (uint32_t)(vol->nx / 4) * (uint32_t)vol->ny * (uint32_t)vol->nz;       /* at most 2^25 */
    hipLaunchKernelGGL(k_tsdf_shift, dim3((n_quads + SHIFT_T - 1u) / SHIFT_T), dim3(SHIFT_T), 0, (hipStream_t)stream, vol->words, dst,
                       vol->nx, vol->ny, vol->nz, sh, n_quads, kept);
    return (int)hipGetLastError();
}
