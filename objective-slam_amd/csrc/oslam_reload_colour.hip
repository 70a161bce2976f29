/*
 * oslam_reload_colour.hip -- the colour words that travel with the records of oslam_reload.hip through a colour store
 * (semantics: include/oslam.h at oslam_volume_shift_world, "Colour"; host side: oslam_volume.c and oslam_world.c).  Its
 * own translation unit: the kernels of oslam_reload.hip are as they were.  No float operation: words are copied.
 *
 *   k_pack_colours      one thread per record {lin, word} that k_tsdf_pack_emit made: colours_out[r] = colours[lin].  A
 *                       gather behind the emit, in stream order; no second scan of the volume.
 *   k_unpack_colours    one thread per record {lin in the new window, word}: dst[lin] = colours_in[r].  The host gives
 *                       distinct lin and launches it behind the k_tsdf_shift that wrote the colour spare buffer dst.
 * Bounds.  A record's number is checked against the number of records before anything is loaded; its lin is checked
 * against nx*ny*nz before the colour is loaded (pack; a record beyond gets 0) or stored (unpack; skipped).  The launchers
 * check the sides, the alignment of the records and that there are no more records than voxels.  No LDS, no scratch.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "oslam_kernels.h"

#define PACK_T OSLAMK_PACK_THREADS

__global__ __launch_bounds__(PACK_T) void k_pack_colours(const uint32_t *__restrict__ colours, uint32_t n_vox,
                                                         const uint2 *__restrict__ recs, uint32_t n_rec,
                                                         uint32_t *__restrict__ colours_out)
{
    const uint32_t r = blockIdx.x * (uint32_t)PACK_T + threadIdx.x;
    if (r >= n_rec) return;
    const uint32_t lin = recs[r].x;
    colours_out[r] = lin < n_vox ? colours[lin] : 0u;
}

__global__ __launch_bounds__(PACK_T) void k_unpack_colours(uint32_t *__restrict__ dst, uint32_t n_vox, const uint2 *__restrict__ recs,
                                                           const uint32_t *__restrict__ colours_in, uint32_t n_rec)
{
    const uint32_t r = blockIdx.x * (uint32_t)PACK_T + threadIdx.x;
    if (r >= n_rec) return;
    const uint32_t lin = recs[r].x;
    if (lin < n_vox) dst[lin] = colours_in[r];
}

static bool colour_records_ok(const uint32_t *buf, int nx, int ny, int nz, const uint32_t *recs, const uint32_t *cols, uint32_t n_rec,
                              uint32_t *n_vox)
{
    if (!buf || !recs || !cols || !oslamk_sides_ok(nx, ny, nz, 1) || ((uintptr_t)recs & 7u)) return false;
    *n_vox = (uint32_t)nx * (uint32_t)ny * (uint32_t)nz;                          /* at most 2^27 */
    return n_rec != 0 && n_rec <= *n_vox;
}

extern "C" int oslamk_pack_colours(const uint32_t *colours, int nx, int ny, int nz, const uint32_t *recs, uint32_t n_rec,
                                   uint32_t *colours_out, void *stream)
{
    uint32_t n_vox;
    if (!colour_records_ok(colours, nx, ny, nz, recs, colours_out, n_rec, &n_vox)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pack_colours, dim3((n_rec + PACK_T - 1u) / PACK_T), dim3(PACK_T), 0, (hipStream_t)stream, colours, n_vox,
                       reinterpret_cast<const uint2 *>(recs), n_rec, colours_out);
    return (int)hipGetLastError();
}

extern "C" int oslamk_unpack_colours(uint32_t *dst, int nx, int ny, int nz, const uint32_t *recs, const uint32_t *colours_in,
                                     uint32_t n_rec, void *stream)
{
    uint32_t n_vox;
    if (!colour_records_ok(dst, nx, ny, nz, recs, colours_in, n_rec, &n_vox)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_unpack_colours, dim3((n_rec + PACK_T - 1u) / PACK_T), dim3(PACK_T), 0, (hipStream_t)stream, dst, n_vox,
                       reinterpret_cast<const uint2 *>(recs), colours_in, n_rec);
    return (int)hipGetLastError();
}
