/*
 * oslam_vote.hip -- the vote launches of the PPF registration path (gfx950; host side: oslam_vote.c; the overview of
 * the path is at the top of oslam_kernels.h).  The workgroup itself is vote_body of oslam_vote_body.inc, instantiated
 * here with 16-bit counters (PASS 0) for exact and fast mode; the rare re-vote with 32-bit counters is a unit of its own
 * with its own flag (oslam_vote_wide.hip).  Built with -ffp-contract=off.
 *
 *   k_vote        one workgroup per (scene reference point, model slice of 2046 points)
 *   k_vote_group  the same for all the members of a database group in one grid
 *   k_selftest    the device's float path (pm_acosf, pm_atan2f, the key quantisation) and the alpha bins from
 *                 k_alpha_thr, the table of this instantiation of oslam_vote_body.inc, for the host to compare with
 *                 its own
 * Bounds are vote_body's (see there).  The resources are in profiles/r31_kernel_resources_split.txt; the vote kernels
 * need float_denorm_mode_32 = 3, which tools/kernel_resources.sh prints for this unit and for oslam_vote_wide.
 */
#include <hip/hip_runtime.h>

#include "oslam_kernels.h"
#include "ppf_core.h"

#include "oslam_vote_body.inc"

template <int MODE>
__global__ __launch_bounds__(VOTE_THREADS) void k_vote(oslamk_vote_args a)
{
    vote_body<MODE, 0>(a, blockIdx.x);
}
/* The votes of all the members of a database group in ONE grid: member j = blockIdx / workgroups per member, its
 * arguments from an array in device memory (copied to scalar registers as a kernel argument would be).  Every member
 * votes the same batch of reference points; a member with fewer slices than the widest leaves its surplus
 * workgroups at once (vote_body's own test of the reference point).  Fifty models on a depth frame are fifty grids of
 * some 280 workgroups otherwise -- each a little more than one round on 256 CUs, each with its own tail. */
template <int MODE>
__global__ __launch_bounds__(VOTE_THREADS) void k_vote_group(const oslamk_vote_args *all, uint32_t wgs_per_member)
{
    const uint32_t j = blockIdx.x / wgs_per_member;
    const oslamk_vote_args a = all[j];
    vote_body<MODE, 0>(a, blockIdx.x - j * wgs_per_member);
}
/* k_vote_wide (the re-vote of workgroups whose 16-bit counters overflowed) lives in oslam_vote_wide.hip */

/* --------------------------------------------------------------------------
 * device self-test of the float path
 * ------------------------------------------------------------------------*/
__global__ void k_selftest(const float *x, const float *y, const float *x2, size_t n, float *out_acos,
                           float *out_atan2, uint32_t *out_quant, uint32_t *out_bin)
{
    __shared__ uint32_t s_tbl[32];
    if (threadIdx.x < 32) s_tbl[threadIdx.x] = k_alpha_thr[threadIdx.x];
    __syncthreads();
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_acos[i] = pm_acosf(x[i]);
    out_atan2[i] = pm_atan2f(y[i], x2[i]);
    out_quant[i] = pc_quant_bits(pm_fabsf(y[i]) * 7.0f, 0.0371f + pm_fabsf(x[i]) * 0.01f,
                                 1.0f / (0.0371f + pm_fabsf(x[i]) * 0.01f));
    out_bin[i] = pc_alpha_bin_table(y[i], x2[i], x[i], y[i] - x2[i], s_tbl);
}

/* --------------------------------------------------------------------------
 * launchers
 * ------------------------------------------------------------------------*/
extern "C" {

int oslamk_vote(const oslamk_vote_args *a, void *stream)
{
    if (a->n_launch <= 0) return 0;
    /* padded to groups of 8 reference points: see the workgroup -> (reference point, slice) map in k_vote */
    dim3 grid((unsigned)(((size_t)a->n_launch + 7) / 8 * 8 * a->table.n_slices));
    hipLaunchKernelGGL((a->mode == 0 ? k_vote<0> : k_vote<1>), grid, dim3(VOTE_THREADS), 0, (hipStream_t)stream, *a);
    return oslamk_vote_wide(a, stream);             /* the redo list of this launch (oslam_vote_wide.hip) */
}

int oslamk_vote_group(const oslamk_vote_args *d_all, const oslamk_vote_args *h_all, int nm, void *stream)
{
    if (nm <= 0 || h_all[0].n_launch <= 0) return 0;
    int max_slices = 1;
    for (int j = 0; j < nm; j++) {
        if (h_all[j].n_launch != h_all[0].n_launch || h_all[j].mode != h_all[0].mode) return (int)hipErrorInvalidValue;
        if (h_all[j].table.n_slices > max_slices) max_slices = h_all[j].table.n_slices;
    }
    const size_t wgs = ((size_t)h_all[0].n_launch + 7) / 8 * 8 * (size_t)max_slices;
    if (wgs * (size_t)nm > 0x7fffffffu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((h_all[0].mode == 0 ? k_vote_group<0> : k_vote_group<1>), dim3((unsigned)(wgs * (size_t)nm)),
                       dim3(VOTE_THREADS), 0, (hipStream_t)stream, d_all, (uint32_t)wgs);
    return (int)hipGetLastError();      /* the caller runs oslamk_vote_wide for the members whose redo list is not empty */
}

int oslamk_selftest(const float *x, const float *y, const float *x2, size_t n, float *out_acos,
                    float *out_atan2, uint32_t *out_quant, uint32_t *out_bin, void *stream)
{
    hipLaunchKernelGGL(k_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       x, y, x2, n, out_acos, out_atan2, out_quant, out_bin);
    return (int)hipGetLastError();
}

} /* extern "C" */
