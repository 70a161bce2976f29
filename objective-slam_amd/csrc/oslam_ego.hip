/*
 * oslam_ego.hip -- the camera motion stage's kernels (semantics: include/oslam.h at oslam_view_egomotion; host side:
 * oslam_ego.c).
 *
 *   k_ego_step   one launch per scheduled iteration, lv.n_slots workgroups of 256 threads.  A workgroup walks lv.chunk
 *                consecutive blocks of 256 selected source pixels: per thread one 32-byte record of the source map, the
 *                transform under the float32 pose, the projection with the destination's camera, one 32-byte gather
 *                from the destination map and the gates (oslam_icp_core.h), the 29 terms of the step
 *                (oslam_refine_step.h); the block's sums in the fixed order of oslam_icp_block_sums (two LDS buffers
 *                taken in turn, one barrier per block; its extra column [29]: the selected source pixels that have a
 *                normal, counted by ballots), added in double in block order by the threads 0..29.  The
 *                workgroup's 30 doubles go to its slot of the partials buffer.  Then the hand-off: every wave drains
 *                its stores, a barrier, thread 0 releases at agent scope and draws a ticket from the launch's arrival
 *                counter; the workgroup that draws the last ticket acquires at agent scope, adds the slots in the
 *                pinned order (8 strands in LDS), and its thread 0 solves (oslam_refine_step) and writes the state for
 *                the next launch.  Nobody waits for anybody: a workgroup that is not the last one leaves.  A launch
 *                whose level is over or whose call is done returns at its first instruction.  No float atomics.
 *   k_ego_corr   the tap: one thread per source pixel, the destination pixel of its correspondence.
 * Bounds: a lattice index is checked against the level's count before any load and maps to a pixel inside the source
 * image (lw = ceil(w / stride) columns, ceil(h / stride) rows); the destination pixel is range-checked in float before
 * it becomes an int, so the gather reads inside the w * h records of the destination map; a workgroup writes the slot
 * of its own index (n_slots <= OSLAMK_EGO_MAX_SLOTS, the size of the buffer) and the last one reads n_slots slots.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_icp_core.h"
#include "oslam_kernels.h"
#include "oslam_refine_step.h"

/* The correspondence of the source pixel spix under the float32 pose T (rows of [R | t]): its pixel index in dst, or -1.
 * *has = the source pixel has a normal; q = p'; with a pixel, a and b = its vertex and normal records. */
__device__ __forceinline__ int ego_correspond(const float4 *smaps, size_t spix, const float *T, const oslamk_view &dv,
                                              const float4 *dmaps, float r2, float min_dot, bool *has, float q[3],
                                              float4 *a_out, float4 *b_out)
{
    const float4 p = smaps[2 * spix], n = smaps[2 * spix + 1];
    *has = p.w != 0.0f;
    if (!*has) return -1;
    float m[3];
    int u, vv;
    oslam_icp_transform(T, p.x, p.y, p.z, n.x, n.y, n.z, q, m);
    if (!oslam_icp_project(dv, q, &u, &vv)) return -1;
    const int pix = vv * dv.w + u;
    return oslam_icp_gate(dmaps, pix, q, m, r2, min_dot, a_out, b_out) ? pix : -1;
}

/* One workgroup: the slots in the pinned order, the step, the state of the next launch. */
__device__ __forceinline__ void ego_finish(const oslamk_ego_level &lv, oslamk_ego_state *st, const double *slots)
{
    __shared__ double sS[OSLAMK_EGO_STRANDS][OSLAMK_EGO_SLOT];
    __shared__ double S[OSLAMK_EGO_SLOT];
    const int tid = threadIdx.x, strand = tid / OSLAMK_EGO_SLOT, k = tid % OSLAMK_EGO_SLOT;
    double acc = 0.0;
    if (k <= OSLAMK_REFINE_SUMS)
        for (uint32_t g = (uint32_t)strand; g < lv.n_slots; g += OSLAMK_EGO_STRANDS) acc += slots[(size_t)g * OSLAMK_EGO_SLOT + k];
    sS[strand][k] = acc;
    __syncthreads();
    if (tid < OSLAMK_EGO_SLOT) {
        double x = sS[0][tid];
#pragma unroll
        for (int j = 1; j < OSLAMK_EGO_STRANDS; j++) x += sS[j][tid];
        S[tid] = x;
    }
    __syncthreads();
    if (tid != 0) return;
    double T[12], th, vn;
    const double cm[3] = {0.0, 0.0, 0.0};
    float Tf[12], cf[3];
    const int L = lv.level;
    for (int a = 0; a < 12; a++) T[a] = st->T[a];
    st->last_corr = (uint32_t)S[27];
    st->rmse = S[27] > 0.0 ? sqrtf((float)(S[28] / S[27])) : 0.0f;
    st->corr[L] = (uint32_t)S[27];
    st->n_src[L] = (uint32_t)S[OSLAMK_REFINE_SUMS];
    if (!oslam_refine_step(S, T, cm, Tf, cf, &th, &vn)) {
        st->converged = 0;
        st->done = 1;
        return;
    }
    const int32_t iter = st->iter + 1;
    const int conv = th < (double)st->stop_rot && vn < (double)st->stop_trans;
    const bool over = conv || (uint32_t)iter >= lv.max_iter;
    for (int a = 0; a < 12; a++) {
        st->T[a] = over ? (double)Tf[a] : T[a];    /* the next level starts from the float32 pose this one leaves */
        st->Tf[a] = Tf[a];
    }
    for (int a = 0; a < 3; a++) st->c[a] = cf[a];
    st->iterations[L] = (uint32_t)iter;
    if (over) {
        st->converged = conv;
        st->level = lv.next_level;
        st->iter = 0;
        if (lv.next_level >= st->n_levels) st->done = 1;
    } else {
        st->iter = iter;
    }
}

__global__ __launch_bounds__(OSLAMK_EGO_THREADS) void k_ego_step(const oslamk_view sv, const float *smaps_,
                                                                 const oslamk_view dv, const float *dmaps_,
                                                                 const oslamk_ego_level lv, oslamk_ego_state *st,
                                                                 double *slots, uint32_t *arrive)
{
    constexpr int NS = OSLAMK_REFINE_SUMS, NW = OSLAMK_EGO_THREADS / 64;
    if (st->done || st->level != lv.level) return;
    __shared__ float sh[2][NW][NS + 1];
    __shared__ float sT[12], sc[3];
    __shared__ int s_last;
    const float4 *smaps = reinterpret_cast<const float4 *>(smaps_), *dmaps = reinterpret_cast<const float4 *>(dmaps_);
    const int tid = threadIdx.x;
    if (tid < 12) sT[tid] = st->Tf[tid];
    if (tid < 3) sc[tid] = st->c[tid];
    const float r2 = st->r2_corr, min_dot = st->min_dot;
    __syncthreads();
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = sT[k];

    double acc = 0.0;
    const uint32_t b0 = blockIdx.x * lv.chunk;
    for (uint32_t j = 0; j < lv.chunk && b0 + j < lv.n_blocks; j++) {
        float s[NS + 1];
#pragma unroll
        for (int k = 0; k < NS; k++) s[k] = 0.0f;
        const uint32_t i = (b0 + j) * OSLAMK_EGO_THREADS + (uint32_t)tid;
        bool has = false;
        if (i < lv.n) {
            const int lu = (int)(i % (uint32_t)lv.lw), lr = (int)(i / (uint32_t)lv.lw);
            const size_t spix = (size_t)(lr * lv.stride) * sv.w + (size_t)(lu * lv.stride);
            float q[3];
            float4 pa, pb;
            if (ego_correspond(smaps, spix, T, dv, dmaps, r2, min_dot, &has, q, &pa, &pb) >= 0)
                oslam_refine_point_sums(q[0], q[1], q[2], pa, pb, sc, s);
        }
        s[NS] = (float)__popcll(__ballot(has));    /* the extra column: the wave's count, not summed by the tree */
        const float x = oslam_icp_block_sums<NS>(s, sh[j & 1u]);
        if (tid <= NS) acc += (double)x;
    }
    if (tid <= NS) slots[(size_t)blockIdx.x * OSLAMK_EGO_SLOT + tid] = acc;
    /* the hand-off: drain, barrier, release, ticket; the last arriver acquires before anyone of it reads a slot */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t ticket = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == lv.n_slots - 1u;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!s_last) return;
    ego_finish(lv, st, slots);
}

struct ego_pose {
    float T[12];
};

__global__ __launch_bounds__(OSLAMK_EGO_THREADS) void k_ego_corr(const oslamk_view sv, const float *smaps,
                                                                 const oslamk_view dv, const float *dmaps,
                                                                 const ego_pose P, float r2, float min_dot,
                                                                 int32_t *pixel_out)
{
    const size_t i = (size_t)blockIdx.x * OSLAMK_EGO_THREADS + threadIdx.x;
    if (i >= (size_t)sv.w * (size_t)sv.h) return;
    bool has;
    float q[3];
    float4 a, b;
    pixel_out[i] = ego_correspond(reinterpret_cast<const float4 *>(smaps), i, P.T, dv,
                                  reinterpret_cast<const float4 *>(dmaps), r2, min_dot, &has, q, &a, &b);
}

extern "C" int oslamk_ego_step(const oslamk_view *src, const float *src_maps, const oslamk_view *dst, const float *dst_maps,
                               const oslamk_ego_level *lv, oslamk_ego_state *st, double *slots, uint32_t *arrive,
                               void *stream)
{
    if (!src_maps || !dst_maps || !st || !slots || !arrive || lv->stride < 1 || lv->n == 0 || lv->chunk == 0 ||
        lv->lw != (src->w + lv->stride - 1) / lv->stride ||
        lv->n != (uint32_t)lv->lw * (uint32_t)((src->h + lv->stride - 1) / lv->stride) ||
        lv->n_blocks != (lv->n + OSLAMK_EGO_THREADS - 1) / OSLAMK_EGO_THREADS ||
        lv->n_slots != (lv->n_blocks + lv->chunk - 1) / lv->chunk || lv->n_slots > OSLAMK_EGO_MAX_SLOTS || lv->level < 0 ||
        lv->level >= OSLAMK_EGO_MAX_LEVELS)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ego_step, dim3(lv->n_slots), dim3(OSLAMK_EGO_THREADS), 0, (hipStream_t)stream, *src, src_maps, *dst,
                       dst_maps, *lv, st, slots, arrive);
    return (int)hipGetLastError();
}

extern "C" int oslamk_ego_corr(const oslamk_view *src, const float *src_maps, const oslamk_view *dst, const float *dst_maps,
                               const float *T12, float r2_corr, float min_dot, int32_t *pixel_out, void *stream)
{
    const size_t n = (size_t)src->w * (size_t)src->h;
    ego_pose P;
    if (!src_maps || !dst_maps || !pixel_out || n == 0) return (int)hipErrorInvalidValue;
    for (int k = 0; k < 12; k++) P.T[k] = T12[k];
    hipLaunchKernelGGL(k_ego_corr, dim3((unsigned)((n + OSLAMK_EGO_THREADS - 1) / OSLAMK_EGO_THREADS)),
                       dim3(OSLAMK_EGO_THREADS), 0, (hipStream_t)stream, *src, src_maps, *dst, dst_maps, P, r2_corr, min_dot,
                       pixel_out);
    return (int)hipGetLastError();
}
