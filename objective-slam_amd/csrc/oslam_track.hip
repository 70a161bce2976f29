/*
 * oslam_track.hip -- the tracking stage's kernels (semantics: include/oslam.h at oslam_track; host side:
 * oslam_track.c).
 *
 *   k_view_normals   one thread per pixel of the view's z image: the point and the normal of oslam_depth_to_cloud
 *                    (oslam_depth_normal.h, the code of k_depth_points) into a 32-byte record per pixel, x y z has |
 *                    nx ny nz 0, so that a correspondence is one 32-byte gather.
 *   k_track          one workgroup of 256 threads per hypothesis runs the whole call.  Per iteration it walks its
 *                    model's blocks of 256 points: the transform, k_verify's BACK test, the pixel, the gather and the
 *                    gates (oslam_icp_core.h; the z image is not read), the 29 terms of the step (oslam_refine_step.h);
 *                    the block's sums in the fixed order of oslam_icp_block_sums (two LDS buffers taken in turn, so one
 *                    barrier per block), added in double in block order by the threads 0..28.  Thread 0 solves the 6x6
 *                    system in double (oslam_refine_step, the code of k_refine_solve) and publishes the float32 pose and
 *                    the transformed centroid through LDS; a barrier, then the next iteration.  No float atomics: the
 *                    result is bitwise reproducible.  After the last iteration the blocks are classed with the caller's
 *                    window (oslam_verify_class, k_verify's class), counted per wave by ballots and summed as integers.
 *   k_track_corr     the tap: one thread per model point, the pixel of its correspondence.
 * Bounds: a model point index is checked against the model's point count before its loads; the pixel is range-checked
 * in float before it becomes an int (oslam_icp_project), so the gather reads inside the w * h records of the map.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_depth_normal.h"
#include "oslam_icp_core.h"
#include "oslam_kernels.h"
#include "oslam_refine_step.h"
#include "oslam_verify_class.h"

__global__ __launch_bounds__(256) void k_view_normals(const oslamk_view v, float max_jump, float *maps)
{
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), vv = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (u >= v.w || vv >= v.h) return;
    const size_t i = (size_t)vv * v.w + u;
    const depth_cam c = {v.fx, v.fy, v.cx, v.cy, 1.0f, v.z_min, v.z_max, max_jump};
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    const float z = v.z[i];                        /* 0 = not valid; a valid z lies in [z_min, z_max] */
    if (depth_ok(z, c) && u > 0 && vv > 0 && u + 1 < v.w && vv + 1 < v.h) {
        const float zl = v.z[i - 1], zr = v.z[i + 1], zu = v.z[i - v.w], zd = v.z[i + v.w];
        float p[3], n[3];
        if (depth_ok(zl, c) && depth_ok(zr, c) && depth_ok(zu, c) && depth_ok(zd, c) &&
            depth_point_normal(u, vv, z, zl, zr, zu, zd, c, p, n)) {
            a = make_float4(p[0], p[1], p[2], 1.0f);
            b = make_float4(n[0], n[1], n[2], 0.0f);
        }
    }
    float4 *dst = reinterpret_cast<float4 *>(maps) + 2 * i;
    dst[0] = a;
    dst[1] = b;
}

/* The correspondence of point i (i < d->m.n) of a hypothesis with pose d->T: its pixel index, or -1.  q = p'; with a
 * pixel, a and b = its vertex and normal records. */
__device__ __forceinline__ int track_correspond(const oslamk_view &v, const float4 *maps, const oslamk_verify_member *d, int i,
                                                float r2, float min_dot, float q[3], float4 *a_out, float4 *b_out)
{
    float m[3];
    int u, vv;
    oslam_icp_transform(d->T, d->m.px[i], d->m.py[i], d->m.pz[i], d->m.nx[i], d->m.ny[i], d->m.nz[i], q, m);
    if ((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2] >= 0.0f) return -1;  /* BACK, k_verify's test */
    if (!oslam_icp_project(v, q, &u, &vv)) return -1;                  /* OUT */
    const int pix = vv * v.w + u;
    return oslam_icp_gate(maps, pix, q, m, r2, min_dot, a_out, b_out) ? pix : -1;
}

__global__ __launch_bounds__(OSLAMK_TRACK_THREADS) void k_track(const oslamk_view v, const float *maps_,
                                                                const oslamk_track_member *mem, int window,
                                                                oslamk_track_rec *rec)
{
    constexpr int NS = OSLAMK_REFINE_SUMS, NW = OSLAMK_TRACK_THREADS / 64;
    __shared__ float sh[2][NW][NS];
    __shared__ double S[NS];
    __shared__ double sT[12], scm[3];
    __shared__ oslamk_verify_member vm;            /* the cloud, the float32 pose in force, the judgement's tolerance */
    __shared__ float sc[3];
    __shared__ int32_t s_done, s_iter, s_conv, s_ncorr;
    __shared__ uint32_t s_cnt[NW][OSLAMK_VERIFY_CLASSES];
    const oslamk_track_member *d = &mem[blockIdx.x];
    if (d->n_blocks == 0) return;                  /* skipped: the whole workgroup leaves */
    const float4 *maps = reinterpret_cast<const float4 *>(maps_);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

    if (tid < 12) {
        sT[tid] = d->T[tid];
        vm.T[tid] = (float)d->T[tid];
    }
    if (tid < 3) {
        scm[tid] = d->cm[tid];
        sc[tid] = d->c[tid];
    }
    if (tid == 0) {
        vm.m = d->m;
        vm.tol = d->tol;
        vm.n_blocks = d->n_blocks;
        s_done = d->max_iter == 0;
        s_iter = 0;
        s_conv = 0;
        s_ncorr = 0;
    }
    __syncthreads();
    const int n = d->m.n;
    const uint32_t nb = d->n_blocks, max_iter = d->max_iter;
    const float r2 = d->r2_corr, min_dot = d->min_dot;
    const double stop_rot = (double)d->stop_rot, stop_trans = (double)d->stop_trans;

    for (uint32_t it = 0; it < max_iter; it++) {
        double acc = 0.0;
        for (uint32_t b = 0; b < nb; b++) {
            float s[NS];
#pragma unroll
            for (int k = 0; k < NS; k++) s[k] = 0.0f;
            const int i = (int)(b * OSLAMK_TRACK_THREADS) + tid;
            if (i < n) {
                float q[3];
                float4 pa, pb;
                if (track_correspond(v, maps, &vm, i, r2, min_dot, q, &pa, &pb) >= 0)
                    oslam_refine_point_sums(q[0], q[1], q[2], pa, pb, sc, s);
            }
            const float x = oslam_icp_block_sums<NS>(s, sh[b & 1u]);
            if (tid < NS) acc += (double)x;
        }
        if (tid < NS) S[tid] = acc;
        __syncthreads();
        if (tid == 0) {
            double th, vn;
            s_ncorr = (int32_t)S[27];
            if (!oslam_refine_step(S, sT, scm, vm.T, sc, &th, &vn)) {
                s_done = 1;
            } else {
                s_iter += 1;
                if (th < stop_rot && vn < stop_trans) {
                    s_conv = 1;
                    s_done = 1;
                } else if ((uint32_t)s_iter >= max_iter) {
                    s_done = 1;
                }
            }
        }
        __syncthreads();
        if (s_done) break;
    }

    /* the judgement at the final pose: k_verify's classes, counted per wave */
    uint32_t cnt[OSLAMK_VERIFY_CLASSES];
#pragma unroll
    for (int c = 0; c < OSLAMK_VERIFY_CLASSES; c++) cnt[c] = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const int i = (int)(b * OSLAMK_TRACK_THREADS) + tid;
        const int cls = i < n ? oslam_verify_class<false>(v, &vm, i, window, NULL, NULL, NULL) : -1;
#pragma unroll
        for (int c = 0; c < OSLAMK_VERIFY_CLASSES; c++) cnt[c] += (uint32_t)__popcll(__ballot(cls == c));
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < OSLAMK_VERIFY_CLASSES; c++) s_cnt[w][c] = cnt[c];
    }
    __syncthreads();
    oslamk_track_rec *r = &rec[blockIdx.x];
    if (tid < OSLAMK_VERIFY_CLASSES) {
        uint32_t x = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ww++) x += s_cnt[ww][tid];
        r->counts[tid] = x;
    }
    if (tid < 12) r->T[tid] = vm.T[tid];
    if (tid == 0) {
        r->n_corr = (uint32_t)s_ncorr;
        r->iterations = (uint32_t)s_iter;
        r->converged = s_conv;
        r->pad = 0;
    }
}

__global__ __launch_bounds__(OSLAMK_TRACK_THREADS) void k_track_corr(const oslamk_view v, const float *maps,
                                                                     const oslamk_track_member *mem, int32_t *pixel_out)
{
    __shared__ oslamk_verify_member vm;
    const oslamk_track_member *d = &mem[0];
    if (threadIdx.x < 12) vm.T[threadIdx.x] = (float)d->T[threadIdx.x];
    if (threadIdx.x == 0) {
        vm.m = d->m;
        vm.tol = d->tol;
        vm.n_blocks = d->n_blocks;
    }
    __syncthreads();
    const int i = (int)(blockIdx.x * OSLAMK_TRACK_THREADS + threadIdx.x);
    if (i >= d->m.n) return;
    float q[3];
    float4 a, b;
    pixel_out[i] = track_correspond(v, reinterpret_cast<const float4 *>(maps), &vm, i, d->r2_corr, d->min_dot, q, &a, &b);
}

extern "C" int oslamk_view_normals(const oslamk_view *v, float max_jump, float *maps, void *stream)
{
    if (v->w <= 0 || v->h <= 0 || !maps) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_view_normals, dim3((v->w + 31) / 32, (v->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *v, max_jump,
                       maps);
    return (int)hipGetLastError();
}

extern "C" int oslamk_track(const oslamk_view *v, const float *maps, const oslamk_track_member *d_mem, uint32_t n_mem,
                            int window, oslamk_track_rec *rec, void *stream)
{
    if (n_mem == 0) return 0;
    if (!maps || n_mem > OSLAMK_ARB_MAX_HYP || window < 0 || window > 3) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_track, dim3(n_mem), dim3(OSLAMK_TRACK_THREADS), 0, (hipStream_t)stream, *v, maps, d_mem, window, rec);
    return (int)hipGetLastError();
}

extern "C" int oslamk_track_corr(const oslamk_view *v, const float *maps, const oslamk_track_member *d_mem,
                                 uint32_t n_blocks, int32_t *pixel_out, void *stream)
{
    if (n_blocks == 0) return 0;
    if (!maps) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_track_corr, dim3(n_blocks), dim3(OSLAMK_TRACK_THREADS), 0, (hipStream_t)stream, *v, maps, d_mem,
                       pixel_out);
    return (int)hipGetLastError();
}
