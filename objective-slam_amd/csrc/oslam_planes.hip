/*
 * oslam_planes.hip -- the planes stage's kernels (semantics: include/oslam.h at oslam_view_planes; host side:
 * oslam_planes.c).  A call enqueues four kernels per round r = 0 .. max_planes - 1, whatever the image holds; each reads
 * the `done` word of the call's block first and leaves at once when the search has ended, so the end costs no host
 * round trip.
 *
 *   k_planes_score    the hot path: 256 candidates x w * h gates.  One workgroup of 256 threads, thread c = lattice node c
 *                     with its plane (n0, d0) in registers and a private counter.  The workgroup walks tiles of 256
 *                     consecutive pixels (tile t, t + grid, ...): every thread stages one pixel's map record into LDS
 *                     (x y z flag | nx ny nz, flag = free and has a normal), then all threads walk the tile, every lane
 *                     reading the same LDS address (a broadcast, no bank conflict).  A tile without a flagged pixel is
 *                     skipped after one barrier, and so is an unflagged pixel inside a tile (the branch is uniform).  One
 *                     integer atomicAdd per candidate and workgroup at the end; at most 512 workgroups.  This shape was
 *                     kept: the transposed one (a pixel per lane, a ballot per candidate) needs 256 ballots per 64 pixels
 *                     where this one needs 128 broadcast reads, and it was not measured.  Round 0 also counts the valid
 *                     pixels.  LDS 8 KiB.
 *   k_planes_moments  every workgroup picks the round's winner from the 256 counts (the same pick in each: integers
 *                     only), then a grid-stride walk over the pixels sums the ten int64 moments of the winner's inliers in
 *                     registers; per wave by shuffles, the four waves in LDS, one unsigned long long atomicAdd per sum
 *                     and workgroup (two's complement: the sums wrap to the signed result).
 *   k_planes_round    one workgroup: picks the winner again, decides the end of the search (no candidate, a count below
 *                     min_pixels, a degenerate fit) and otherwise the winner's own lane turns the moments into the plane
 *                     in double (k_normals' covariance and Jacobi sweeps, restated here so that k_normals' code stays
 *                     as it is) and writes the plane record.
 *   k_planes_label    one thread per pixel in 32 x 8 tiles: the label rule; the labelled pixels by ballot + popcount, the
 *                     four waves summed in LDS, one atomicAdd per workgroup.
 *   k_planes_mask     oslam_view_remove_planes: k_view_mask's tile and k_view_mask's three counters.
 *
 * No float atomics, no scratch.  Every sum is a whole number, so the results do not depend on the order of pixels, waves
 * or workgroups; every double operation is + - * / sqrt or a comparison and -ffp-contract=off keeps them apart: the
 * results equal tests/planes_ref.py bit for bit.
 *
 * Bounds.  Lattice node (a, b), 0 <= a, b <= 15, is pixel u = ((2a + 1) w) / 32 <= (31 w) / 32 < w for w >= 1, and the
 * same in v: inside the image, and (2a + 1) w <= 31 * 16384 fits an int.  Every other pixel index i is checked against
 * w * h (or (u, v) against (w, h)) before any load or store.  Pixel indices are size_t: w * h may reach 2^28.  The round
 * index r < max_planes <= OSLAMK_PLANES_MAX is checked by the launcher; a candidate index is threadIdx.x < 256.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam.h"
#include "oslam_depth_normal.h"
#include "oslam_kernels.h"

#define PLANES_THREADS 256

/* lattice node c of the image: its plane from the pixel's own point and normal; false when the pixel carries a label
 * or has no normal */
__device__ __forceinline__ bool planes_candidate(const oslamk_planes_args &a, int c, float &nx, float &ny, float &nz, float &d0,
                                                 float &px, float &py, float &pz)
{
    const int u = ((2 * (c & 15) + 1) * a.v.w) / 32, vv = ((2 * (c >> 4) + 1) * a.v.h) / 32;
    const size_t i = (size_t)vv * a.v.w + u;
    const float4 *maps = reinterpret_cast<const float4 *>(a.maps);
    const float4 m0 = maps[2 * i], m1 = maps[2 * i + 1];
    px = m0.x; py = m0.y; pz = m0.z;
    nx = m1.x; ny = m1.y; nz = m1.z;
    d0 = -((nx * px + ny * py) + nz * pz);
    return m0.w == 1.0f && a.labels[i] < 0;
}

/* The winner of the round over the workgroup's 256 threads (thread c = candidate c): 0 when no node is a candidate,
 * otherwise 1 + (count << 8 | 255 - c) of the largest count, the lowest index on a tie.  The same value in every thread;
 * sh: 4 words of LDS.  Ends with a barrier. */
__device__ __forceinline__ unsigned long long planes_pick(const uint32_t *counts, bool ok, unsigned long long *sh)
{
    const int c = (int)threadIdx.x;
    unsigned long long key = ok ? ((((unsigned long long)counts[c]) << 8) | (unsigned long long)(255 - c)) + 1ull : 0ull;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, off);
        key = o > key ? o : key;
    }
    if ((c & 63) == 0) sh[c >> 6] = key;
    __syncthreads();
    const unsigned long long k01 = sh[0] > sh[1] ? sh[0] : sh[1], k23 = sh[2] > sh[3] ? sh[2] : sh[3];
    return k01 > k23 ? k01 : k23;
}

__global__ __launch_bounds__(PLANES_THREADS) void k_planes_score(const oslamk_planes_args a, int r)
{
    __shared__ float4 sp[PLANES_THREADS], sn[PLANES_THREADS];
    __shared__ uint32_t sv[PLANES_THREADS / 64];
    if (a.blk->done) return;                        /* the whole grid leaves together */
    const int c = (int)threadIdx.x;
    float nx, ny, nz, d0, px, py, pz;
    const bool ok = planes_candidate(a, c, nx, ny, nz, d0, px, py, pz);
    const float4 *maps = reinterpret_cast<const float4 *>(a.maps);
    const size_t n_pix = (size_t)a.v.w * (size_t)a.v.h, n_tiles = (n_pix + PLANES_THREADS - 1) / PLANES_THREADS;
    uint32_t cnt = 0, n_valid = 0;

    for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const size_t i = t * PLANES_THREADS + threadIdx.x;
        float4 m0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m1 = m0;
        int flag = 0;
        if (i < n_pix) {
            m0 = maps[2 * i];
            if (m0.w == 1.0f && a.labels[i] < 0) {
                m1 = maps[2 * i + 1];
                flag = 1;
            }
            if (r == 0) n_valid += a.v.z[i] > 0.0f ? 1u : 0u;
        }
        __syncthreads();                            /* the walk over the tile before is over */
        sp[c] = make_float4(m0.x, m0.y, m0.z, flag ? 1.0f : 0.0f);
        sn[c] = m1;
        if (!__syncthreads_or(flag)) continue;      /* no free pixel with a normal in this tile */
        for (int k = 0; k < PLANES_THREADS; k++) {
            const float4 q = sp[k];                 /* the same address in every lane: a broadcast */
            if (q.w == 0.0f) continue;
            const float4 m = sn[k];
            const float dist = ((nx * q.x + ny * q.y) + nz * q.z) + d0;
            const float dot = (nx * m.x + ny * m.y) + nz * m.z;
            cnt += (fabsf(dist) <= a.dist_tol && dot >= a.min_normal_dot) ? 1u : 0u;
        }
    }
    if (ok && cnt) atomicAdd(&a.blk->counts[r][c], cnt);

    if (r == 0) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) n_valid += (uint32_t)__shfl_xor((int)n_valid, off);
        __syncthreads();
        if ((c & 63) == 0) sv[c >> 6] = n_valid;
        __syncthreads();
        if (c == 0) {
            const uint32_t s = (sv[0] + sv[1]) + (sv[2] + sv[3]);
            if (s) atomicAdd(&a.blk->valid_in, s);
        }
    }
}

__global__ __launch_bounds__(PLANES_THREADS) void k_planes_moments(const oslamk_planes_args a, int r)
{
    __shared__ unsigned long long shk[PLANES_THREADS / 64];
    __shared__ long long shm[PLANES_THREADS / 64][10];
    __shared__ float shw[8];
    if (a.blk->done) return;
    const int c = (int)threadIdx.x;
    float nx, ny, nz, d0, px, py, pz;
    const bool ok = planes_candidate(a, c, nx, ny, nz, d0, px, py, pz);
    const unsigned long long key = planes_pick(a.blk->counts[r], ok, shk);
    if (key == 0) return;                           /* the same key in every thread of the grid */
    if ((uint32_t)((key - 1) >> 8) < a.min_pixels) return;
    if (c == 255 - (int)((key - 1) & 255)) {        /* the winner's own thread publishes its plane and point */
        shw[0] = nx; shw[1] = ny; shw[2] = nz; shw[3] = d0;
        shw[4] = px; shw[5] = py; shw[6] = pz;
    }
    __syncthreads();
    nx = shw[0]; ny = shw[1]; nz = shw[2]; d0 = shw[3];
    px = shw[4]; py = shw[5]; pz = shw[6];

    const float4 *maps = reinterpret_cast<const float4 *>(a.maps);
    const size_t n_pix = (size_t)a.v.w * (size_t)a.v.h;
    long long n = 0, sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    for (size_t i = (size_t)blockIdx.x * PLANES_THREADS + threadIdx.x; i < n_pix; i += (size_t)gridDim.x * PLANES_THREADS) {
        const float4 m0 = maps[2 * i];
        if (!(m0.w == 1.0f && a.labels[i] < 0)) continue;
        const float4 m1 = maps[2 * i + 1];
        const float dist = ((nx * m0.x + ny * m0.y) + nz * m0.z) + d0;
        const float dot = (nx * m1.x + ny * m1.y) + nz * m1.z;
        if (!(fabsf(dist) <= a.dist_tol && dot >= a.min_normal_dot)) continue;
        const float fx = (m0.x - px) * a.scale, fy = (m0.y - py) * a.scale, fz = (m0.z - pz) * a.scale;
        /* the range test in float before the conversion: |q_a| <= 2^17, a product <= 2^34, a sum over 2^28 pixels <= 2^62 */
        if (!(fabsf(fx) <= OSLAMK_PLANES_BOUND && fabsf(fy) <= OSLAMK_PLANES_BOUND && fabsf(fz) <= OSLAMK_PLANES_BOUND)) continue;
        const long long qx = (long long)(int32_t)rintf(fx), qy = (long long)(int32_t)rintf(fy), qz = (long long)(int32_t)rintf(fz);
        n += 1;
        sx += qx;
        sy += qy;
        sz += qz;
        sxx += qx * qx;
        sxy += qx * qy;
        sxz += qx * qz;
        syy += qy * qy;
        syz += qy * qz;
        szz += qz * qz;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n += __shfl_xor(n, off);
        sx += __shfl_xor(sx, off);
        sy += __shfl_xor(sy, off);
        sz += __shfl_xor(sz, off);
        sxx += __shfl_xor(sxx, off);
        sxy += __shfl_xor(sxy, off);
        sxz += __shfl_xor(sxz, off);
        syy += __shfl_xor(syy, off);
        syz += __shfl_xor(syz, off);
        szz += __shfl_xor(szz, off);
    }
    if ((c & 63) == 0) {
        long long *m = shm[c >> 6];
        m[0] = n;   m[1] = sx;  m[2] = sy;  m[3] = sz;  m[4] = sxx;
        m[5] = sxy; m[6] = sxz; m[7] = syy; m[8] = syz; m[9] = szz;
    }
    __syncthreads();
    if (c < 10) {
        const long long s = (shm[0][c] + shm[1][c]) + (shm[2][c] + shm[3][c]);
        if (s) atomicAdd(&a.blk->moments[r][c], (unsigned long long)s);
    }
}

/* one Jacobi rotation in the plane (p, q); r is the third index.  vNp / vNq: row N of V.  The statement of
 * oslam_normals.hip's, operation for operation */
__device__ __forceinline__ void planes_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                              double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = theta < 0.0 ? -theta : theta;
    const double tt = 1.0 / (at + sqrt(theta * theta + 1.0));
    const double t = theta < 0.0 ? -tt : tt;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
    x = v0p; y = v0q;
    v0p = c * x - s * y;
    v0q = s * x + c * y;
    x = v1p; y = v1q;
    v1p = c * x - s * y;
    v1q = s * x + c * y;
    x = v2p; y = v2q;
    v2p = c * x - s * y;
    v2q = s * x + c * y;
}

__global__ __launch_bounds__(PLANES_THREADS) void k_planes_round(const oslamk_planes_args a, int r)
{
    __shared__ unsigned long long shk[PLANES_THREADS / 64];
    if (a.blk->done) return;
    const int c = (int)threadIdx.x;
    float fnx, fny, fnz, d0, px, py, pz;
    const bool ok = planes_candidate(a, c, fnx, fny, fnz, d0, px, py, pz);
    const unsigned long long key = planes_pick(a.blk->counts[r], ok, shk);
    if (key == 0) {
        if (c == 0) a.blk->done = 3;
        return;
    }
    if ((uint32_t)((key - 1) >> 8) < a.min_pixels) {
        if (c == 0) a.blk->done = 1;
        return;
    }
    if (c != 255 - (int)((key - 1) & 255)) return;  /* one lane goes on: the winner's own, which holds its point */

    const unsigned long long *m = a.blk->moments[r];
    const long long n = (long long)m[0], sx = (long long)m[1], sy = (long long)m[2], sz = (long long)m[3];
    const long long sxx = (long long)m[4], sxy = (long long)m[5], sxz = (long long)m[6], syy = (long long)m[7];
    const long long syz = (long long)m[8], szz = (long long)m[9];
    if (n < 3) {
        a.blk->done = 2;
        return;
    }
    const double dn = (double)n;
    const double mx = (double)sx / dn, my = (double)sy / dn, mz = (double)sz / dn;
    double a00 = (double)sxx / dn - mx * mx, a01 = (double)sxy / dn - mx * my, a02 = (double)sxz / dn - mx * mz;
    double a11 = (double)syy / dn - my * my, a12 = (double)syz / dn - my * mz, a22 = (double)szz / dn - mz * mz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int s = 0; s < OSLAM_NORMALS_SWEEPS; s++) {
        planes_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        planes_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        planes_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    const double lo01 = a00 < a11 ? a00 : a11, hi01 = a00 < a11 ? a11 : a00;
    const double lmin = lo01 < a22 ? lo01 : a22;
    const double lmax = hi01 < a22 ? a22 : hi01;
    const double h2 = hi01 < a22 ? hi01 : a22;
    const double lmid = lo01 < h2 ? h2 : lo01;
    if (lmid <= a.line_ratio * lmax) {
        a.blk->done = 2;
        return;
    }
    double nx, ny, nz;
    if (a00 <= a11 && a00 <= a22) { nx = v00; ny = v10; nz = v20; }
    else if (a11 <= a22)          { nx = v01; ny = v11; nz = v21; }
    else                          { nx = v02; ny = v12; nz = v22; }
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len;
    ny = ny / len;
    nz = nz / len;
    const double sc = (double)a.scale;
    const double cx = (double)px + mx / sc, cy = (double)py + my / sc, cz = (double)pz + mz / sc;
    if ((nx * cx + ny * cy) + nz * cz > 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    const double d = -((nx * cx + ny * cy) + nz * cz);
    oslamk_plane *o = &a.blk->rec[r];
    o->normal[0] = (float)nx;
    o->normal[1] = (float)ny;
    o->normal[2] = (float)nz;
    o->d = (float)d;
    o->support = (uint32_t)n;
    o->pixels = 0;
    o->candidate = (uint32_t)c;
    o->rms = (float)(sqrt(lmin < 0.0 ? 0.0 : lmin) / sc);
    a.blk->n_planes = (uint32_t)r + 1u;
}

__global__ __launch_bounds__(PLANES_THREADS) void k_planes_label(const oslamk_planes_args a, int r)
{
    __shared__ uint32_t sh[PLANES_THREADS / 64];
    if (a.blk->done) return;
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), vv = blockIdx.y * 8 + (threadIdx.x >> 5);
    const float nx = a.blk->rec[r].normal[0], ny = a.blk->rec[r].normal[1], nz = a.blk->rec[r].normal[2], d = a.blk->rec[r].d;
    bool hit = false;
    if (u < a.v.w && vv < a.v.h) {
        const size_t i = (size_t)vv * a.v.w + u;
        const float z = a.v.z[i];
        if (z > 0.0f && a.labels[i] < 0) {
            const depth_cam cam = {a.v.fx, a.v.fy, a.v.cx, a.v.cy, 1.0f, a.v.z_min, a.v.z_max, 0.0f};
            float p[3];
            back_project(u, vv, z, cam, p);
            const float dist = ((nx * p[0] + ny * p[1]) + nz * p[2]) + d;
            if (fabsf(dist) <= a.dist_tol) {
                const float4 *maps = reinterpret_cast<const float4 *>(a.maps);
                hit = true;
                if (maps[2 * i].w == 1.0f) {
                    const float4 m1 = maps[2 * i + 1];
                    hit = (nx * m1.x + ny * m1.y) + nz * m1.z >= a.label_min_dot;
                }
                if (hit) a.labels[i] = r;
            }
        }
    }
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (s) atomicAdd(&a.blk->rec[r].pixels, s);
    }
}

__global__ __launch_bounds__(256) void k_planes_mask(const oslamk_view v, const int32_t *labels, int mode, int32_t only,
                                                     float *z_out, uint32_t *counts)
{
    __shared__ uint32_t sh[4][3];
    const int u = blockIdx.x * 32 + (threadIdx.x & 31), vv = blockIdx.y * 8 + (threadIdx.x >> 5);
    bool valid = false, object = false, kept = false;
    if (u < v.w && vv < v.h) {
        const size_t i = (size_t)vv * v.w + u;
        const float zo = v.z[i];
        valid = zo > 0.0f;
        if (valid) {
            const int32_t l = labels[i];
            object = l >= 0 && (only < 0 || l == only);
        }
        kept = valid && (mode == 1 ? object : !object);
        z_out[i] = kept ? zo : 0.0f;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b0 = __ballot(valid), b1 = __ballot(object), b2 = __ballot(kept);
    if (lane == 0) {
        sh[wv][0] = (uint32_t)__popcll(b0);
        sh[wv][1] = (uint32_t)__popcll(b1);
        sh[wv][2] = (uint32_t)__popcll(b2);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t s = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
        if (s) atomicAdd(&counts[threadIdx.x], s);
    }
}

extern "C" int oslamk_planes_find(const oslamk_planes_args *a, unsigned max_planes, void *stream)
{
    if (a->v.w <= 0 || a->v.h <= 0 || a->v.w > 16384 || a->v.h > 16384 || !a->maps || !a->labels || !a->blk ||
        max_planes < 1 || max_planes > OSLAMK_PLANES_MAX)
        return (int)hipErrorInvalidValue;
    const size_t n_pix = (size_t)a->v.w * (size_t)a->v.h, n_tiles = (n_pix + PLANES_THREADS - 1) / PLANES_THREADS;
    const unsigned groups = (unsigned)(n_tiles < OSLAMK_PLANES_MAX_GROUPS ? n_tiles : OSLAMK_PLANES_MAX_GROUPS);
    const dim3 tiles((a->v.w + 31) / 32, (a->v.h + 7) / 8);
    for (unsigned r = 0; r < max_planes; r++) {
        hipLaunchKernelGGL(k_planes_score, dim3(groups), dim3(PLANES_THREADS), 0, (hipStream_t)stream, *a, (int)r);
        hipLaunchKernelGGL(k_planes_moments, dim3(groups), dim3(PLANES_THREADS), 0, (hipStream_t)stream, *a, (int)r);
        hipLaunchKernelGGL(k_planes_round, dim3(1), dim3(PLANES_THREADS), 0, (hipStream_t)stream, *a, (int)r);
        hipLaunchKernelGGL(k_planes_label, tiles, dim3(PLANES_THREADS), 0, (hipStream_t)stream, *a, (int)r);
        const int e = (int)hipGetLastError();
        if (e != 0) return e;
    }
    return 0;
}

extern "C" int oslamk_planes_mask(const oslamk_view *v, const int32_t *labels, int mode, int32_t only, float *z_out,
                                  uint32_t *counts, void *stream)
{
    if (v->w <= 0 || v->h <= 0 || !labels || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_planes_mask, dim3((v->w + 31) / 32, (v->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *v, labels,
                       mode, only, z_out, counts);
    return (int)hipGetLastError();
}
