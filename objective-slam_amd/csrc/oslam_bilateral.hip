/*
 * oslam_bilateral.hip -- the bilateral depth filter's kernel (semantics: include/oslam.h at oslam_view_bilateral; host
 * side: oslam_bilateral.c).
 *
 *   k_bilateral   one launch per call: the z image of a view (w x h) -> the filtered z image of the same size.  One
 *                 thread per output pixel in 32 x 8 tiles (k_pyr_down's tiling).  A value of the image is read by up to
 *                 (2R + 1)^2 = 289 threads and a thread has 169 .. 289 taps at the usual radii, so the workgroup first
 *                 stages the (32 + 2R) x (8 + 2R) pixels its windows cover in LDS, at a fixed pitch of 48 floats, and the
 *                 288 words of the weight table beside them (a per-lane index into constant memory would serialise):
 *                 4608 + 1152 = 5760 bytes of static LDS, whatever the radius.  Tile elements outside the image are
 *                 loaded as 0.0f, so the rule's z > 0 test does the clipping and the tap loop has no bounds checks.
 *                 Every thread, also one whose pixel lies outside the image, loads its share of the tile and reaches the
 *                 barrier; only then does it skip its pixel.  The taps are walked dy outer, dx inner, and added in float
 *                 in that order.  The translation unit is built with -ffp-contract=off: no fused multiply-add, and the
 *                 division is the correctly rounded one.  The valid pixels and the taps are summed over the wave
 *                 (wave_sum, oslam_block_scan.h), the four waves in LDS, one integer atomicAdd per counter and
 *                 workgroup.  No scratch.
 * Bounds: a tile index is ty * 48 + tx with tx < 32 + 2R <= 48 and ty < 8 + 2R <= 24, below the 1152 floats of the tile;
 * a tap reads (ly + R + dy, lx + R + dx) with ly < 8, lx < 32 and |dy|, |dx| <= R, inside the same rectangle.  A global
 * load happens only for 0 <= x < w and 0 <= y < h, the store only for u < w and v < h; both index with size_t.  The table
 * index is (int)(t * 32) with 0 <= t < 9, below 288.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_block_scan.h"
#include "oslam_gauss_table.h"
#include "oslam_kernels.h"

#define BIL_PITCH (32 + 2 * OSLAMK_BILATERAL_MAX_RADIUS)
#define BIL_ROWS (8 + 2 * OSLAMK_BILATERAL_MAX_RADIUS)

static __device__ const uint32_t d_gauss_bits[OSLAM_GAUSS_N] = {OSLAM_GAUSS_BITS_FLAT};

__global__ __launch_bounds__(256) void k_bilateral(const oslamk_view sv, int R, float inv_s, float inv_r, float *z_out,
                                                   uint32_t *counts)
{
    __shared__ float tile[BIL_ROWS * BIL_PITCH];
    __shared__ float gauss[OSLAM_GAUSS_N];
    __shared__ uint32_t s_valid[4], s_taps[4];
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int x0 = blockIdx.x * 32 - R, y0 = blockIdx.y * 8 - R;
    const int tw = 32 + 2 * R, th = 8 + 2 * R;
    for (int i = threadIdx.x; i < tw * th; i += 256) {
        const int ty = i / tw, tx = i - ty * tw;
        const int x = x0 + tx, y = y0 + ty;
        float z = 0.0f;
        if (x >= 0 && x < sv.w && y >= 0 && y < sv.h) z = sv.z[(size_t)y * sv.w + x];
        tile[ty * BIL_PITCH + tx] = z;
    }
    for (int i = threadIdx.x; i < OSLAM_GAUSS_N; i += 256) gauss[i] = __uint_as_float(d_gauss_bits[i]);
    __syncthreads();

    const int u = blockIdx.x * 32 + lx, v = blockIdx.y * 8 + ly;
    uint32_t taps = 0, valid = 0;
    if (u < sv.w && v < sv.h) {
        const float *centre = tile + (ly + R) * BIL_PITCH + (lx + R);
        const float c = *centre;
        float out = 0.0f;
        if (c != 0.0f) {
            float sd = 0.0f, sw = 0.0f;
            for (int dy = -R; dy <= R; dy++) {
                const float *row = centre + dy * BIL_PITCH;
                for (int dx = -R; dx <= R; dx++) {
                    const float z = row[dx];
                    const float d = z - c;
                    const float t = (float)(dx * dx + dy * dy) * inv_s + (d * d) * inv_r;
                    if (z > 0.0f && t < (float)OSLAM_GAUSS_CUT) {
                        const float wgt = gauss[(int)(t * (float)OSLAM_GAUSS_BINS)];
                        sd += wgt * d;
                        sw += wgt;
                        taps++;
                    }
                }
            }
            out = fminf(fmaxf(c + sd / sw, sv.z_min), sv.z_max);
        }
        valid = out > 0.0f;
        z_out[(size_t)v * sv.w + u] = out;
    }
    valid = wave_sum(valid);
    taps = wave_sum(taps);
    if ((threadIdx.x & 63u) == 0u) {
        s_valid[threadIdx.x >> 6] = valid;
        s_taps[threadIdx.x >> 6] = taps;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const uint32_t *s = threadIdx.x == 0 ? s_valid : s_taps;
        const uint32_t sum = (s[0] + s[1]) + (s[2] + s[3]);
        if (sum) atomicAdd(&counts[threadIdx.x], sum);
    }
}

extern "C" int oslamk_bilateral(const oslamk_view *src, int radius, float inv_s, float inv_r, float *z_out,
                                uint32_t *counts, void *stream)
{
    if (!src || !src->z || !z_out || !counts || src->w <= 0 || src->h <= 0 || radius < 1 ||
        radius > OSLAMK_BILATERAL_MAX_RADIUS || !(inv_s >= 0.0f) || !isfinite(inv_s) || !(inv_r >= 0.0f) || !isfinite(inv_r))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bilateral, dim3((src->w + 31) / 32, (src->h + 7) / 8), dim3(256), 0, (hipStream_t)stream, *src,
                       radius, inv_s, inv_r, z_out, counts);
    return (int)hipGetLastError();
}
