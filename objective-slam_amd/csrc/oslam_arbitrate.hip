/*
 * oslam_arbitrate.hip -- the arbitration stage's kernels (semantics: include/oslam.h at oslam_arbitrate; host side:
 * oslam_arbitrate.c).
 *
 *   k_claim      one thread per model point, every hypothesis of the call in one grid (y = hypothesis, x = block of 256
 *                model points), the shape of k_verify and its class (oslam_verify_class.h).  A SUPPORTED point adds
 *                (1 << 40) + q to the 64-bit word of its hypothesis and tile: count in the upper 24 bits, sum of the
 *                quantised residuals in the lower 40.  One integer atomic per point: the table does not depend on the
 *                order of the points.
 *   k_arbitrate  one workgroup runs the whole elimination.  The table is copied into LDS when it fits
 *                (OSLAMK_ARB_LDS_BYTES), otherwise every round reads it from L2.  Per round: the threads stride over
 *                the tiles, find each tile's owner among the live claimants and count `owned` with integer LDS atomics;
 *                the loser comes from a tree reduction under a total order (share ascending, index descending), so
 *                the order of the reduction does not matter.  No float atomics; the only float operation is the
 *                division owned / claimed.
 * Bounds: the tile index is checked against n_tiles before the atomic; every hypothesis index is < n_mem <=
 * OSLAMK_ARB_MAX_HYP (checked by the launcher), every table index is < n_mem * n_tiles.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"
#include "oslam_verify_class.h"

typedef unsigned long long u64;
#define ARB_SUM_MASK ((1ull << OSLAMK_ARB_CNT_SHIFT) - 1ull)

__global__ __launch_bounds__(OSLAMK_VERIFY_THREADS) void k_claim(const oslamk_view v, const oslamk_verify_member *mem,
                                                                 int window, const oslamk_arb_grid g, u64 *claims)
{
    const uint32_t j = blockIdx.y;
    const oslamk_verify_member *d = &mem[j];
    if (blockIdx.x >= d->n_blocks) return;
    const int i = (int)(blockIdx.x * OSLAMK_VERIFY_THREADS + threadIdx.x);
    if (i >= d->m.n) return;
    int u = 0, vv = 0;
    float r = 0.0f;
    if (oslam_verify_class<true>(v, d, i, window, &u, &vv, &r) != 2) return;
    const float x = r * (65535.0f / d->tol);
    const uint32_t q = x < 65535.0f ? (uint32_t)x : 65535u;
    const uint32_t t = (uint32_t)(vv / g.tile) * (uint32_t)g.tiles_x + (uint32_t)(u / g.tile);
    if (t < g.n_tiles) atomicAdd(&claims[(size_t)j * g.n_tiles + t], (1ull << OSLAMK_ARB_CNT_SHIFT) + (u64)q);
}

/* the live claimant of tile t with the smallest mean residual (sum_a * cnt_b < sum_b * cnt_a; ties: the lower index) */
__device__ __forceinline__ int arb_owner(const u64 *tb, uint32_t H, uint32_t n_tiles, uint32_t t, const uint32_t *live)
{
    int best = -1;
    u64 bs = 0, bc = 0;
    for (uint32_t h = 0; h < H; h++) {
        if (!live[h]) continue;
        const u64 w = tb[(size_t)h * n_tiles + t];
        const u64 c = w >> OSLAMK_ARB_CNT_SHIFT;
        if (!c) continue;
        const u64 s = w & ARB_SUM_MASK;
        if (best < 0 || s * bc < bs * c) {
            best = (int)h;
            bs = s;
            bc = c;
        }
    }
    return best;
}

template <bool LDS>
__global__ __launch_bounds__(OSLAMK_ARB_THREADS) void k_arbitrate(const oslamk_verify_member *mem, uint32_t H,
                                                                  uint32_t n_tiles, const u64 *claims, uint32_t min_tiles,
                                                                  float min_share, oslamk_arb_rec *rec)
{
    extern __shared__ u64 s_tbl[];
    __shared__ uint32_t s_live[OSLAMK_ARB_MAX_HYP], s_claimed[OSLAMK_ARB_MAX_HYP], s_owned[OSLAMK_ARB_MAX_HYP],
        s_beat[OSLAMK_ARB_MAX_HYP];
    __shared__ float s_rs[OSLAMK_ARB_THREADS];
    __shared__ uint32_t s_rb[OSLAMK_ARB_THREADS];
    __shared__ int s_ri[OSLAMK_ARB_THREADS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n_ent = (size_t)H * n_tiles;

    if (LDS)
        for (size_t e = tid; e < n_ent; e += OSLAMK_ARB_THREADS) s_tbl[e] = claims[e];
    const u64 *tb = LDS ? s_tbl : claims;
    __syncthreads();

    /* per hypothesis: claimed tiles, SUPPORTED points and the sum of their q; one wave per hypothesis, no atomics */
    for (uint32_t h = wave; h < H; h += OSLAMK_ARB_THREADS / 64) {
        uint32_t cl = 0, cn = 0;
        u64 sm = 0;
        for (uint32_t t = lane; t < n_tiles; t += 64) {
            const u64 w = tb[(size_t)h * n_tiles + t];
            const uint32_t c = (uint32_t)(w >> OSLAMK_ARB_CNT_SHIFT);
            if (c) {
                cl++;
                cn += c;
                sm += w & ARB_SUM_MASK;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            cl += __shfl_down(cl, o);
            cn += __shfl_down(cn, o);
            sm += __shfl_down(sm, o);
        }
        if (lane == 0) {
            oslamk_arb_rec r;
            r.claimed = cl;
            r.owned = 0;
            r.share = 0.0f;
            r.kept = 0;
            r.suppressed_by = -1;
            r.cnt_total = cn;
            r.sum_total = sm;
            rec[1 + h] = r;
            s_claimed[h] = cl;
            s_live[h] = mem[h].n_blocks != 0 && cl >= 1 && cl >= min_tiles;
        }
    }
    __syncthreads();

    uint32_t rounds = 0;
    for (uint32_t round = 0; round < H; round++) {
        for (uint32_t h = tid; h < H; h += OSLAMK_ARB_THREADS) s_owned[h] = 0;
        __syncthreads();
        for (uint32_t t = tid; t < n_tiles; t += OSLAMK_ARB_THREADS) {
            const int o = arb_owner(tb, H, n_tiles, t, s_live);
            if (o >= 0) atomicAdd(&s_owned[o], 1u);
        }
        __syncthreads();
        /* the loser: smallest share, ties the larger index */
        float bs = 0.0f;
        int bi = -1;
        for (uint32_t h = tid; h < H; h += OSLAMK_ARB_THREADS) {
            if (!s_live[h]) continue;
            const float sh = (float)s_owned[h] / (float)s_claimed[h];
            rec[1 + h].owned = s_owned[h];
            rec[1 + h].share = sh;
            if (bi < 0 || sh <= bs) {            /* h ascends: <= keeps the larger index of a tie */
                bs = sh;
                bi = (int)h;
            }
        }
        s_rs[tid] = bs;
        s_ri[tid] = bi;
        __syncthreads();
        for (uint32_t s = OSLAMK_ARB_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const float os = s_rs[tid + s];
                const int oi = s_ri[tid + s];
                if (oi >= 0 && (s_ri[tid] < 0 || os < s_rs[tid] || (os == s_rs[tid] && oi > s_ri[tid]))) {
                    s_rs[tid] = os;
                    s_ri[tid] = oi;
                }
            }
            __syncthreads();
        }
        const int loser = s_ri[0];
        const float ls = s_rs[0];
        if (loser < 0) break;                    /* nobody is live */
        rounds++;
        if (!(ls < min_share)) break;
        /* who suppresses it: the live hypothesis that owns most of the loser's claimed tiles, ties the lower index */
        for (uint32_t h = tid; h < H; h += OSLAMK_ARB_THREADS) s_beat[h] = 0;
        __syncthreads();
        for (uint32_t t = tid; t < n_tiles; t += OSLAMK_ARB_THREADS) {
            if (!(tb[(size_t)loser * n_tiles + t] >> OSLAMK_ARB_CNT_SHIFT)) continue;
            const int o = arb_owner(tb, H, n_tiles, t, s_live);
            if (o >= 0 && o != loser) atomicAdd(&s_beat[o], 1u);
        }
        __syncthreads();
        uint32_t bb = 0;
        bi = -1;
        for (uint32_t h = tid; h < H; h += OSLAMK_ARB_THREADS)
            if (s_beat[h] > bb) {                /* h ascends: > keeps the lower index of a tie */
                bb = s_beat[h];
                bi = (int)h;
            }
        s_rb[tid] = bb;
        s_ri[tid] = bi;
        __syncthreads();
        for (uint32_t s = OSLAMK_ARB_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const uint32_t ob = s_rb[tid + s];
                const int oi = s_ri[tid + s];
                if (oi >= 0 && (s_ri[tid] < 0 || ob > s_rb[tid] || (ob == s_rb[tid] && oi < s_ri[tid]))) {
                    s_rb[tid] = ob;
                    s_ri[tid] = oi;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            rec[1 + loser].suppressed_by = s_ri[0];
            s_live[loser] = 0;
        }
        __syncthreads();
    }
    for (uint32_t h = tid; h < H; h += OSLAMK_ARB_THREADS) rec[1 + h].kept = (int32_t)s_live[h];
    if (tid == 0) {
        oslamk_arb_rec r;
        r.claimed = rounds;
        r.owned = 0;
        r.share = 0.0f;
        r.kept = 0;
        r.suppressed_by = -1;
        r.cnt_total = 0;
        r.sum_total = 0;
        rec[0] = r;
    }
}

static bool arb_args_ok(uint32_t n_mem, uint32_t n_tiles)
{
    return n_mem >= 1 && n_mem <= OSLAMK_ARB_MAX_HYP && n_tiles >= 1;
}

extern "C" int oslamk_claim(const oslamk_view *v, const oslamk_verify_member *d_mem, uint32_t n_mem, uint32_t max_blocks,
                            int window, oslamk_arb_grid g, unsigned long long *claims, void *stream)
{
    if (max_blocks == 0) return 0;
    if (!arb_args_ok(n_mem, g.n_tiles) || window < 0 || window > 3 || g.tile < 4 || g.tile > 128 || g.tiles_x < 1 ||
        (uint32_t)g.tiles_x != (uint32_t)((v->w + g.tile - 1) / g.tile) ||
        g.n_tiles != (uint32_t)g.tiles_x * (uint32_t)((v->h + g.tile - 1) / g.tile))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_claim, dim3(max_blocks, n_mem), dim3(OSLAMK_VERIFY_THREADS), 0, (hipStream_t)stream, *v, d_mem,
                       window, g, claims);
    return (int)hipGetLastError();
}

extern "C" int oslamk_arbitrate(const oslamk_verify_member *d_mem, uint32_t n_mem, uint32_t n_tiles,
                                const unsigned long long *claims, uint32_t min_tiles, float min_owned_share,
                                oslamk_arb_rec *rec, void *stream)
{
    if (!arb_args_ok(n_mem, n_tiles)) return (int)hipErrorInvalidValue;
    const size_t bytes = (size_t)n_mem * n_tiles * sizeof(u64);
    if (bytes <= OSLAMK_ARB_LDS_BYTES)
        hipLaunchKernelGGL(k_arbitrate<true>, dim3(1), dim3(OSLAMK_ARB_THREADS), bytes, (hipStream_t)stream, d_mem, n_mem,
                           n_tiles, claims, min_tiles, min_owned_share, rec);
    else
        hipLaunchKernelGGL(k_arbitrate<false>, dim3(1), dim3(OSLAMK_ARB_THREADS), 0, (hipStream_t)stream, d_mem, n_mem,
                           n_tiles, claims, min_tiles, min_owned_share, rec);
    return (int)hipGetLastError();
}
