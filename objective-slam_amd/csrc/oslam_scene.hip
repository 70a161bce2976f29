/*
 * oslam_scene.hip -- the scene-key stage of the PPF registration path (gfx950; host side: oslam_scene.c for the Morton
 * order and its boxes, oslam_vote.c for the launches; the overview of the path is at the top of oslam_kernels.h).
 * Built with -ffp-contract=off: the float sequences of ppf_core.h must round exactly as on the host.
 *
 * What the reference does with N^2-sized arrays (Scene::Scene's key pass, scene.cu:24-55: K1 ppf_kernel + K2
 * ppf_hash_kernel) is fused with the lookup of model.cu:96-97:
 *   k_scene_count  per reference point, the pairs whose distance bin can reach a model key: sizes the hit lists by
 *                  demand;
 *   k_scene_hits   per (8 reference points, tile of scene points): distance bin of every pair, unreachable bins dropped,
 *                  the rest compacted in LDS; the pair's feature as bins -> key map (one load, no hash, no probing) ->
 *                  per-reference hit list {key number} + {theta_v, i} written by wave-aggregated appends.
 * Both drop whole blocks (reference point, 64 points of the scene's Morton order) whose box cannot hold a pair within
 * reach (group_keep).  Bounds: a place of the order is checked against the scene's size before it is loaded; a hit list
 * has keep_count[] places by the same predicate in both kernels, and a hit that would not fit is dropped and flagged
 * (list_overflow), never written.  The lane helpers are oslam_lane.h's; the hit sort that follows is oslam_sort.hip.
 * The resources are in profiles/r31_kernel_resources_split.txt.
 */
#include <hip/hip_runtime.h>

#include "oslam_kernels.h"
#include "ppf_core.h"
#include "oslam_lane.h"

/* --------------------------------------------------------------------------
 * scene pair keys -> hit lists (Scene::Scene's key pass, scene.cu:24-55: K1 ppf_kernel + K2
 * ppf_hash_kernel, fused with the lookup of model.cu:96-97)
 * ------------------------------------------------------------------------*/
#define KEY_TILE 4096                  /* scene points per counting workgroup */
#define COUNT_REFS 8                   /* reference points one workgroup handles against its tile */
#define HIT_TILE 1024                  /* scene points per hit-list workgroup (indices inside it fit 16 bits) */

__device__ const uint32_t d_acos_lut[2 * PC_ACOS_CELLS] = {PC_ACOS_LUT_FLAT};

/* The distance bin of a pair, pc_pair_dist_bin's value at a third of its cost: the hardware's approximate
 * square root (1 ulp) gives the quotient to 3e-7 relative, which decides the bin unless the quotient lies
 * within 1e-6 relative of a bin edge (or the distance is tiny, huge or not a number) -- those lanes, a few
 * in a million, take the exact sequence. */
__device__ __forceinline__ int pair_dist_bin_quick(float dx, float dy, float dz, float d_dist, float inv_d_dist)
{
    const float d2 = dx * dx + dy * dy + dz * dz;
    const float q = __builtin_amdgcn_sqrtf(d2) * inv_d_dist;
    const float kf = __builtin_floorf(q);
    const float fr = q - kf, tol = q * 1e-6f;
    int k = (int)kf;
    if (!(d2 > 1e-30f && q < 1048576.0f && fr > tol && 1.0f - fr > tol)) k = pc_pair_dist_bin(dx, dy, dz, d_dist, inv_d_dist);
    return k;
}

/* Can a pair in distance bin k produce a key of the model at all?  Exact: table.reach has a bit for every
 * distance bin that holds a model key, FNV collisions included (`reach` = the workgroup's LDS copy of its first
 * reach_words words, the rest are zero); bins beyond the bitset and non-finite distances (k < 0) are kept. */
__device__ __forceinline__ bool bin_in_reach(const uint32_t *reach, uint32_t reach_words, int k)
{
    if ((uint32_t)k >= OSLAMK_REACH_BINS) return true;
    const uint32_t w = (uint32_t)k >> 5;
    return w < reach_words && ((reach[w] >> ((uint32_t)k & 31u)) & 1u);
}

/* Phase 1 of the two scene-key kernels, written once: k_scene_count sizes the hit lists by it and k_scene_hits fills
 * them by it, and list_overflow & 1 (hits_chunk) checks at run time that the two agreed.
 * The COUNT_REFS reference points of workgroup column g0 / COUNT_REFS: index and position, in scalar registers (a
 * group beyond the launch: no point's index, at the origin). */
struct KeyRefs {
    uint32_t rr[COUNT_REFS];
    float prx[COUNT_REFS], pry[COUNT_REFS], prz[COUNT_REFS];
};
__device__ __forceinline__ void key_refs_load(KeyRefs &r, const oslamk_vote_args &a, int g0)
{
#pragma unroll
    for (int g = 0; g < COUNT_REFS; g++) {
        const bool v = g0 + g < a.n_launch;
        r.rr[g] = v ? a.ref_idx[a.first_ref + g0 + g] : 0xffffffffu;
        r.prx[g] = v ? a.scene.px[r.rr[g]] : 0.0f;
        r.pry[g] = v ? a.scene.py[r.rr[g]] : 0.0f;
        r.prz[g] = v ? a.scene.pz[r.rr[g]] : 0.0f;
    }
}
/* the workgroup's LDS copy of the reach bitset (256 threads; the caller's barrier follows) */
__device__ __forceinline__ void reach_fill(uint32_t *s_reach, const uint32_t *reach, uint32_t reach_words)
{
    for (uint32_t w = threadIdx.x; w < reach_words; w += 256) s_reach[w] = reach[w];
}
/* Is the pair (reference point g of the workgroup, scene point i at x y z) kept?  `in`: i is a point of the scene;
 * `valid`: what the kernel asks of g itself (k_scene_hits: it is inside the launch; k_scene_count guards its last add). */
__device__ __forceinline__ bool pair_keep(const KeyRefs &r, int g, bool valid, int i, bool in, float x, float y, float z,
                                          const oslamk_vote_args &a, const uint32_t *s_reach, uint32_t reach_words)
{
    const int k = pair_dist_bin_quick(x - r.prx[g], y - r.pry[g], z - r.prz[g], a.d_dist, a.inv_d_dist);
    return in && (uint32_t)i != r.rr[g] && valid && bin_in_reach(s_reach, reach_words, k);
}

/* Does the bitset have a bin in [kmin, kmax] (0 <= kmin <= kmax) that bin_in_reach keeps?  A range that runs past the
 * bitset is kept like its bins are. */
__device__ __forceinline__ bool range_in_reach(const uint32_t *reach, uint32_t reach_words, int kmin, int kmax)
{
    if (kmax >= OSLAMK_REACH_BINS) return true;
    const uint32_t w0 = (uint32_t)kmin >> 5, w1 = (uint32_t)kmax >> 5;
    for (uint32_t w = w0; w <= w1 && w < reach_words; w++) {
        uint32_t m = reach[w];
        if (w == w0) m &= 0xffffffffu << ((uint32_t)kmin & 31u);
        if (w == w1) m &= 0xffffffffu >> (31u - ((uint32_t)kmax & 31u));
        if (m) return true;
    }
    return false;
}
/* Phase 1 by groups: can reference point g0 + g of the launch have a pair that pair_keep keeps among the 64 points of
 * group grp of the scene's Morton order?  One lane answers for one (reference point, group): the bins the group's box
 * can lie in seen from the point (pc_box_bin_range, conservative) against the reach bitset.  No for a group beyond the
 * scene and a reference point beyond the launch (pair_keep keeps none of theirs); yes wherever the box gives no range. */
__device__ __forceinline__ bool group_keep(const oslamk_vote_args &a, int g, int grp, const uint32_t *s_reach, uint32_t reach_words)
{
    if (g >= a.n_launch || grp * OSLAMK_ORDER_GROUP >= a.scene.n) return false;
#ifdef KEY_DIAG_KEEP_ALL        /* timing only (make EXTRA=-DKEY_DIAG_KEEP_ALL): no block is dropped -- what the order and the tests cost by themselves */
    return true;
#endif
    const uint32_t rr = a.ref_idx[a.first_ref + g];
    int kmin, kmax;
    if (!pc_box_bin_range(a.order.box + 6 * (size_t)grp, a.scene.px[rr], a.scene.py[rr], a.scene.pz[rr], a.inv_d_dist, &kmin, &kmax))
        return true;
    return range_in_reach(s_reach, reach_words, kmin, kmax);
}

/* Sizes the hit lists by demand: keep_count[ref] = pairs of the reference point whose distance bin is within
 * reach (what k_scene_hits keys and looks up), an upper bound of its hits -- 16 % above them on the bench
 * scene.  A workgroup tests its tile of scene points against COUNT_REFS reference points (their coordinates
 * sit in scalar registers), so a point is loaded once per 8 pairs.  The tile is a piece of the scene's Morton order
 * (oslamk_order): first one lane per (reference point, group of 64 points) asks the group's box (group_keep), then a wave
 * runs the per-pair test for the reference points its group is live for, and loads nothing for a group that no
 * reference point is live for (bench scene: 0.99 -> 0.71 ms).
 * grid (ceil(n_launch / COUNT_REFS), ceil(S / KEY_TILE)). */
__global__ __launch_bounds__(256) void k_scene_count(oslamk_vote_args a)
{
    __shared__ uint32_t s_cnt[COUNT_REFS];
    __shared__ uint32_t s_reach[OSLAMK_REACH_BINS / 32];
    __shared__ uint32_t s_live[KEY_TILE / WAVE];          /* [grp] bit g: the tile's group grp may hold a pair of reference point g */
    const int S = a.scene.n, lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * COUNT_REFS;
    const uint32_t reach_words = a.table.reach_words;
    KeyRefs r;
    uint32_t cnt[COUNT_REFS] = {0};
    key_refs_load(r, a, g0);
    if (threadIdx.x < COUNT_REFS) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < KEY_TILE / WAVE) s_live[threadIdx.x] = 0;
    reach_fill(s_reach, a.table.reach, reach_words);
    __syncthreads();
    /* the tile's KEY_TILE / 64 = 64 groups against the 8 reference points: a wave takes two reference points, a lane a group */
#pragma unroll
    for (int h = 0; h < COUNT_REFS / 4; h++) {
        const int g = wave + 4 * h;
        if (group_keep(a, g0 + g, blockIdx.y * (KEY_TILE / WAVE) + lane, s_reach, reach_words)) atomicOr(&s_live[lane], 1u << g);
    }
    __syncthreads();
    for (int c = 0; c < KEY_TILE / 256; c++) {
        const uint32_t live = uni_u32(s_live[c * 4 + wave]);           /* of the group of this wave's 64 points */
        if (!live) continue;
        const int si = blockIdx.y * KEY_TILE + c * 256 + threadIdx.x;
        const bool in = si < S;
        const float x = in ? a.order.sx[si] : 0.0f, y = in ? a.order.sy[si] : 0.0f, z = in ? a.order.sz[si] : 0.0f;
        const int i = in ? (int)a.order.perm[si] : -1;
#pragma unroll
        for (int g = 0; g < COUNT_REFS; g++) {
            if (!((live >> g) & 1u)) continue;
            cnt[g] += (uint32_t)__popcll(__ballot(pair_keep(r, g, true, i, in, x, y, z, a, s_reach, reach_words)));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < COUNT_REFS; g++)
            if (cnt[g]) atomicAdd(&s_cnt[g], cnt[g]);
    }
    __syncthreads();
    if (threadIdx.x < COUNT_REFS && g0 + (int)threadIdx.x < a.n_launch && s_cnt[threadIdx.x])
        atomicAdd(&a.keep_count[g0 + threadIdx.x], s_cnt[threadIdx.x]);
}

/* Phase 2 of k_scene_hits for one wave: up to 64 pairs (reference point ref_local of the batch, point
 * at place tile0 + list[j0 + lane] of the scene's Morton order) that are within reach.  The pair's quantised feature as bins (pc_pair_bins: the
 * reference's operations up to each acosf argument, then the tabulated steps), the slot of its key in the
 * union table from table.kmap -- one load instead of the hash and a probe sequence -- and for a pair that
 * hits, theta_v; the hits are appended to the reference point's list, one atomic per wave for the places. */
__device__ __forceinline__ void hits_chunk(const oslamk_vote_args &a, int ref_local, int tile0, const uint16_t *list,
                                           uint32_t j0, uint32_t n, const uint32_t *lut, int lane)
{
    const int ref_ord = a.first_ref + ref_local;
    const uint32_t r = a.ref_idx[ref_ord];
    const float prx = a.scene.px[r], pry = a.scene.py[r], prz = a.scene.pz[r];
    const float nrx = a.scene.nx[r], nry = a.scene.ny[r], nrz = a.scene.nz[r];
    const float nrn = pc_norm3(nrx, nry, nrz);
    const float *rows = a.tsg + 8 * (size_t)ref_ord;
    const uint32_t j = j0 + (uint32_t)lane;
    bool hit = false;
    uint32_t slot = 0;
    oslamk_pay pay;
    pay.theta_t22 = 0;
    pay.idx = 0;
    if (j < n) {
        const int si = tile0 + (int)list[j];
        const int i = (int)a.order.perm[si];
        const float x = a.order.sx[si], y = a.order.sy[si], z = a.order.sz[si];
        const float nx = a.scene.nx[i], ny = a.scene.ny[i], nz = a.scene.nz[i];
        const float nn = pc_norm3(nx, ny, nz);
        uint32_t combo;
        const int k1 = pc_pair_bins(prx, pry, prz, nrx, nry, nrz, nrn, x, y, z, nx, ny, nz, nn, a.d_dist, a.inv_d_dist, lut, &combo);
        if ((uint32_t)k1 < a.table.kmap_bins) {
            slot = a.table.kmap[(size_t)k1 * PC_ANGLE_COMBOS + combo];
            hit = slot != OSLAMK_KMAP_NONE;
        } else {
            /* a bin the map does not cover (or pc_pair_key's generic path): hash and probe */
            const uint32_t key = pc_pair_key(prx, pry, prz, nrx, nry, nrz, nrn, x, y, z, nx, ny, nz, nn, a.d_dist, a.inv_d_dist);
            if (key != 0) {                                       /* kernel.cu:491,520 */
                const uint32_t mask = a.table.ucap - 1;
                slot = oslamk_slot_of(key, a.table.ushift);
                for (uint32_t probe = 0; probe <= mask; probe++) {
                    const uint32_t k = a.table.ukeys[slot];
                    if (k == key) { hit = true; break; }
                    if (k == 0) break;
                    slot = (slot + 1) & mask;
                }
                if (hit) slot = a.table.uids[slot];                /* the key's number, as the key map gives it */
            }
        }
        if (hit) {
            const float vy = pc_row_dot(rows, x, y, z);     /* kernel.cu:334-336 */
            const float vz = pc_row_dot(rows + 4, x, y, z);
            /* fast mode: a degenerate vector counts as theta = 0 (pc_theta_fast); the members of a group that share
             * this list share the vote mode (oslam_db.c: same_group) */
            const uint32_t th = pc_angle_t22(vy, vz);
            pay.theta_t22 = a.mode == 1 ? pc_theta_fast(th) : th;
            pay.idx = (uint32_t)i;
        }
    }
    const unsigned long long hm = __ballot(hit);
    if (hm) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&a.hit_count[ref_local], (uint32_t)__popcll(hm));
        base = readlane_u(base, 0);
        /* The list has as many places as k_scene_count found pairs within reach, by the same predicate as phase 1
         * here -- checked, not assumed: a hit that would not fit is dropped and flagged, and the host turns the flag
         * into an error instead of using lists that ran into their neighbours. */
        const uint32_t cap = a.hit_off[ref_local + 1] - a.hit_off[ref_local];
        const uint32_t at = base + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
        if (hit && at < cap) {
            const size_t pos = (size_t)a.hit_off[ref_local] + at;
            a.hit_key[pos] = slot;
            a.hit_pay[pos] = pay;
        }
        if (lane == 0 && base + (uint32_t)__popcll(hm) > cap) atomicOr(&a.counters->list_overflow, 1u);
    }
}

/* The pairs (reference point, point) of COUNT_REFS reference points and one tile of HIT_TILE scene points.
 * The tile is a piece of the scene's Morton order (oslamk_order); a list entry is a place in it, which phase 2 maps
 * back to the scene's own index (order.perm) for the normals and the payload.
 * Phase 1 (cheap; a point is loaded once for the 8 reference points): the blocks (reference point, group of 64
 * points) whose box cannot hold a pair within reach are dropped by one test each (group_keep), as in k_scene_count;
 * for the pairs of the others the distance bin only; pairs
 * out of reach are dropped, the rest are compacted into one LDS list per reference point.  Phase 2 (dense
 * lanes): the waves share out the lists in chunks of 64 pairs (hits_chunk); a pair that hits is appended
 * to its reference point's hit list as {slot of the key in the union table} + {theta_v, i}.  The list of
 * a reference point has keep_count[] places (k_scene_count: the same predicate), which phase 1 cannot
 * exceed.  grid (ceil(n_launch / COUNT_REFS), ceil(S / HIT_TILE)). */
__global__ __launch_bounds__(256) void k_scene_hits(oslamk_vote_args a)
{
    __shared__ uint16_t s_list[COUNT_REFS][HIT_TILE];
    __shared__ uint32_t s_n[COUNT_REFS];
    __shared__ uint32_t s_reach[OSLAMK_REACH_BINS / 32];
    __shared__ uint32_t s_lut[2 * PC_ACOS_CELLS];
    __shared__ uint32_t s_live[HIT_TILE / WAVE];           /* [grp] bit g: the tile's group grp may hold a pair of reference point g */
    const int S = a.scene.n, lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = threadIdx.x >> 6;
    const int g0 = blockIdx.x * COUNT_REFS, tile0 = blockIdx.y * HIT_TILE;
    const uint32_t reach_words = a.table.reach_words;
    KeyRefs r;
    key_refs_load(r, a, g0);
    if (threadIdx.x < COUNT_REFS) s_n[threadIdx.x] = 0;
    if (threadIdx.x < HIT_TILE / WAVE) s_live[threadIdx.x] = 0;
    reach_fill(s_reach, a.table.reach, reach_words);
    s_lut[threadIdx.x] = d_acos_lut[threadIdx.x];
    __syncthreads();
    /* the tile's HIT_TILE / 64 = 16 groups against the 8 reference points: 128 tests, one a lane of the first two waves */
    if (threadIdx.x < COUNT_REFS * (HIT_TILE / WAVE)
        && group_keep(a, g0 + (int)(threadIdx.x >> 4), blockIdx.y * (HIT_TILE / WAVE) + (lane & 15), s_reach, reach_words))
        atomicOr(&s_live[lane & 15], 1u << (threadIdx.x >> 4));
    __syncthreads();

    for (int c = 0; c < HIT_TILE / 256; c++) {
        const int li = c * 256 + (int)threadIdx.x, si = tile0 + li;
        const uint32_t live = uni_u32(s_live[(uint32_t)c * 4u + wave]);     /* of the group of this wave's 64 points */
        if (!live) continue;
        const bool in = si < S;
        const float x = in ? a.order.sx[si] : 0.0f, y = in ? a.order.sy[si] : 0.0f, z = in ? a.order.sz[si] : 0.0f;
        const int i = in ? (int)a.order.perm[si] : -1;
#pragma unroll
        for (int g = 0; g < COUNT_REFS; g++) {
            if (!((live >> g) & 1u)) continue;
            const bool keep = pair_keep(r, g, g0 + g < a.n_launch, i, in, x, y, z, a, s_reach, reach_words);
            const unsigned long long km = __ballot(keep);
            if (km) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&s_n[g], (uint32_t)__popcll(km));
                base = readlane_u(base, 0);
                if (keep) s_list[g][base + (uint32_t)__popcll(km & ((1ull << lane) - 1ull))] = (uint16_t)li;
            }
        }
    }
    __syncthreads();

    uint32_t cc = 0;
    for (int g = 0; g < COUNT_REFS && g0 + g < a.n_launch; g++) {
        const uint32_t n_g = uni_u32(s_n[g]);
        for (uint32_t j0 = 0; j0 < n_g; j0 += WAVE, cc++)
            if ((cc & 3u) == wave) hits_chunk(a, g0 + g, tile0, &s_list[g][0], j0, n_g, s_lut, lane);
    }
}

/* --------------------------------------------------------------------------
 * launchers
 * ------------------------------------------------------------------------*/
extern "C" {

int oslamk_scene_count(const oslamk_vote_args *a, void *stream)
{
    if (a->n_launch <= 0) return 0;
    dim3 grid((unsigned)((a->n_launch + COUNT_REFS - 1) / COUNT_REFS), (unsigned)((a->scene.n + KEY_TILE - 1) / KEY_TILE));
    hipLaunchKernelGGL(k_scene_count, grid, dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

int oslamk_scene_hits(const oslamk_vote_args *a, void *stream)
{
    if (a->n_launch <= 0) return 0;
    dim3 grid((unsigned)((a->n_launch + COUNT_REFS - 1) / COUNT_REFS), (unsigned)((a->scene.n + HIT_TILE - 1) / HIT_TILE));
    hipLaunchKernelGGL(k_scene_hits, grid, dim3(256), 0, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

} /* extern "C" */
