/*
 * oslam_world_mesh.hip -- the marching-cubes mesh of the whole map, voxel store plus window, extracted from sparse
 * 8 x 8 x 8 bricks with no dense box anywhere (semantics: include/oslam.h at oslam_world_mesh; host side:
 * oslam_world_mesh.c; the table, the tile, the trilinear read and the point of a crossing: oslam_brick.h; the "seen"
 * rule, the sign test and the rank of a crossing in its chunk: oslam_surf_edge.h; the cases: oslam_mc_table.h).  The map
 * on the device is oslam_world_surface.hip's, window written in by its k_brick_window.  Every kernel has that file's
 * shape: one workgroup of 256 threads per table entry, two voxels per thread, own words loaded first; a workgroup none
 * of whose words is seen leaves at once, because a crossing's start voxel and a cube's corner voxel must both be seen.
 * The others find their 27 slots and load the 12 x 12 x 12 tile; the eight corners of a cube lie at local + (0|1),
 * inside the tile, so no cube read goes through the table.
 *
 *   k_wmesh_count      per entry the crossings (all of them, with or without a normal) to vcounts[e] and the triangles of
 *                      its full cubes to tcounts[e]; a workgroup that leaves early stores a zero for both.  The full cubes
 *                      with a case other than 0 and 255 go to the totals as one integer atomic per wave.  Both arrays
 *                      are scanned by oslamk_surface_scan in chunks of 2^17 entries; the host forms the chunks' bases.
 *   k_wmesh_vertices   recomputes the crossings.  The rank of a vertex is surf_chunk_rank's over the crossing masks (voxel
 *                      order, then axis) plus the first chunk's, the entry's offset and its scan chunk's base.  One axis
 *                      at a time: position, then (with nrm) the six trilinear reads; a crossing without a normal gets
 *                      zeros.  edge_id[rank] = 3 * local + axis, ascending inside its entry.
 *   k_wmesh_triangles  recomputes the case from the tile.  The rank of a cube's first triangle is a scan of the row lengths
 *                      (block_excl_scan).  A corner's edge belongs to voxel local + EDGE_START, in this brick or in one of
 *                      its seven +x/+y/+z neighbours: eight lanes find those entries and the runs [start, end) of their
 *                      vertices (end = the next entry's start, across a scan chunk's boundary too, or the total at the
 *                      last entry); the vertex is found by binary search of 3 * local + axis in that run, at most 1536
 *                      ids, 11 steps.  A miss skips the store and is counted, and the host fails the call.
 * Bounds.  A table index is below n by the grid and checked again; a slot and an entry index are checked against n before
 * any access through them; a tile index is checked against the tile before every LDS read; the case is 8 bits and a
 * triangle number is below the row's length, at most OSLAM_MC_MAX_TRI; a run is checked to lie inside the vertices and to
 * hold at most 1536 of them, and the search reads inside it only; every rank is checked against its total before a
 * store.  The launchers check the map, the "seen" weight, the anchor, the counts and the pointers.  No scratch, no float
 * atomics; registers, LDS and occupancy: profiles/r27_kernel_resources_world_mesh.txt.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_brick.h"
#include "oslam_kernels.h"
#include "oslam_mc_table.h"
#include "oslam_surf_edge.h"

#define WM_RUN_MAX (3u * OSLAMK_BRICK_WORDS)          /* the most vertices of one entry */

static __device__ const uint8_t d_wm_ntri[256] = {OSLAM_MC_NTRI_FLAT};
static __device__ const uint8_t d_wm_edges[256 * OSLAM_MC_ROW] = {OSLAM_MC_EDGES_FLAT};

/* a thread's own words of entry e (slot *own, BRK_NONE without a brick: zeros); true when one of them is seen */
__device__ __forceinline__ bool wm_own_words(const oslamk_brick_map &m, uint32_t e, uint32_t min_w, uint32_t *own, uint32_t w0[BRK_ITEMS])
{
    bool any = false;
    *own = m.slots[e] < m.n ? m.slots[e] : BRK_NONE;
#pragma unroll
    for (int it = 0; it < BRK_ITEMS; it++) {
        w0[it] = *own != BRK_NONE ? m.words[(size_t)*own * OSLAMK_BRICK_WORDS + (uint32_t)it * BRK_T + threadIdx.x] : 0u;
        any |= surf_seen(w0[it], min_w);
    }
    return any;
}

/* the tile index of the brick's voxel l */
__device__ __forceinline__ uint32_t wm_tile_index(uint32_t l)
{
    return (((l >> 6) + BRK_HALO) * BRK_TILE + (l >> 3 & 7u) + BRK_HALO) * BRK_TILE + (l & 7u) + BRK_HALO;
}

/* the crossings of the seen voxel at tile index p (word w0) as a mask of axes; nb[a] = the +a neighbour's word */
__device__ __forceinline__ uint32_t wm_crossings(const uint32_t *tile, uint32_t p, uint32_t w0, uint32_t min_w, uint32_t nb[3])
{
    const uint32_t stride[3] = {1u, BRK_TILE, BRK_TILE * BRK_TILE};
    uint32_t mask = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        nb[a] = tile_at(tile, p + stride[a]);
        if (surf_seen(nb[a], min_w) && surf_neg(w0) != surf_neg(nb[a])) mask |= 1u << a;
    }
    return mask;
}

/* the case of the cube whose corner is the voxel at tile index p; false when the cube is not full */
__device__ __forceinline__ bool wm_case(const uint32_t *tile, uint32_t p, uint32_t min_w, uint32_t *mc_case)
{
    bool full = true;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
        const uint32_t w = tile_at(tile, p + (k & 1u) + (k >> 1 & 1u) * BRK_TILE + (k >> 2) * (BRK_TILE * BRK_TILE));
        full &= surf_seen(w, min_w);
        c |= (uint32_t)surf_neg(w) << k;
    }
    *mc_case = c;
    return full;
}

__global__ __launch_bounds__(BRK_T) void k_wmesh_count(const oslamk_brick_map m, uint32_t min_w, uint32_t *vcounts, uint32_t *tcounts,
                                                       uint32_t *totals)
{
    __shared__ uint32_t s_tile[BRK_TILE_WORDS];
    __shared__ uint32_t s_nb[27];
    __shared__ uint32_t s_v[SURF_WAVES], s_t[SURF_WAVES];
    const uint32_t e = blockIdx.x, tid = threadIdx.x;
    if (e >= m.n) return;
    uint32_t own, w0[BRK_ITEMS];
    if (!__syncthreads_or(wm_own_words(m, e, min_w, &own, w0))) {
        if (tid == 0) {
            vcounts[e] = 0u;
            tcounts[e] = 0u;
        }
        return;
    }
    int kb[3];
    brick_coords(m.keys[e], kb);
    BRICK_TILE_LOAD(m, kb, own, tid, s_nb, s_tile);
    uint32_t verts = 0, tris = 0, cubes = 0;
#pragma unroll
    for (int it = 0; it < BRK_ITEMS; it++) {
        if (!surf_seen(w0[it], min_w)) continue;
        const uint32_t p = wm_tile_index((uint32_t)it * BRK_T + tid);
        uint32_t nb[3], c;
        verts += (uint32_t)__popc(wm_crossings(s_tile, p, w0[it], min_w, nb));
        if (wm_case(s_tile, p, min_w, &c) && c != 0u && c != 255u) {
            cubes++;
            tris += d_wm_ntri[c];
        }
    }
    verts = wave_sum(verts);
    tris = wave_sum(tris);
    cubes = wave_sum(cubes);
    if ((tid & 63u) == 0) {
        s_v[tid >> 6] = verts;
        s_t[tid >> 6] = tris;
        if (cubes) atomicAdd(totals + OSLAMK_MESH_T_CUBES, cubes);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t sv = 0, st = 0;
#pragma unroll
        for (int w = 0; w < SURF_WAVES; w++) {
            sv += s_v[w];
            st += s_t[w];
        }
        vcounts[e] = sv;
        tcounts[e] = st;
    }
}

__global__ __launch_bounds__(BRK_T) void k_wmesh_vertices(const oslamk_brick_map m, uint32_t min_w, const uint32_t *voffsets,
                                                          const oslamk_brick_bases vbases, uint32_t n_verts, float *xyz, float *nrm,
                                                          int32_t *key_out, uint32_t *edge_id)
{
    __shared__ uint32_t s_tile[BRK_TILE_WORDS];
    __shared__ uint32_t s_nb[27];
    __shared__ uint32_t s_cnt[BRK_ITEMS][SURF_WAVES];
    const uint32_t e = blockIdx.x, tid = threadIdx.x;
    if (e >= m.n) return;
    uint32_t own, w0[BRK_ITEMS];
    if (!__syncthreads_or(wm_own_words(m, e, min_w, &own, w0))) return;
    int kb[3];
    brick_coords(m.keys[e], kb);
    BRICK_TILE_LOAD(m, kb, own, tid, s_nb, s_tile);
    const int g0[3] = {kb[0] * OSLAMK_BRICK_SIDE, kb[1] * OSLAMK_BRICK_SIDE, kb[2] * OSLAMK_BRICK_SIDE};
    const int tg[3] = {g0[0] - BRK_HALO, g0[1] - BRK_HALO, g0[2] - BRK_HALO};
    uint32_t run = voffsets[e] + vbases.base[e / OSLAMK_BRICK_SCAN % OSLAMK_BRICK_CHUNKS];
    for (int it = 0; it < BRK_ITEMS; it++) {
        const uint32_t l = (uint32_t)it * BRK_T + tid;
        const int g[3] = {g0[0] + (int)(l & 7u), g0[1] + (int)(l >> 3 & 7u), g0[2] + (int)(l >> 6)};
        const int r[3] = {g[0] - m.anchor[0], g[1] - m.anchor[1], g[2] - m.anchor[2]};
        uint32_t nb[3] = {0u, 0u, 0u}, mask = 0, all;
        if (surf_seen(w0[it], min_w)) mask = wm_crossings(s_tile, wm_tile_index(l), w0[it], min_w, nb);
        uint32_t rank = run + surf_chunk_rank(mask, s_cnt[it], &all);
        /* one axis at a time, as in k_mesh_vertices: the six reads of three normals at once cost too many registers */
#pragma unroll 1
        for (int a = 0; a < 3; a++) {
            if (!(mask >> a & 1u)) continue;
            if (rank < n_verts) {
                float P[3], n[3] = {0.0f, 0.0f, 0.0f};
                brick_position(m, r, a, w0[it], surf_pick(nb, a), P);
                xyz[(size_t)rank * 3] = P[0];
                xyz[(size_t)rank * 3 + 1] = P[1];
                xyz[(size_t)rank * 3 + 2] = P[2];
                if (nrm) {
                    if (!brick_normal(m, s_tile, tg, P, n)) n[0] = n[1] = n[2] = 0.0f;
                    nrm[(size_t)rank * 3] = n[0];
                    nrm[(size_t)rank * 3 + 1] = n[1];
                    nrm[(size_t)rank * 3 + 2] = n[2];
                }
                if (key_out) reinterpret_cast<int4 *>(key_out)[rank] = make_int4(g[0], g[1], g[2], a);
                edge_id[rank] = 3u * l + (uint32_t)a;
            }
            rank++;
        }
        run += all;
    }
}

/* the index of id in the ascending edge_id [lo, hi), hi <= n; n when it is not there */
__device__ __forceinline__ uint32_t wm_find(const uint32_t *edge_id, uint32_t lo, uint32_t hi, uint32_t n, uint32_t id)
{
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (edge_id[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < end && edge_id[lo] == id ? lo : n;
}

__global__ __launch_bounds__(BRK_T) void k_wmesh_triangles(const oslamk_brick_map m, uint32_t min_w, const uint32_t *toffsets,
                                                           const oslamk_brick_bases tbases, uint32_t n_tris, const uint32_t *voffsets,
                                                           const oslamk_brick_bases vbases, const uint32_t *edge_id, uint32_t n_verts,
                                                           uint32_t *tri, uint32_t *totals)
{
    __shared__ uint32_t s_tile[BRK_TILE_WORDS];
    __shared__ uint32_t s_nb[27];
    __shared__ uint32_t s_cnt[BRK_ITEMS][SURF_WAVES];
    __shared__ uint32_t s_lo[8], s_hi[8];               /* the vertex runs of this entry and its seven + neighbours */
    const uint32_t e = blockIdx.x, tid = threadIdx.x;
    if (e >= m.n) return;
    uint32_t own, w0[BRK_ITEMS];
    if (!__syncthreads_or(wm_own_words(m, e, min_w, &own, w0))) return;
    int kb[3];
    brick_coords(m.keys[e], kb);
    if (tid >= 64u && tid < 72u) {                      /* the second wave, while 27 lanes of the first find the slots */
        const uint32_t j = tid - 64u;
        const uint32_t ent = j == 0u ? e : brick_find_entry(m, OSLAMK_BRICK_KEY(kb[0] + (int)(j & 1u), kb[1] + (int)(j >> 1 & 1u), kb[2] + (int)(j >> 2)));
        uint32_t lo = 0, hi = 0;
        if (ent < m.n) {
            lo = voffsets[ent] + vbases.base[ent / OSLAMK_BRICK_SCAN % OSLAMK_BRICK_CHUNKS];
            hi = ent + 1u < m.n ? voffsets[ent + 1u] + vbases.base[(ent + 1u) / OSLAMK_BRICK_SCAN % OSLAMK_BRICK_CHUNKS] : n_verts;
            if (!(lo <= hi && hi <= n_verts && hi - lo <= WM_RUN_MAX)) lo = hi = 0;
        }
        s_lo[j] = lo;
        s_hi[j] = hi;
    }
    BRICK_TILE_LOAD(m, kb, own, tid, s_nb, s_tile);
    uint32_t run = toffsets[e] + tbases.base[e / OSLAMK_BRICK_SCAN % OSLAMK_BRICK_CHUNKS], missed = 0;
    for (int it = 0; it < BRK_ITEMS; it++) {
        const uint32_t l = (uint32_t)it * BRK_T + tid;
        const uint32_t ijk[3] = {l & 7u, l >> 3 & 7u, l >> 6};
        uint32_t c = 0, nt = 0, all;
        if (surf_seen(w0[it], min_w) && wm_case(s_tile, wm_tile_index(l), min_w, &c)) nt = d_wm_ntri[c];
        uint32_t rank = run + block_excl_scan<SURF_WAVES>(nt, s_cnt[it], &all);        /* over the cubes' row lengths */
        const uint8_t *row = d_wm_edges + c * OSLAM_MC_ROW;     /* c <= 255 */
        for (uint32_t t = 0; t < nt; t++, rank++) {             /* nt <= OSLAM_MC_MAX_TRI */
            uint32_t v[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                /* cube edge 4 * a + m starts at the corner voxel plus m's two offsets on the other axes, each 0 or 1 */
                const uint32_t ed = row[3 * t + k], a = ed >> 2, o0 = ed & 1u, o1 = ed >> 1 & 1u;
                const uint32_t sx = ijk[0] + (a == 0u ? 0u : o0), sy = ijk[1] + (a == 0u ? o0 : a == 1u ? 0u : o1), sz = ijk[2] + (a == 2u ? 0u : o1);
                const uint32_t j = (sx >> 3) + 2u * (sy >> 3) + 4u * (sz >> 3);          /* s in 0 .. 8: j in 0 .. 7 */
                v[k] = wm_find(edge_id, s_lo[j & 7u], s_hi[j & 7u], n_verts, 3u * brick_local((int)sx, (int)sy, (int)sz) + a);
            }
            if (v[0] >= n_verts || v[1] >= n_verts || v[2] >= n_verts) {
                missed++;
                continue;
            }
            if (rank < n_tris) {
                tri[(size_t)rank * 3] = v[0];
                tri[(size_t)rank * 3 + 1] = v[1];
                tri[(size_t)rank * 3 + 2] = v[2];
            }
        }
        run += all;
    }
    if (missed) atomicAdd(totals + OSLAMK_MESH_T_MISS, missed);
}

static bool wm_launch_ok(const oslamk_brick_map *map, uint32_t min_weight) { return brick_map_ok(map) && min_weight >= 1u && min_weight <= 65535u; }

extern "C" int oslamk_brick_mesh_count(const oslamk_brick_map *map, uint32_t min_weight, uint32_t *vcounts, uint32_t *tcounts,
                                       uint32_t *totals, uint32_t *vsums, uint32_t *tsums, void *stream)
{
    if (!wm_launch_ok(map, min_weight) || !vcounts || !tcounts || !totals || !vsums || !tsums) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wmesh_count, dim3(map->n), dim3(BRK_T), 0, (hipStream_t)stream, *map, min_weight, vcounts, tcounts, totals);
    hipError_t e = hipGetLastError();
    for (uint32_t c = 0; e == hipSuccess && c * OSLAMK_BRICK_SCAN < map->n; c++) {
        const uint32_t left = map->n - c * OSLAMK_BRICK_SCAN, len = left < OSLAMK_BRICK_SCAN ? left : OSLAMK_BRICK_SCAN;
        e = (hipError_t)oslamk_surface_scan(vcounts + (size_t)c * OSLAMK_BRICK_SCAN, len, vsums + c, stream);
        if (e == hipSuccess) e = (hipError_t)oslamk_surface_scan(tcounts + (size_t)c * OSLAMK_BRICK_SCAN, len, tsums + c, stream);
    }
    return (int)e;
}

extern "C" int oslamk_brick_mesh_vertices(const oslamk_brick_map *map, uint32_t min_weight, const uint32_t *voffsets,
                                          const oslamk_brick_bases *vbases, uint32_t n_verts, float *xyz, float *nrm, int32_t *key_out,
                                          uint32_t *edge_id, void *stream)
{
    if (!wm_launch_ok(map, min_weight) || !voffsets || !vbases || !xyz || !edge_id || n_verts == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wmesh_vertices, dim3(map->n), dim3(BRK_T), 0, (hipStream_t)stream, *map, min_weight, voffsets, *vbases, n_verts,
                       xyz, nrm, key_out, edge_id);
    return (int)hipGetLastError();
}

extern "C" int oslamk_brick_mesh_triangles(const oslamk_brick_map *map, uint32_t min_weight, const uint32_t *toffsets,
                                           const oslamk_brick_bases *tbases, uint32_t n_tris, const uint32_t *voffsets,
                                           const oslamk_brick_bases *vbases, const uint32_t *edge_id, uint32_t n_verts, uint32_t *tri,
                                           uint32_t *totals, void *stream)
{
    if (!wm_launch_ok(map, min_weight) || !toffsets || !tbases || !voffsets || !vbases || !edge_id || !tri || !totals || n_tris == 0 ||
        n_verts == 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wmesh_triangles, dim3(map->n), dim3(BRK_T), 0, (hipStream_t)stream, *map, min_weight, toffsets, *tbases, n_tris,
                       voffsets, *vbases, edge_id, n_verts, tri, totals);
    return (int)hipGetLastError();
}
