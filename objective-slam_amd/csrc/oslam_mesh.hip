/*
 * oslam_mesh.hip -- the fused surface of a TSDF volume as a triangle mesh by marching cubes (semantics: include/oslam.h at
 * oslam_volume_mesh; host side: oslam_surface.c; table: oslam_mc_table.h, written by tools/gen_mc_table.py).  As in
 * oslam_surface.hip nothing proportional to the number of voxels is stored: the volume is read three times.  Workgroups
 * and runs are the surface extraction's (256 threads own OSLAMK_SURF_RUN consecutive voxels as chunks of 256; a wave
 * none of whose words is seen does nothing more: an unseen voxel owns no crossing and is the corner of no full cube).
 *
 *   k_mesh_count      a seen voxel counts the crossings on its three owned edges and, where it is the corner of a full
 *                     cube, the triangles of the cube's row.  Both sums go to the workgroup's two counters (waves summed in
 *                     LDS, no atomic); the full cubes with a case other than 0 and 255 are added to the totals as one integer
 *                     atomic per wave.
 *   k_surface_scan    (oslam_surface.hip, run once per counter array) turns them into exclusive offsets and totals.
 *   k_mesh_vertices   recomputes the crossings.  The rank of a vertex is k_surface_emit's (surf_chunk_rank).  It is known
 *                     before the point is, so each axis computes its point (and, with nrm, its normal) and stores it at
 *                     once: one axis at a time, no record array.  edge_id[rank] = 3 * voxel + axis, ascending by
 *                     construction.
 *   k_mesh_triangles  recomputes the case.  The rank of a cube's first triangle is a scan of the row lengths over the
 *                     chunk (block_excl_scan) plus the earlier chunks and the workgroup's offset.  For each triangle corner
 *                     the cube edge becomes the global id 3 * (start voxel) + axis and its vertex index is found by
 *                     binary search in edge_id (17 steps for 100 000 vertices, in an array that stays in L2).  The hit
 *                     must match exactly: a miss skips the store and is counted, and the host fails the call.
 * Bounds.  A voxel index is checked against nx*ny*nz before its word is loaded; the three owned neighbours are loaded
 * only where the coordinate is below n_a - 1 (surf_crossings), the four other corners of a cube only when that holds on
 * all three axes, which keeps idx + 1 + nx + nx*ny inside the volume; the table's row is indexed by an 8-bit case and a
 * triangle number below the row's length, at most OSLAM_MC_MAX_TRI; the binary search reads edge_id below n_verts only;
 * every rank is checked against its count before the store.  The launchers check the volume's sizes, the number of
 * workgroups and the counts.  No scratch, no spills (profiles/r12_kernel_resources_mesh.txt).
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "oslam_kernels.h"
#include "oslam_mc_table.h"
#include "oslam_surf_edge.h"

__device__ const uint8_t d_mc_ntri[256] = {OSLAM_MC_NTRI_FLAT};
__device__ const uint8_t d_mc_edges[256 * OSLAM_MC_ROW] = {OSLAM_MC_EDGES_FLAT};

/* the case of the cube whose corner is the seen voxel idx (ijk, w0, nb as surf_crossings left them); false when the
 * cube does not exist or is not full */
__device__ __forceinline__ bool mesh_case(const oslamk_volume &vol, uint32_t idx, uint32_t w0, uint32_t min_w, const int ijk[3],
                                          const uint32_t nb[3], uint32_t *mc_case)
{
    if (!(ijk[0] + 1 < vol.nx && ijk[1] + 1 < vol.ny && ijk[2] + 1 < vol.nz)) return false;
    const size_t sy = (size_t)vol.nx, sz = (size_t)vol.nx * vol.ny;
    const uint32_t *p = vol.words + idx;
    const uint32_t w[8] = {w0, nb[0], nb[1], p[sy + 1], nb[2], p[sz + 1], p[sz + sy], p[sz + sy + 1]};
    bool full = true;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        full &= surf_seen(w[k], min_w);
        c |= (uint32_t)surf_neg(w[k]) << k;
    }
    *mc_case = c;
    return full;
}

/* the global id 3 * (start voxel) + axis of cube edge e = 4 * axis + m of the cube at voxel idx */
__device__ __forceinline__ uint32_t mesh_edge_id(uint32_t idx, uint32_t e, uint32_t nx, uint32_t nxy)
{
    const uint32_t a = e >> 2, lo = e & 1u, hi = e >> 1 & 1u;
    const uint32_t off = a == 0 ? lo * nx + hi * nxy : a == 1 ? lo + hi * nxy : lo + hi * nx;
    return 3u * (idx + off) + a;
}

__global__ __launch_bounds__(SURF_T) void k_mesh_count(const oslamk_volume vol, uint32_t min_w, uint32_t n_vox, uint32_t *vcounts,
                                                       uint32_t *tcounts, uint32_t *totals)
{
    __shared__ uint32_t s_v[SURF_WAVES], s_t[SURF_WAVES];   /* two sums behind one barrier: wave_sum, not two block_sum */
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t w0[SURF_ITEMS], verts = 0, tris = 0, cubes = 0;
    const bool any = surf_load(vol, n_vox, min_w, w0);
    if (__ballot(any)) {
        for (int it = 0; it < SURF_ITEMS; it++) {
            if (!surf_seen(w0[it], min_w)) continue;
            const uint32_t idx = surf_idx(it);
            int ijk[3];
            uint32_t nb[3], c;
            verts += (uint32_t)__popc(surf_crossings(vol, idx, w0[it], min_w, ijk, nb));
            if (mesh_case(vol, idx, w0[it], min_w, ijk, nb, &c) && c != 0u && c != 255u) {
                cubes++;
                tris += d_mc_ntri[c];
            }
        }
        verts = wave_sum(verts);
        tris = wave_sum(tris);
        cubes = wave_sum(cubes);
    }
    if (lane == 0) {
        s_v[wave] = verts;
        s_t[wave] = tris;
        if (cubes) atomicAdd(totals + OSLAMK_MESH_T_CUBES, cubes);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sv = 0, st = 0;
#pragma unroll
        for (int w = 0; w < SURF_WAVES; w++) {
            sv += s_v[w];
            st += s_t[w];
        }
        vcounts[blockIdx.x] = sv;
        tcounts[blockIdx.x] = st;
    }
}

__global__ __launch_bounds__(SURF_T) void k_mesh_vertices(const oslamk_volume vol, uint32_t min_w, uint32_t n_vox,
                                                          const uint32_t *offsets, uint32_t n_verts, float *xyz, float *nrm,
                                                          uint32_t *edge_id)
{
    __shared__ uint32_t s_cnt[SURF_ITEMS][SURF_WAVES];
    uint32_t w0[SURF_ITEMS];
    const bool any = surf_load(vol, n_vox, min_w, w0);
    if (!__syncthreads_or(any)) return;
    const bool wave_any = __ballot(any) != 0ull;
    uint32_t run = offsets[blockIdx.x];
    for (int it = 0; it < SURF_ITEMS; it++) {
        const uint32_t idx = surf_idx(it);
        int ijk[3] = {0, 0, 0};
        uint32_t nb[3] = {0u, 0u, 0u}, mask = 0, all;
        if (wave_any && surf_seen(w0[it], min_w)) mask = surf_crossings(vol, idx, w0[it], min_w, ijk, nb);
        uint32_t rank = run + surf_chunk_rank(mask, s_cnt[it], &all);
        /* one axis at a time, as in k_surface_emit: the six reads of three normals at once cost 200 registers */
#pragma unroll 1
        for (int a = 0; a < 3; a++) {
            if (!(mask >> a & 1u)) continue;
            if (rank < n_verts) {
                float P[3], n[3] = {0.0f, 0.0f, 0.0f};
                surf_position(vol, ijk, a, w0[it], surf_pick(nb, a), P);
                xyz[(size_t)rank * 3] = P[0];
                xyz[(size_t)rank * 3 + 1] = P[1];
                xyz[(size_t)rank * 3 + 2] = P[2];
                if (nrm) {
                    if (!surf_normal(vol, P, n)) n[0] = n[1] = n[2] = 0.0f;
                    nrm[(size_t)rank * 3] = n[0];
                    nrm[(size_t)rank * 3 + 1] = n[1];
                    nrm[(size_t)rank * 3 + 2] = n[2];
                }
                edge_id[rank] = 3u * idx + (uint32_t)a;
            }
            rank++;
        }
        run += all;
    }
}

/* the index of id in the ascending edge_id [n]; n when it is not there */
__device__ __forceinline__ uint32_t mesh_find(const uint32_t *edge_id, uint32_t n, uint32_t id)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (edge_id[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && edge_id[lo] == id ? lo : n;
}

__global__ __launch_bounds__(SURF_T) void k_mesh_triangles(const oslamk_volume vol, uint32_t min_w, uint32_t n_vox,
                                                           const uint32_t *offsets, uint32_t n_tris, const uint32_t *edge_id,
                                                           uint32_t n_verts, uint32_t *tri, uint32_t *totals)
{
    __shared__ uint32_t s_cnt[SURF_ITEMS][SURF_WAVES];
    const uint32_t nx = (uint32_t)vol.nx, nxy = (uint32_t)vol.nx * (uint32_t)vol.ny;
    uint32_t w0[SURF_ITEMS], missed = 0;
    const bool any = surf_load(vol, n_vox, min_w, w0);
    if (!__syncthreads_or(any)) return;
    const bool wave_any = __ballot(any) != 0ull;
    uint32_t run = offsets[blockIdx.x];
    for (int it = 0; it < SURF_ITEMS; it++) {
        const uint32_t idx = surf_idx(it);
        uint32_t c = 0, nt = 0, all;
        if (wave_any && surf_seen(w0[it], min_w)) {
            int ijk[3];
            uint32_t nb[3];
            (void)surf_crossings(vol, idx, w0[it], min_w, ijk, nb);
            if (mesh_case(vol, idx, w0[it], min_w, ijk, nb, &c)) nt = d_mc_ntri[c];
        }
        uint32_t rank = run + block_excl_scan<SURF_WAVES>(nt, s_cnt[it], &all);    /* over the cubes' row lengths */
        const uint8_t *row = d_mc_edges + c * OSLAM_MC_ROW;     /* c <= 255 */
        for (uint32_t t = 0; t < nt; t++, rank++) {             /* nt <= OSLAM_MC_MAX_TRI */
            uint32_t v[3];
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = mesh_find(edge_id, n_verts, mesh_edge_id(idx, row[3 * t + k], nx, nxy));
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

extern "C" int oslamk_mesh_count(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, uint32_t *vcounts,
                                 uint32_t *tcounts, uint32_t *totals, void *stream)
{
    uint32_t n_vox;
    hipError_t e;
    int rc;
    if (!surf_launch_ok(vol, min_weight, n_groups, &n_vox) || !vcounts || !tcounts || !totals) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_count, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, vcounts, tcounts,
                       totals);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    rc = oslamk_surface_scan(vcounts, n_groups, totals + OSLAMK_MESH_T_VERTS, stream);
    if (rc != 0) return rc;
    return oslamk_surface_scan(tcounts, n_groups, totals + OSLAMK_MESH_T_TRIS, stream);
}

extern "C" int oslamk_mesh_vertices(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, const uint32_t *voffsets,
                                    uint32_t n_verts, float *xyz, float *nrm, uint32_t *edge_id, void *stream)
{
    uint32_t n_vox;
    if (!surf_launch_ok(vol, min_weight, n_groups, &n_vox) || !voffsets || !xyz || !edge_id || n_verts == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_vertices, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, voffsets,
                       n_verts, xyz, nrm, edge_id);
    return (int)hipGetLastError();
}

extern "C" int oslamk_mesh_triangles(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, const uint32_t *toffsets,
                                     uint32_t n_tris, const uint32_t *edge_id, uint32_t n_verts, uint32_t *tri, uint32_t *totals,
                                     void *stream)
{
    uint32_t n_vox;
    if (!surf_launch_ok(vol, min_weight, n_groups, &n_vox) || !toffsets || !edge_id || !tri || !totals || n_tris == 0 || n_verts == 0)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_triangles, dim3(n_groups), dim3(SURF_T), 0, (hipStream_t)stream, *vol, min_weight, n_vox, toffsets,
                       n_tris, edge_id, n_verts, tri, totals);
    return (int)hipGetLastError();
}
