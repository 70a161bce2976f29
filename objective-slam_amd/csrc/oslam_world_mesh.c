/*
 * oslam_world_mesh.c -- the marching-cubes mesh of the whole map, voxel store plus window (include/oslam.h at
 * oslam_world_mesh): the host side of the kernels in oslam_world_mesh.hip.  The map on the device is the one the surface
 * of the whole map extracts from (oslam_world_map_open in oslam_world_surface.c).  A call counts, waits for the chunks'
 * sums, forms the chunks' bases and the two totals in 64 bits, allocates exactly that and lets the device write the
 * vertices and then the triangles, under the volume lock and the store's.
 */
#include "oslam_internal.h"
#include "oslam_world.h"

#define WM_VSUMS 64                                      /* words of the counter block: 64 totals, the chunks' vertex sums, */
#define WM_TSUMS (WM_VSUMS + OSLAMK_BRICK_CHUNKS)        /* their triangle sums, */
#define WM_COUNTS (WM_TSUMS + OSLAMK_BRICK_CHUNKS)       /* then the entries' vertex counts [n] and triangle counts [n] */

int oslam_world_mesh(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, float *xyz_out, float *nrm_out,
                     int32_t *key_out, size_t v_cap, uint32_t *tri_out, size_t t_cap, size_t *nv_out, size_t *nt_out,
                     oslam_world_mesh_result *res)
{
    int rc, launched = 0;
    const double t0 = now_ms();
    oslam_world_surface_params p;
    oslam_world_map wm;
    oslamk_brick_bases vbases, tbases;
    uint32_t *d_cnt = NULL, *d_eid = NULL, *d_tri = NULL, tot[WM_COUNTS], launches = 0, miss = 0;
    float *d_xyz = NULL, *d_nrm = NULL;
    int32_t *d_key = NULL;
    uint64_t nv64 = 0, nt64 = 0;
    size_t n, c, chunks;
    void *stream = oslam_stream();
    if (!w || !nv_out || !nt_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!xyz_out != !tri_out) return fail(OSLAM_E_INVALID, "xyz_out and tri_out must both be given or both be NULL");
    if (!xyz_out && (v_cap != 0 || t_cap != 0 || nrm_out || key_out))
        return fail(OSLAM_E_INVALID, "v_cap and t_cap must be 0 and nrm_out and key_out NULL without outputs");
    rc = oslam_world_surface_check_params(sp, &p);
    if (rc != OSLAM_OK) return rc;
    *nv_out = *nt_out = 0;
    if (res) memset(res, 0, sizeof *res);
    memset(&wm, 0, sizeof wm);
    memset(&vbases, 0, sizeof vbases);
    memset(&tbases, 0, sizeof tbases);
    memset(tot, 0, sizeof tot);
    oslam_volume_lock();
    oslam_world_lock(w);
    rc = oslam_world_map_open(w, vol, &p, OSLAM_MAP_TSDF, stream, &wm);
    launches = wm.launches;
    n = wm.bricks;
    if (rc != OSLAM_OK || n == 0) goto done;                        /* an empty map: zero counts, no device call */
    launched = 1;
    chunks = (n + OSLAMK_BRICK_SCAN - 1) / OSLAMK_BRICK_SCAN;
    KCHK(oslam_counters_open(&d_cnt, WM_COUNTS - 64 + 2 * n, stream));
    KCHK(oslamk_brick_mesh_count(&wm.m, p.min_weight, d_cnt + WM_COUNTS, d_cnt + WM_COUNTS + n, d_cnt, d_cnt + WM_VSUMS, d_cnt + WM_TSUMS,
                                 stream));
    launches += 1 + 2 * (uint32_t)chunks;
    HIPCHK(hipMemcpyAsync(tot, d_cnt, sizeof tot, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    for (c = 0; c < chunks; c++) {                                  /* the sums before a chunk fit uint32 whenever the totals do */
        vbases.base[c] = (uint32_t)nv64;
        tbases.base[c] = (uint32_t)nt64;
        nv64 += tot[WM_VSUMS + c];
        nt64 += tot[WM_TSUMS + c];
    }
    *nv_out = (size_t)nv64;
    *nt_out = (size_t)nt64;
    if (nv64 > UINT32_MAX || nt64 > UINT32_MAX) { rc = fail(OSLAM_E_LIMIT, "the map's mesh has more than 2^32 vertices or triangles"); goto done; }
    if (xyz_out && ((size_t)nv64 > v_cap || (size_t)nt64 > t_cap)) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    if (xyz_out && nv64 > 0) {
        const uint32_t nv = (uint32_t)nv64, nt = (uint32_t)nt64;
        KCHK(oslam_dev_alloc((void **)&d_xyz, sizeof(float) * 3 * (size_t)nv));
        if (nrm_out) KCHK(oslam_dev_alloc((void **)&d_nrm, sizeof(float) * 3 * (size_t)nv));
        if (key_out) KCHK(oslam_dev_alloc((void **)&d_key, sizeof(int32_t) * 4 * (size_t)nv));
        KCHK(oslam_dev_alloc((void **)&d_eid, sizeof(uint32_t) * (size_t)nv));
        KCHK(oslamk_brick_mesh_vertices(&wm.m, p.min_weight, d_cnt + WM_COUNTS, &vbases, nv, d_xyz, d_nrm, d_key, d_eid, stream));
        launches++;
        if (nt > 0) {
            KCHK(oslam_dev_alloc((void **)&d_tri, sizeof(uint32_t) * 3 * (size_t)nt));
            KCHK(oslamk_brick_mesh_triangles(&wm.m, p.min_weight, d_cnt + WM_COUNTS + n, &tbases, nt, d_cnt + WM_COUNTS, &vbases, d_eid, nv,
                                             d_tri, d_cnt, stream));
            launches++;
        }
        HIPCHK(hipMemcpyAsync(&miss, d_cnt + OSLAMK_MESH_T_MISS, sizeof miss, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        if (miss) { rc = fail(OSLAM_E_DEVICE, "a triangle corner found no vertex on its edge: the mesh was not written"); goto done; }
        HIPCHK(hipMemcpy(xyz_out, d_xyz, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost));
        if (nrm_out) HIPCHK(hipMemcpy(nrm_out, d_nrm, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost));
        if (key_out) HIPCHK(hipMemcpy(key_out, d_key, sizeof(int32_t) * 4 * (size_t)nv, hipMemcpyDeviceToHost));
        if (nt > 0) HIPCHK(hipMemcpy(tri_out, d_tri, sizeof(uint32_t) * 3 * (size_t)nt, hipMemcpyDeviceToHost));
    }
done:
    if (rc != OSLAM_OK && rc != OSLAM_E_LIMIT && launched) (void)hipStreamSynchronize((hipStream_t)stream);
    oslam_world_unlock(w);
    oslam_volume_unlock();
    if (d_tri) oslam_dev_free(d_tri);
    if (d_eid) oslam_dev_free(d_eid);
    if (d_key) oslam_dev_free(d_key);
    if (d_nrm) oslam_dev_free(d_nrm);
    if (d_xyz) oslam_dev_free(d_xyz);
    if (d_cnt) oslam_dev_free(d_cnt);
    oslam_world_map_close(&wm);
    if ((rc == OSLAM_OK || rc == OSLAM_E_LIMIT) && res) {
        res->vertices = nv64 > UINT32_MAX ? UINT32_MAX : (uint32_t)nv64;       /* a total beyond uint32 is reported as its limit */
        res->triangles = nt64 > UINT32_MAX ? UINT32_MAX : (uint32_t)nt64;
        res->cubes = tot[OSLAMK_MESH_T_CUBES];
        res->bricks = wm.bricks;
        res->window_bricks = wm.window_bricks;
        res->launches = launches;
        memcpy(res->anchor, wm.anchor, sizeof wm.anchor);
        res->ms_total = (float)(now_ms() - t0);
    }
    return rc;
}
