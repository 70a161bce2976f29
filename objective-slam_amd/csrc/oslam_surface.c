/*
 * oslam_surface.c -- the fused surface of a TSDF volume as a cloud (include/oslam.h at oslam_volume_surface) and as a
 * triangle mesh (oslam_volume_mesh): the host side of the kernels in oslam_surface.hip and oslam_mesh.hip, and of the
 * extraction of what a shift loses (oslam_volume_leaving; the same launchers of oslam_surface.hip with a shift; the shift
 * itself is oslam_window.c).  A call counts, waits for the totals, allocates exactly that and emits, under the volume
 * lock of oslam_volume.c.
 */
#include "oslam_internal.h"
#include "oslam_mc_table.h"

/* ---- the fused surface as a cloud (include/oslam.h at oslam_volume_surface; kernels: oslam_surface.hip) ---- */
int oslam_surface_params_default(oslam_surface_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->min_weight = 1;
    return OSLAM_OK;
}

int oslam_surface_check_params(const oslam_surface_params *sp, oslam_surface_params *out)
{
    if (sp) *out = *sp; else oslam_surface_params_default(out);
    if (out->min_weight < 1 || out->min_weight > 65535) return fail(OSLAM_E_INVALID, "min_weight must lie in 1..65535");
    return OSLAM_OK;
}

/* the two passes, with the volume lock held and the volume's device bound.  shift NULL: the whole surface, otherwise the part a
 * shift by it loses.  cap: the most points the caller takes (the second pass is skipped above it, and with d_out6 == NULL);
 * *d_out6 = device [points][6] from oslam_dev_alloc, NULL without points */
static int surface_passes(oslam_volume *vol, const int *shift, unsigned min_weight, size_t cap, float **d_out6, uint32_t tot[2],
                          uint32_t *launches)
{
    int rc = OSLAM_OK;
    const uint32_t n_groups = oslamk_surface_groups(&vol->k);
    uint32_t *d_cnt = NULL;                       /* totals in the first 256 bytes, then one counter per workgroup */
    void *stream = oslam_stream();
    tot[0] = tot[1] = 0;
    *launches = 0;
    KCHK(oslam_counters_open(&d_cnt, n_groups, stream));
    KCHK(oslamk_surface_count(&vol->k, shift, min_weight, n_groups, d_cnt + 64, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(tot, d_cnt, sizeof(uint32_t) * 2, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    *launches = 2;
    if (d_out6 && tot[1] > 0 && (size_t)tot[1] <= cap) {
        KCHK(oslam_dev_alloc((void **)d_out6, sizeof(float) * 6 * (size_t)tot[1]));
        KCHK(oslamk_surface_emit(&vol->k, shift, min_weight, n_groups, d_cnt + 64, tot[1], *d_out6, stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        *launches = 3;
    }
done:
    if (rc != OSLAM_OK) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        if (d_out6 && *d_out6) { oslam_dev_free(*d_out6); *d_out6 = NULL; }
    }
    if (d_cnt) oslam_dev_free(d_cnt);
    return rc;
}

/* oslam_volume_surface (shift NULL) and oslam_volume_leaving after their checks of vol and shift */
static int surface_call(oslam_volume *vol, const int *shift, const oslam_surface_params *sp, float *xyz_out, float *nrm_out,
                        size_t cap, size_t *n_out, oslam_surface_result *res)
{
    int rc;
    const double t0 = now_ms();
    oslam_surface_params p;
    float *d_out = NULL, *h_out = NULL;
    uint32_t tot[2] = {0, 0}, launches = 0;
    if (!n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!xyz_out != !nrm_out) return fail(OSLAM_E_INVALID, "xyz_out and nrm_out must both be given or both be NULL");
    if (!xyz_out && cap != 0) return fail(OSLAM_E_INVALID, "cap must be 0 without outputs");
    rc = oslam_surface_check_params(sp, &p);
    if (rc != OSLAM_OK) return rc;
    *n_out = 0;
    if (res) memset(res, 0, sizeof *res);
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    rc = surface_passes(vol, shift, p.min_weight, cap, xyz_out ? &d_out : NULL, tot, &launches);
    if (rc != OSLAM_OK) goto done;
    *n_out = tot[1];
    if (xyz_out && (size_t)tot[1] > cap) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    if (d_out) {
        h_out = (float *)malloc(sizeof(float) * 6 * (size_t)tot[1]);
        if (!h_out) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        HIPCHK(hipMemcpy(h_out, d_out, sizeof(float) * 6 * (size_t)tot[1], hipMemcpyDeviceToHost));
        split_points(h_out, tot[1], xyz_out, nrm_out);
    }
done:
    oslam_volume_unlock();
    free(h_out);
    if (d_out) oslam_dev_free(d_out);
    if ((rc == OSLAM_OK || rc == OSLAM_E_LIMIT) && res) {
        res->crossings = tot[0];
        res->points = tot[1];
        res->launches = launches;
        res->ms_total = (float)(now_ms() - t0);
    }
    return rc;
}

int oslam_volume_surface(oslam_volume *vol, const oslam_surface_params *sp, float *xyz_out, float *nrm_out, size_t cap,
                         size_t *n_out, oslam_surface_result *res)
{
    if (!vol) return fail(OSLAM_E_INVALID, "NULL argument");
    return surface_call(vol, NULL, sp, xyz_out, nrm_out, cap, n_out, res);
}

int oslam_volume_leaving(oslam_volume *vol, const int shift[3], const oslam_surface_params *sp, float *xyz_out, float *nrm_out,
                         size_t cap, size_t *n_out, oslam_surface_result *res)
{
    if (!vol || !shift) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!oslamk_shift_ok(shift)) return fail(OSLAM_E_INVALID, "a shift is at most 2^20 voxels");
    return surface_call(vol, shift, sp, xyz_out, nrm_out, cap, n_out, res);
}

int oslam_volume_surface_cloud(oslam_volume *vol, unsigned min_weight, int *dev, float **d_pts6, uint32_t *np)
{
    int rc;
    uint32_t tot[2], launches;
    *d_pts6 = NULL;
    *np = 0;
    *dev = vol->dev;
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    rc = surface_passes(vol, NULL, min_weight, (size_t)-1, d_pts6, tot, &launches);
    oslam_volume_unlock();
    if (rc == OSLAM_OK) *np = tot[1];
    return rc;
}

/* ---- the fused surface as a triangle mesh (include/oslam.h at oslam_volume_mesh; kernels: oslam_mesh.hip) ---- */
int oslam_mesh_params_default(oslam_mesh_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->min_weight = 1;
    return OSLAM_OK;
}

int oslam_mc_table_row(unsigned mc_case, uint8_t *edges_out, unsigned *n_tri_out)
{
    static const uint8_t ntri[256] = {OSLAM_MC_NTRI_FLAT};
    static const uint8_t edges[256 * OSLAM_MC_ROW] = {OSLAM_MC_EDGES_FLAT};
    if (mc_case > 255u || !edges_out || !n_tri_out) return fail(OSLAM_E_INVALID, "case must lie in 0..255 and the outputs must be given");
    *n_tri_out = ntri[mc_case];
    memcpy(edges_out, edges + (size_t)mc_case * OSLAM_MC_ROW, 3 * (size_t)ntri[mc_case]);
    return OSLAM_OK;
}

int oslam_volume_mesh(oslam_volume *vol, const oslam_mesh_params *mp, float *xyz_out, float *nrm_out, size_t v_cap,
                      uint32_t *tri_out, size_t t_cap, size_t *nv_out, size_t *nt_out, oslam_mesh_result *res)
{
    int rc = OSLAM_OK;
    const double t0 = now_ms();
    oslam_surface_params p = {mp ? mp->min_weight : 1u, {0}};   /* a mesh's parameters are a surface's */
    uint32_t *d_cnt = NULL, *d_eid = NULL, *d_tri = NULL;       /* totals in the first 256 bytes, then two counters per workgroup */
    float *d_xyz = NULL, *d_nrm = NULL;
    uint32_t tot[4] = {0, 0, 0, 0}, launches = 0, n_groups, miss = 0;
    void *stream = oslam_stream();
    if (!vol || !nv_out || !nt_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (!xyz_out != !tri_out) return fail(OSLAM_E_INVALID, "xyz_out and tri_out must both be given or both be NULL");
    if (!xyz_out && nrm_out) return fail(OSLAM_E_INVALID, "nrm_out needs xyz_out");
    if (!xyz_out && (v_cap != 0 || t_cap != 0)) return fail(OSLAM_E_INVALID, "v_cap and t_cap must be 0 without outputs");
    rc = oslam_surface_check_params(&p, &p);
    if (rc != OSLAM_OK) return rc;
    *nv_out = *nt_out = 0;
    if (res) memset(res, 0, sizeof *res);
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    n_groups = oslamk_surface_groups(&vol->k);
    KCHK(oslam_counters_open(&d_cnt, 2 * (size_t)n_groups, stream));
    KCHK(oslamk_mesh_count(&vol->k, p.min_weight, n_groups, d_cnt + 64, d_cnt + 64 + n_groups, d_cnt, stream));
    HIPCHK(hipMemcpyAsync(tot, d_cnt, sizeof tot, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    launches = 3;
    *nv_out = tot[OSLAMK_MESH_T_VERTS];
    *nt_out = tot[OSLAMK_MESH_T_TRIS];
    if (xyz_out && (*nv_out > v_cap || *nt_out > t_cap)) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    if (xyz_out && *nv_out > 0) {
        const uint32_t nv = tot[OSLAMK_MESH_T_VERTS], nt = tot[OSLAMK_MESH_T_TRIS];
        KCHK(oslam_dev_alloc((void **)&d_xyz, sizeof(float) * 3 * (size_t)nv));
        if (nrm_out) KCHK(oslam_dev_alloc((void **)&d_nrm, sizeof(float) * 3 * (size_t)nv));
        KCHK(oslam_dev_alloc((void **)&d_eid, sizeof(uint32_t) * (size_t)nv));
        KCHK(oslamk_mesh_vertices(&vol->k, p.min_weight, n_groups, d_cnt + 64, nv, d_xyz, d_nrm, d_eid, stream));
        launches++;
        if (nt > 0) {
            KCHK(oslam_dev_alloc((void **)&d_tri, sizeof(uint32_t) * 3 * (size_t)nt));
            KCHK(oslamk_mesh_triangles(&vol->k, p.min_weight, n_groups, d_cnt + 64 + n_groups, nt, d_eid, nv, d_tri, d_cnt, stream));
            launches++;
        }
        HIPCHK(hipMemcpyAsync(&miss, d_cnt + OSLAMK_MESH_T_MISS, sizeof miss, hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        if (miss) { rc = fail(OSLAM_E_DEVICE, "a triangle corner found no vertex on its edge: the mesh was not written"); goto done; }
        HIPCHK(hipMemcpy(xyz_out, d_xyz, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost));
        if (nrm_out) HIPCHK(hipMemcpy(nrm_out, d_nrm, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost));
        if (nt > 0) HIPCHK(hipMemcpy(tri_out, d_tri, sizeof(uint32_t) * 3 * (size_t)nt, hipMemcpyDeviceToHost));
    }
done:
    if (rc != OSLAM_OK && rc != OSLAM_E_LIMIT) (void)hipStreamSynchronize((hipStream_t)stream);
    oslam_volume_unlock();
    if (d_tri) oslam_dev_free(d_tri);
    if (d_eid) oslam_dev_free(d_eid);
    if (d_nrm) oslam_dev_free(d_nrm);
    if (d_xyz) oslam_dev_free(d_xyz);
    if (d_cnt) oslam_dev_free(d_cnt);
    if ((rc == OSLAM_OK || rc == OSLAM_E_LIMIT) && res) {
        res->vertices = tot[OSLAMK_MESH_T_VERTS];
        res->triangles = tot[OSLAMK_MESH_T_TRIS];
        res->cubes = tot[OSLAMK_MESH_T_CUBES];
        res->launches = launches;
        res->ms_total = (float)(now_ms() - t0);
    }
    return rc;
}
