/*
 * oslam_normals.c -- normals for clouds and meshes that come without them (include/oslam.h at oslam_cloud_normals): the
 * host side of k_normals (oslam_normals.hip) and the mesh rule, which is host code.  A cloud call checks its arguments,
 * lays the refinement stage's grid over the finite points (edge = radius, enlarged by scene_grid's rule at the cell cap),
 * uploads the coordinates, enqueues the grid build and the one kernel, and reads the results once.
 */
#include <math.h>

#include "oslam_internal.h"

int oslam_normals_params_default(oslam_normals_params *p)
{
    if (!p) return oslam_fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->min_neighbours = 5;
    p->orient = 1;
    p->line_ratio = 0.01f;
    return OSLAM_OK;
}

static int check_cloud_args(const float *xyz, size_t n, size_t stride_bytes, const oslam_normals_params *np)
{
    if (!xyz || !np) return oslam_fail(OSLAM_E_INVALID, "normals: NULL argument");
    if (n == 0 || n > 0x7fffffffu || stride_bytes < 12) return oslam_fail(OSLAM_E_INVALID, "normals: bad cloud");
    if (!(np->radius > 0.0f) || !isfinite(np->radius) || !isfinite(16384.0f / np->radius)) return oslam_fail(OSLAM_E_INVALID, "normals: radius must be > 0 and finite");
    if (np->min_neighbours < 3) return oslam_fail(OSLAM_E_INVALID, "normals: min_neighbours below 3");
    if (!isfinite(np->viewpoint[0]) || !isfinite(np->viewpoint[1]) || !isfinite(np->viewpoint[2]))
        return oslam_fail(OSLAM_E_INVALID, "normals: viewpoint is not finite");
    if (!(np->line_ratio >= 0.0f) || !isfinite(np->line_ratio)) return oslam_fail(OSLAM_E_INVALID, "normals: line_ratio must be >= 0 and finite");
    return OSLAM_OK;
}

/* the whole device call; every output pointer may be NULL */
static int cloud_normals(const float *xyz, size_t n, size_t stride, const oslam_normals_params *np, int dev, float *nrm_out,
                         float *curvature_out, uint8_t *valid_out, int64_t *moments_out, oslam_normals_result *res)
{
    int rc = OSLAM_OK, devsel, a, have = 0;
    const double t0 = now_ms();
    scratch_pool *pool = NULL;
    oslamk_grid g;
    oslamk_normals_args ka;
    oslamk_cloud c;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, edge, cells;
    size_t i, n_items, nb, bytes, off_out;
    float *h_soa = NULL, *d_soa;
    char *block = NULL, *base, *h_res = NULL;
    hipEvent_t ev[3] = {NULL, NULL, NULL};
    void *stream = oslam_stream();
    float ms_grid = 0.0f, ms_kernel = 0.0f;
    uint32_t n_valid = 0;

    rc = oslam_pick_device(dev, &devsel);
    if (rc != OSLAM_OK) return rc;
    h_soa = (float *)malloc(sizeof(float) * 3 * n);
    if (!h_soa) return oslam_fail(OSLAM_E_NOMEM, "host allocation failed");
    for (i = 0; i < n; i++) {
        const float *p = (const float *)((const char *)xyz + i * stride);
        for (a = 0; a < 3; a++) h_soa[(size_t)a * n + i] = p[a];
        if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) continue;
        for (a = 0; a < 3; a++) {
            if (!have || p[a] < lo[a]) lo[a] = p[a];
            if (!have || p[a] > hi[a]) hi[a] = p[a];
        }
        have = 1;
    }
    /* scene_grid's rule (oslam_refine.c): an edge a little above the radius, so that a point within the radius is at most
     * one cell away in every axis; enlarged until the cells fit */
    edge = (double)np->radius * (1.0 + 1e-4);
    for (;;) {
        cells = 1.0;
        for (a = 0; a < 3; a++) cells *= floor((hi[a] - lo[a]) / edge) + 1.0;
        if (cells <= (double)OSLAMK_GRID_MAX_CELLS) break;
        edge *= cbrt(cells / (double)OSLAMK_GRID_MAX_CELLS) * 1.01;
    }
    memset(&g, 0, sizeof g);
    g.inv_edge = 1.0 / edge;
    for (a = 0; a < 3; a++) {
        g.lo[a] = lo[a];
        g.dim[a] = (int)floor((hi[a] - lo[a]) * g.inv_edge) + 1;
    }
    g.n_cells = (uint32_t)g.dim[0] * (uint32_t)g.dim[1] * (uint32_t)g.dim[2];
    if (g.n_cells > OSLAMK_GRID_MAX_CELLS) { free(h_soa); return oslam_fail(OSLAM_E_LIMIT, "normals: grid too large"); }
    g.n = (int)n;
    n_items = (size_t)g.n_cells + 1;
    nb = (n_items + OSLAMK_SCAN_ITEMS - 1) / OSLAMK_SCAN_ITEMS;

    rc = oslam_pool_enter(devsel, &pool);
    if (rc != OSLAM_OK) { free(h_soa); return rc; }
    /* device block: grid arrays | coordinates (structure of arrays) | normals, curvature, moments, valid */
    off_out = 2 * align256(4 * n_items) + align256(4 * nb) + 2 * align256(4 * n) + align256(32 * n) + align256(12 * n);
    bytes = off_out + align256(12 * n) + align256(4 * n) + align256(moments_out ? 80 * n : 0) + align256(n);
    h_res = (char *)malloc(bytes - off_out);
    if (!h_res) { rc = oslam_fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    KCHK(oslam_dev_alloc((void **)&block, bytes));
    base = block;
    g.start = (uint32_t *)base;   base += align256(4 * n_items);
    g.local = (uint32_t *)base;   base += align256(4 * n_items);
    g.bsum = (uint32_t *)base;    base += align256(4 * nb);
    g.cell_of = (uint32_t *)base; base += align256(4 * n);
    g.rank = (uint32_t *)base;    base += align256(4 * n);
    g.pts = (float *)base;        base += align256(32 * n);
    d_soa = (float *)base;        base += align256(12 * n);
    memset(&ka, 0, sizeof ka);
    ka.nrm = (float *)base;       base += align256(12 * n);
    ka.curvature = (float *)base; base += align256(4 * n);
    if (moments_out) { ka.moments = (int64_t *)base; base += align256(80 * n); }
    ka.valid = (uint8_t *)base;
    ka.r2 = np->radius * np->radius;
    ka.scale = 16384.0f / np->radius;
    for (a = 0; a < 3; a++) ka.view[a] = (double)np->viewpoint[a];
    ka.line_ratio = (double)np->line_ratio;
    ka.min_neighbours = (int64_t)np->min_neighbours;
    ka.orient = np->orient != 0;
    /* the grid wants a cloud with normal arrays: they alias the coordinates (pts[2k + 1] is never read here) */
    c.px = c.nx = d_soa;
    c.py = c.ny = d_soa + n;
    c.pz = c.nz = d_soa + 2 * n;
    c.n = (int)n;

    for (a = 0; a < 3; a++) HIPCHK(hipEventCreate(&ev[a]));
    HIPCHK(hipMemcpyAsync(d_soa, h_soa, sizeof(float) * 3 * n, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(hipEventRecord(ev[0], (hipStream_t)stream));
    KCHK(oslamk_refine_grid_build(&g, c, stream));
    HIPCHK(hipEventRecord(ev[1], (hipStream_t)stream));
    KCHK(oslamk_normals(&g, &ka, stream));
    HIPCHK(hipEventRecord(ev[2], (hipStream_t)stream));
    HIPCHK(hipMemcpyAsync(h_res, block + off_out, bytes - off_out, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHK(hipEventElapsedTime(&ms_grid, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(&ms_kernel, ev[1], ev[2]));

    {
        const char *h = h_res;
        const uint8_t *v;
        if (nrm_out) memcpy(nrm_out, h, 12 * n);
        h += align256(12 * n);
        if (curvature_out) memcpy(curvature_out, h, 4 * n);
        h += align256(4 * n);
        if (moments_out) { memcpy(moments_out, h, 80 * n); h += align256(80 * n); }
        v = (const uint8_t *)h;
        for (i = 0; i < n; i++) n_valid += v[i];
        if (valid_out) memcpy(valid_out, v, n);
    }
    if (res) {
        res->n_valid = n_valid;
        res->n_cells = g.n_cells;
        res->edge = (float)edge;
        res->launches = 6;            /* the grid build's memset and four kernels, then k_normals */
        res->ms_grid = ms_grid;
        res->ms_kernel = ms_kernel;
        res->ms_total = (float)(now_ms() - t0);
    }
done:
    if (rc != OSLAM_OK) (void)hipStreamSynchronize((hipStream_t)stream);
    for (a = 0; a < 3; a++)
        if (ev[a]) (void)hipEventDestroy(ev[a]);
    if (block) oslam_dev_free(block);
    oslam_pool_unlock(pool);
    free(h_res);
    free(h_soa);
    return rc;
}

int oslam_cloud_normals(const float *xyz, size_t n, size_t stride_bytes, const oslam_normals_params *np, int dev,
                        float *nrm_out, float *curvature_out, uint8_t *valid_out, oslam_normals_result *res)
{
    int rc;
    if (!nrm_out) return oslam_fail(OSLAM_E_INVALID, "normals: NULL argument");
    rc = check_cloud_args(xyz, n, stride_bytes, np);
    if (rc != OSLAM_OK) return rc;
    return cloud_normals(xyz, n, stride_bytes, np, dev, nrm_out, curvature_out, valid_out, NULL, res);
}

int oslam_cloud_normal_moments(const float *xyz, size_t n, size_t stride_bytes, const oslam_normals_params *np, int dev,
                               int64_t *moments_out)
{
    int rc;
    if (!moments_out) return oslam_fail(OSLAM_E_INVALID, "normals: NULL argument");
    rc = check_cloud_args(xyz, n, stride_bytes, np);
    if (rc != OSLAM_OK) return rc;
    return cloud_normals(xyz, n, stride_bytes, np, dev, NULL, NULL, NULL, moments_out, NULL);
}

/* ------------------------------------------------------------------------ */
int oslam_mesh_normals(const float *xyz, size_t nv, size_t stride_bytes, const uint32_t *tri, size_t nt, float *nrm_out,
                       uint8_t *valid_out)
{
    double *acc;
    size_t t, v;
    int a;
    if (!xyz || !nrm_out || (nt && !tri) || nv == 0 || stride_bytes < 12) return oslam_fail(OSLAM_E_INVALID, "mesh normals: bad arguments");
    for (t = 0; t < 3 * nt; t++)
        if (tri[t] >= nv) return oslam_fail(OSLAM_E_INVALID, "mesh normals: vertex index out of range");
    acc = (double *)calloc(3 * nv, sizeof *acc);
    if (!acc) return oslam_fail(OSLAM_E_NOMEM, "host allocation failed");
    for (t = 0; t < nt; t++) {
        const float *pa = (const float *)((const char *)xyz + (size_t)tri[3 * t] * stride_bytes);
        const float *pb = (const float *)((const char *)xyz + (size_t)tri[3 * t + 1] * stride_bytes);
        const float *pc = (const float *)((const char *)xyz + (size_t)tri[3 * t + 2] * stride_bytes);
        double e1[3], e2[3], cr[3];
        for (a = 0; a < 3; a++) {
            e1[a] = (double)pb[a] - (double)pa[a];
            e2[a] = (double)pc[a] - (double)pa[a];
        }
        cr[0] = e1[1] * e2[2] - e1[2] * e2[1];
        cr[1] = e1[2] * e2[0] - e1[0] * e2[2];
        cr[2] = e1[0] * e2[1] - e1[1] * e2[0];
        for (a = 0; a < 3; a++) {
            acc[3 * (size_t)tri[3 * t] + a] += cr[a];
            acc[3 * (size_t)tri[3 * t + 1] + a] += cr[a];
            acc[3 * (size_t)tri[3 * t + 2] + a] += cr[a];
        }
    }
    for (v = 0; v < nv; v++) {
        const double *s = acc + 3 * v;
        const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
        const int ok = len > 0.0 && isfinite(len);
        for (a = 0; a < 3; a++) nrm_out[3 * v + a] = ok ? (float)(s[a] / len) : 0.0f;
        if (valid_out) valid_out[v] = (uint8_t)ok;
    }
    free(acc);
    return OSLAM_OK;
}
