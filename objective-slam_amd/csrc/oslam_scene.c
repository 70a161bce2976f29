/*
 * oslam_scene.c -- a scene: from host buffers, from a depth image, from a volume's surface or from the surface of the
 * whole map (voxel store plus window), with its reference points and their frames (scene.cu:24-55).
 */

#include "oslam_internal.h"
#include "oslam_pose.h"

void oslam_scene_destroy(oslam_scene *s)
{
    if (!s) return;
    (void)hipSetDevice(s->dev);
    oslam_refine_release_grids(s);
    oslam_cloud_free(&s->c);
    free(s->h_ref_idx);
    oslam_dev_free(s->d_ref_idx);
    oslam_dev_free(s->d_tsg);
    oslam_dev_free(s->d_Ts16);
    free(s);
}

/* Scene::Scene (scene.cu:24-55) from host buffers (xyz != NULL) or from a cloud that lies in HBM as [n][6] */
static int scene_create_any(const float *xyz, const float *nrm, size_t stride_bytes, const float *d_aos6, size_t n,
                            float d_dist, unsigned df, const oslam_params *params, oslam_scene **out)
{
    int rc = OSLAM_OK;
    oslam_scene *s = NULL;
    oslam_params p;
    float *h_tsg = NULL;
    size_t n_all, t;

    *out = NULL;
    if (!(d_dist >= 0.0f) || df == 0) return fail(OSLAM_E_INVALID, "bad scene arguments");
    if (n < 2) return fail(OSLAM_E_INVALID, "scene needs at least 2 points");
    if (n > (1u << 28)) return fail(OSLAM_E_LIMIT, "scene larger than 2^28 points");
    if (params) p = *params; else oslam_params_default(&p);
    if (p.shard_world < 1 || p.shard_rank < 0 || p.shard_rank >= p.shard_world) return fail(OSLAM_E_INVALID, "bad shard");
    s = (oslam_scene *)calloc(1, sizeof *s);
    if (!s) return fail(OSLAM_E_NOMEM, "host allocation failed");
    rc = oslam_pick_device(p.dev, &s->dev);
    if (rc != OSLAM_OK) goto done;
    rc = oslam_cloud_make(&s->c, xyz, nrm, stride_bytes, d_aos6, n);
    if (rc != OSLAM_OK) goto done;
    s->d_dist = d_dist;
    s->df = df;
    s->rank = p.shard_rank;
    s->world = p.shard_world;
    /* reference points: idx % df == 0 (kernel.cu:432), dealt round-robin to ranks */
    n_all = (n + df - 1) / df;
    s->n_ref = 0;
    for (t = (size_t)s->rank; t < n_all; t += (size_t)s->world) s->n_ref++;
    s->h_ref_idx = (uint32_t *)malloc(sizeof(uint32_t) * (s->n_ref ? s->n_ref : 1));
    h_tsg = (float *)malloc(sizeof(float) * 8 * (s->n_ref ? s->n_ref : 1));
    if (!s->h_ref_idx || !h_tsg) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    {
        int k = 0;
        for (t = (size_t)s->rank; t < n_all; t += (size_t)s->world) s->h_ref_idx[k++] = (uint32_t)(t * df);
    }
    oslam_T_g_rows(s->c.h_xyz, s->c.h_nrm, s->h_ref_idx, (size_t)s->n_ref, h_tsg);
    HIPCHK((hipError_t)oslam_dev_alloc((void **)&s->d_ref_idx, sizeof(uint32_t) * (s->n_ref ? s->n_ref : 1)));
    HIPCHK((hipError_t)oslam_dev_alloc((void **)&s->d_tsg, sizeof(float) * 8 * (s->n_ref ? s->n_ref : 1)));
    if (s->n_ref) {
        HIPCHK(hipMemcpy(s->d_ref_idx, s->h_ref_idx, sizeof(uint32_t) * s->n_ref, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s->d_tsg, h_tsg, sizeof(float) * 8 * s->n_ref, hipMemcpyHostToDevice));
    }
done:
    free(h_tsg);
    if (rc != OSLAM_OK) { oslam_scene_destroy(s); return rc; }
    *out = s;
    return OSLAM_OK;
}

int oslam_scene_create(const float *xyz, const float *nrm, size_t n, size_t stride_bytes,
                       float d_dist, unsigned df, const oslam_params *params, oslam_scene **out)
{
    if (!out) return fail(OSLAM_E_INVALID, "out is NULL");
    *out = NULL;
    if (!xyz || !nrm || stride_bytes < 12) return fail(OSLAM_E_INVALID, "bad scene arguments");
    return scene_create_any(xyz, nrm, stride_bytes, NULL, n, d_dist, df, params, out);
}

/* a cloud that lies in HBM as [np][6] -> voxel grid (leaf > 0) -> scene; `few` names the source when fewer than 2 points
 * are left */
static int scene_from_points6(const float *d_pts6, uint32_t np, float leaf, float d_dist, unsigned df, const oslam_params *p,
                              const char *few, oslam_scene **out, size_t *n_points_out)
{
    int rc = OSLAM_OK, k;
    float *d_soa = NULL, *d_vox6 = NULL;
    const float *d_final = d_pts6;
    uint32_t nv = 0;
    size_t n_final = np;
    if (leaf > 0.0f && np > 0) {
        HIPCHK((hipError_t)oslam_dev_alloc((void **)&d_soa, sizeof(float) * 6 * (size_t)np));
        HIPCHK((hipError_t)oslam_dev_alloc((void **)&d_vox6, sizeof(float) * 6 * (size_t)np));
        KCHK(oslamk_aos6_to_soa(d_pts6, np, d_soa, oslam_stream()));
        k = oslamk_voxel_grid(oslam_soa_cloud(d_soa, np), leaf, d_vox6, &nv, oslam_stream());
        if (k == -1) { rc = fail(OSLAM_E_LIMIT, "leaf size too small for the cloud extent (voxel count overflows int32)"); goto done; }
        if (k != 0) { rc = fail(OSLAM_E_DEVICE, hipGetErrorString((hipError_t)k)); goto done; }
        d_final = d_vox6;
        n_final = nv;
    }
    if (n_final < 2) { rc = fail(OSLAM_E_INVALID, few); goto done; }
    /* the scene's arrays are made from the cloud where it lies; one copy comes back for the host's reference frames */
    rc = scene_create_any(NULL, NULL, 0, d_final, n_final, d_dist, df, p, out);
    if (rc == OSLAM_OK && n_points_out) *n_points_out = n_final;
done:
    oslam_dev_free(d_soa);
    oslam_dev_free(d_vox6);
    return rc;
}

int oslam_scene_from_depth(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam,
                           float leaf, float d_dist, unsigned df, const oslam_params *params, oslam_scene **out,
                           size_t *n_points_out)
{
    int rc;
    oslam_params p;
    void *d_img = NULL;
    float *d_pts6 = NULL;
    uint32_t np = 0;
    if (!out) return fail(OSLAM_E_INVALID, "out is NULL");
    *out = NULL;
    if (n_points_out) *n_points_out = 0;
    if (!(leaf >= 0.0f)) return fail(OSLAM_E_INVALID, "bad depth image arguments");
    if (params) p = *params; else oslam_params_default(&p);
    rc = oslam_depth_points(depth, depth_is_u16, width, height, cam, p.dev, &d_img, &d_pts6, &np);
    if (rc == OSLAM_OK)
        rc = scene_from_points6(d_pts6, np, leaf, d_dist, df, &p, "the depth image leaves fewer than 2 scene points", out,
                                n_points_out);
    oslam_dev_free(d_img);
    oslam_dev_free(d_pts6);
    return rc;
}

/* the extraction at the head of a chain: checks its own parameters before anything else, then leaves the cloud in HBM as
 * [*np][6] on device *dev (NULL without points) */
typedef int (*scene_extract_fn)(void *ctx, int *dev, float **d_pts6, uint32_t *np);

/* oslam_scene_from_volume and oslam_scene_from_world: the checks, the extraction, then grid and scene.  handle_ok: the
 * handle the extraction reads was given */
static int scene_from_extraction(scene_extract_fn extract, void *ctx, int handle_ok, const char *no_handle, float leaf, float d_dist,
                                 unsigned df, const oslam_params *params, const char *few, oslam_scene **out, size_t *n_points_out)
{
    int rc;
    oslam_params p;
    float *d_pts6 = NULL;
    uint32_t np = 0;
    if (!out) return fail(OSLAM_E_INVALID, "out is NULL");
    *out = NULL;
    if (n_points_out) *n_points_out = 0;
    if (!handle_ok) return fail(OSLAM_E_INVALID, no_handle);
    if (!(leaf >= 0.0f) || !(d_dist >= 0.0f) || df == 0) return fail(OSLAM_E_INVALID, "bad scene arguments");
    if (params) p = *params; else oslam_params_default(&p);
    /* the scene lives where the extraction ran */
    rc = extract(ctx, &p.dev, &d_pts6, &np);
    if (rc == OSLAM_OK) rc = scene_from_points6(d_pts6, np, leaf, d_dist, df, &p, few, out, n_points_out);
    oslam_dev_free(d_pts6);
    return rc;
}

typedef struct volume_extract {
    oslam_volume *vol;
    const oslam_surface_params *sp;
} volume_extract;

static int extract_volume(void *ctx, int *dev, float **d_pts6, uint32_t *np)
{
    const volume_extract *x = (const volume_extract *)ctx;
    oslam_surface_params s;
    const int rc = oslam_surface_check_params(x->sp, &s);
    return rc != OSLAM_OK ? rc : oslam_volume_surface_cloud(x->vol, s.min_weight, dev, d_pts6, np);
}

int oslam_scene_from_volume(oslam_volume *vol, const oslam_surface_params *sp, float leaf, float d_dist, unsigned df,
                            const oslam_params *params, oslam_scene **out, size_t *n_points_out)
{
    volume_extract x = {vol, sp};
    return scene_from_extraction(extract_volume, &x, vol != NULL, "volume is NULL", leaf, d_dist, df, params,
                                 "the volume's surface leaves fewer than 2 scene points", out, n_points_out);
}

typedef struct world_extract {
    oslam_world *w;
    oslam_volume *vol;
    const oslam_world_surface_params *sp;
} world_extract;

static int extract_world(void *ctx, int *dev, float **d_pts6, uint32_t *np)
{
    const world_extract *x = (const world_extract *)ctx;
    oslam_world_surface_params s;
    const int rc = oslam_world_surface_check_params(x->sp, &s);
    return rc != OSLAM_OK ? rc : oslam_world_surface_cloud(x->w, x->vol, &s, dev, d_pts6, np);
}

int oslam_scene_from_world(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, float leaf, float d_dist,
                           unsigned df, const oslam_params *params, oslam_scene **out, size_t *n_points_out)
{
    world_extract x = {w, vol, sp};
    return scene_from_extraction(extract_world, &x, w != NULL, "world is NULL", leaf, d_dist, df, params,
                                 "the map's surface leaves fewer than 2 scene points", out, n_points_out);
}
