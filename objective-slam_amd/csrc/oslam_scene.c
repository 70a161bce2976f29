/*
 * oslam_scene.c -- a scene: from host buffers, from a depth image, from a volume's surface or from the surface of the
 * whole map (voxel store plus window), with its reference points and their frames (scene.cu:24-55).
 */

#include <float.h>
#include <math.h>

#include "oslam_internal.h"
#include "oslam_pose.h"

void oslam_scene_destroy(oslam_scene *s)
{
    if (!s) return;
    (void)hipSetDevice(s->dev);
    oslam_refine_release_grids(s);
    oslam_cloud_free(&s->c);
    free(s->h_ref_idx);
    oslam_dev_free(s->d_block);        /* d_ref_idx, d_tsg and the order are pieces of it */
    oslam_dev_free(s->d_Ts16);
    free(s);
}

/* 10 bits spread to every third bit */
static uint32_t morton_part(uint32_t v)
{
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

/* s->order: the scene's positions a second time in Morton order (cells of 1/1024 of the cloud's largest side, the same
 * on every axis; points with a coordinate that is not finite at the end), the permutation back, and the bounding box of
 * every OSLAMK_ORDER_GROUP consecutive points -- what phase 1 of the scene-key kernels walks (oslamk_order).  It
 * depends on the positions alone, not on d_dist, and is made once per scene from the host copy: three counting passes
 * over n keys.  The scene's own arrays and indices are not touched.  h receives the SCENE_ORDER_WORDS(n) words as they
 * lie in HBM: x, y, z [n] each, the permutation [n], the boxes. */
#define SCENE_ORDER_GROUPS(n) (((n) + OSLAMK_ORDER_GROUP - 1) / OSLAMK_ORDER_GROUP)
#define SCENE_ORDER_WORDS(n) (4 * (n) + 6 * SCENE_ORDER_GROUPS(n))
static int finite3(const float *p)
{
    uint32_t b[3];
    memcpy(b, p, sizeof b);
    return (b[0] & 0x7f800000u) != 0x7f800000u && (b[1] & 0x7f800000u) != 0x7f800000u && (b[2] & 0x7f800000u) != 0x7f800000u;
}

static int scene_order_fill(const oslam_scene *s, uint32_t *h)
{
    int a;
    const size_t n = (size_t)s->c.n, G = SCENE_ORDER_GROUPS(n);
    const float *xyz = s->c.h_xyz;
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f}, side = 0.0f, scale, *f = (float *)h;
    uint64_t *blk, *key, *key2;       /* Morton code << 32 | index */
    uint32_t count[2048], pass;
    size_t i, g;
    int any = 0;
    blk = (uint64_t *)malloc(sizeof(uint64_t) * 2 * n);
    if (!blk) return fail(OSLAM_E_NOMEM, "host allocation failed");
    key = blk;
    key2 = key + n;
    for (i = 0; i < n; i++) {
        const float *p = xyz + 3 * i;
        if (!finite3(p)) continue;
        for (a = 0; a < 3; a++) {
            if (!any || p[a] < lo[a]) lo[a] = p[a];
            if (!any || p[a] > hi[a]) hi[a] = p[a];
        }
        any = 1;
    }
    for (a = 0; a < 3; a++) if (hi[a] - lo[a] > side) side = hi[a] - lo[a];
    scale = side > 0.0f && side <= FLT_MAX ? 1023.0f / side : 0.0f;
    for (i = 0; i < n; i++) {
        const float *p = xyz + 3 * i;
        uint32_t code = 0x7fffffffu;               /* not finite: behind every Morton code (30 bits) */
        if (finite3(p)) {
            uint32_t c[3];
            for (a = 0; a < 3; a++) {
                const float q = (p[a] - lo[a]) * scale;
                c[a] = q >= 1023.0f ? 1023u : q > 0.0f ? (uint32_t)q : 0u;
            }
            code = morton_part(c[0]) | (morton_part(c[1]) << 1) | (morton_part(c[2]) << 2);
        }
        key[i] = ((uint64_t)code << 32) | (uint64_t)i;
    }
    for (pass = 0; pass < 3; pass++) {               /* 11 bits a pass: 33 >= the codes' 31 */
        const uint32_t sh = 32u + 11u * pass;
        uint32_t run = 0, b;
        uint64_t *t;
        memset(count, 0, sizeof count);
        for (i = 0; i < n; i++) count[(key[i] >> sh) & 2047u]++;
        for (b = 0; b < 2048; b++) { const uint32_t c = count[b]; count[b] = run; run += c; }
        for (i = 0; i < n; i++) key2[count[(key[i] >> sh) & 2047u]++] = key[i];
        t = key; key = key2; key2 = t;
    }
    /* the swaps leave the sorted order in key */
    for (i = 0; i < n; i++) {
        const uint32_t at = (uint32_t)key[i];
        const float *p = xyz + 3 * (size_t)at;
        f[i] = p[0];
        f[n + i] = p[1];
        f[2 * n + i] = p[2];
        h[3 * n + i] = at;
    }
    for (g = 0; g < G; g++) {
        float *box = f + 4 * n + 6 * g;
        const size_t e = (g + 1) * OSLAMK_ORDER_GROUP < n ? (g + 1) * OSLAMK_ORDER_GROUP : n;
        for (a = 0; a < 3; a++) {
            float mn = f[a * n + g * OSLAMK_ORDER_GROUP], mx = mn;
            for (i = g * OSLAMK_ORDER_GROUP + 1; i < e; i++) {
                const float v = f[a * n + i];
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
            }
            box[a] = mn;
            box[3 + a] = mx;
        }
        /* the points that are not finite lie at the end of the order: only groups from the first of them on can hold one */
        if ((uint32_t)(key[e - 1] >> 32) == 0x7fffffffu) for (a = 0; a < 6; a++) box[a] = NAN;
    }
    free(blk);
    return OSLAM_OK;
}

/* Scene::Scene (scene.cu:24-55) from host buffers (xyz != NULL) or from a cloud that lies in HBM as [n][6] */
static int scene_create_any(const float *xyz, const float *nrm, size_t stride_bytes, const float *d_aos6, size_t n,
                            float d_dist, unsigned df, const oslam_params *params, oslam_scene **out)
{
    int rc = OSLAM_OK;
    oslam_scene *s = NULL;
    oslam_params p;
    uint32_t *h_up = NULL;             /* what goes to HBM in one piece: the order, the reference points, their frame rows */
    size_t n_all, t, n_ref1, ow;

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
    n_ref1 = (size_t)(s->n_ref ? s->n_ref : 1);
    ow = SCENE_ORDER_WORDS(n);
    s->h_ref_idx = (uint32_t *)malloc(sizeof(uint32_t) * n_ref1);
    h_up = (uint32_t *)malloc(sizeof(uint32_t) * (ow + 9 * n_ref1));
    if (!s->h_ref_idx || !h_up) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
    {
        int k = 0;
        for (t = (size_t)s->rank; t < n_all; t += (size_t)s->world) s->h_ref_idx[k++] = (uint32_t)(t * df);
    }
    rc = scene_order_fill(s, h_up);
    if (rc != OSLAM_OK) goto done;
    memcpy(h_up + ow, s->h_ref_idx, sizeof(uint32_t) * (size_t)s->n_ref);
    oslam_T_g_rows(s->c.h_xyz, s->c.h_nrm, s->h_ref_idx, (size_t)s->n_ref, (float *)(h_up + ow + n_ref1));
    /* one block, one copy: a depth frame makes a scene, and every copy from the host waits for the device */
    HIPCHK((hipError_t)oslam_dev_alloc((void **)&s->d_block, sizeof(uint32_t) * (ow + 9 * n_ref1)));
    HIPCHK(hipMemcpy(s->d_block, h_up, sizeof(uint32_t) * (ow + 9 * n_ref1), hipMemcpyHostToDevice));
    s->order.sx = (const float *)s->d_block;
    s->order.sy = s->order.sx + n;
    s->order.sz = s->order.sx + 2 * n;
    s->order.perm = s->d_block + 3 * n;
    s->order.box = s->order.sx + 4 * n;
    s->d_ref_idx = s->d_block + ow;
    s->d_tsg = (float *)(s->d_block + ow + n_ref1);
done:
    free(h_up);
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
