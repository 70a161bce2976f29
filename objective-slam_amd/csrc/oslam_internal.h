/*
 * oslam_internal.h -- the handles behind include/oslam.h and the helpers that the host translation units of
 * liboslam_hip.so share (oslam_host.c and the stage files next to it).  Not installed.
 */
#ifndef OSLAM_INTERNAL_H
#define OSLAM_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "oslam.h"
#include "oslam_kernels.h"
#include "oslam_rigid.h"

typedef struct cloud_buf {
    int n;
    float *h_xyz, *h_nrm;             /* packed [n][3] host copies (pose stage) */
    float *d_soa;                     /* 6*n floats: px py pz nx ny nz */
    oslamk_cloud k;
} cloud_buf;

struct oslam_model {
    int dev;
    cloud_buf c;
    float d_dist, inv_d_dist;
    oslam_params params;
    oslamk_table table;
    oslamk_entries ent;
    uint32_t n_entries;
    uint64_t num_model_keys;
    float *weights;
    /* align workspace */
    oslamk_counters *d_counters;
    oslamk_cell *d_out;
    uint32_t out_cap;
    oslam_cell *h_out;
    /* multi-GPU: peaks of the last oslam_align_local (in h_out), survivors of this rank (device) */
    size_t n_local;
    uint32_t local_max;
    oslamk_cell *d_union;
    size_t union_cap;
    /* frames T_g of the model points [M][16] and the point weights, for the pose tail on the device */
    float *d_Tm16, *d_weights;
    /* last result: on the host, or still on the device (pose tail ran there) until a tap asks for it */
    oslam_cell *last_cells;
    float *last_poses;
    size_t n_last;
    int last_on_device;
    oslamk_cell *d_pose_cells;
    float *d_pose_T;
    size_t pose_cap;
    /* host copy of the table for the bucket tap */
    oslamk_slot *h_slots;
    /* member of a database group: table.ukeys / reach belong to the group (oslam_db) */
    int shared_union;
    /* its key tables are gone (a database was destroyed without giving them back, or rebuilding them failed):
     * the model can only be destroyed */
    int unusable;
    /* the cloud's shape (oslam_cloud_shape), made with the cloud and never written again: the double mean of the
     * points (the pivot of the refinement and tracking stages), its float rounding and the extent (the instance rule) */
    double cm[3];
    float inst_c[3], inst_extent;
    /* the largest distance of a point from cm, made on first use by the explain stage (oslam_explain.c) */
    double bound_r;
    int bound_set;
};

struct oslam_scene {
    int dev;
    cloud_buf c;
    float d_dist;
    unsigned df;
    int rank, world;
    int n_ref;
    uint32_t *h_ref_idx, *d_ref_idx;  /* d_ref_idx and d_tsg: pieces of d_block */
    float *d_tsg;
    float *d_Ts16;                    /* frames of every reference-point candidate (index % df == 0, all ranks) */
    uint32_t *d_block;                /* one block: the points in Morton order, the permutation, the group boxes; d_ref_idx; d_tsg */
    oslamk_order order;               /* the first of its pieces (oslam_scene.c: scene_order_fill) */
    struct oslam_scene_grid *grids;   /* uniform grids of the refinement stage (oslam_refine.c), NULL until the first */
};

struct oslam_view {
    int dev;                          /* stays the first field: the argument tests (tests/test_*_host.py) hand the entry
                                         points zeroed stand-in handles and write the device number at offset 0 */
    oslamk_view k;
    float *d_z;
    float max_jump;                   /* of the camera: the normal map's depth-step limit */
    float *d_maps;                    /* vertex and normal map of the tracking stage (oslam_track.c), NULL until the first */
    uint32_t *d_colour;               /* the registered colour image, [h][w] words (oslam_colour.c), NULL without one */
};

struct oslam_volume {
    int dev;                          /* stays the first field, as in oslam_view (the argument tests write it) */
    oslamk_volume k;                  /* k.origin follows off (oslam_volume_shift); p.origin stays the created one */
    oslam_volume_params p;
    int off[3];                       /* the window's offset in voxels: the shift's commit writes it (oslam_window.c) */
    uint32_t *spare;                  /* the second buffer of oslam_volume_shift, NULL until the first shift */
    oslamk_colour colour;             /* the colour buffer (oslam_colour.c); words NULL until oslam_volume_colour_enable */
    uint32_t *colour_spare;           /* its second buffer for a shift, NULL until the first shift of a coloured volume */
};

struct oslam_pyramid {
    int dev;                          /* stays the first field, as in oslam_view */
    unsigned n_levels;
    oslam_view *level[3];             /* [0] is the caller's base (borrowed), the rest are owned */
};

struct oslam_render {
    int dev;                          /* stays the first field, as in oslam_view */
    oslam_view *view;                 /* the z image as a genuine view (owned; oslam_render_view lends it) */
    size_t n_hyp;                     /* the hypotheses of the call: labels lie in -1 .. n_hyp - 1 */
    int32_t *d_labels;                /* [h * w], then tol[n_hyp] behind it in the same block */
    float *d_tol;
};

struct oslam_planes {
    int dev;                          /* stays the first field, as in oslam_view; w and h follow it (the argument tests write them) */
    int w, h;
    uint32_t n_planes, max_planes;
    int32_t *d_labels;                /* [h * w] on the device, -1 = no plane */
    oslam_plane planes[OSLAM_PLANES_MAX];
    uint32_t counts[OSLAM_PLANES_MAX][OSLAMK_PLANES_CAND];    /* the rounds' counts and moments, as the device left them */
    int64_t moments[OSLAM_PLANES_MAX][10];
};

struct oslam_segments {
    int dev;                          /* stays the first field, as in oslam_view; w and h follow it (the argument tests write them) */
    int w, h;
    uint32_t n_segments;
    uint32_t *d_roots;                /* [h * w] on the device: the root of every in pixel, all ones elsewhere */
    int32_t *d_labels;                /* [h * w] on the device, -1 = no segment */
    oslam_segment seg[OSLAM_SEGMENTS_MAX];
};

typedef struct db_group {
    int n;
    size_t *members;                  /* indices into db->models */
    uint32_t *ukeys, *reach, *kmap, *uids;   /* the group's union table, reachable-distance bitset, key map and key numbers (n > 1) */
} db_group;

struct oslam_db {
    int dev;
    size_t n;
    oslam_model **models;             /* borrowed */
    int n_groups;
    db_group *groups;
};

/* ---- error text, stream, device (oslam_host.c) ---- */
/* records `what` for oslam_last_error and returns code */
int oslam_fail(int code, const char *what);
static inline int fail(int code, const char *what) { return oslam_fail(code, what); }
/* records "call: HIP error text (file:line)" and returns OSLAM_E_DEVICE */
int oslam_fail_call(const char *call, int err, const char *file, int line);

/* HIPCHK: a call that returns a hipError_t; KCHK: an oslamk_* launcher (0 or a hipError_t).  On failure the
 * error text names the call and its place, rc = OSLAM_E_DEVICE, and the function goes to its `done:` */
#define KCHK(call)                                                                          \
    do {                                                                                    \
        const int k_ = (int)(call);                                                         \
        if (k_ != 0) { rc = oslam_fail_call(#call, k_, __FILE__, __LINE__); goto done; }    \
    } while (0)
#define HIPCHK(call) KCHK(call)

static inline double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

/* offsets of the parts of one device block */
static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

/* a counter block from the kept scratch blocks: 256 zeroed bytes of totals, then n_words uint32 that the kernels write
 * before they read; a hipError_t */
static inline int oslam_counters_open(uint32_t **d_cnt, size_t n_words, void *stream)
{
    const int k = oslam_dev_alloc((void **)d_cnt, 256 + sizeof(uint32_t) * n_words);
    return k != 0 ? k : (int)hipMemsetAsync(*d_cnt, 0, 256, (hipStream_t)stream);
}

/* interleaved [n][6] points (x y z nx ny nz) into xyz [n][3] and normals [n][3] */
static inline void split_points(const float *pts6, size_t n, float *xyz_out, float *nrm_out)
{
    size_t i;
    for (i = 0; i < n; i++) {
        memcpy(xyz_out + 3 * i, pts6 + 6 * i, 3 * sizeof(float));
        memcpy(nrm_out + 3 * i, pts6 + 6 * i + 3, 3 * sizeof(float));
    }
}

/* the launch stream of this thread's calls (oslam_set_stream) */
void *oslam_stream(void);
/* binds device dev_req (clamped to the last device, ppf.cu:45) */
int oslam_pick_device(int dev_req, int *dev_out);

/* ---- clouds (oslam_cloud.c) ---- */
void oslam_cloud_free(cloud_buf *c);
int oslam_cloud_make(cloud_buf *c, const float *xyz, const float *nrm, size_t stride, const float *d_aos6, size_t n);
oslamk_cloud oslam_soa_cloud(const float *d_soa, size_t n);
/* a depth image's points in HBM as [*np][6] on device dev (*d_img: the image); the caller frees both blocks */
int oslam_depth_points(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam, int dev,
                       void **d_img, float **d_pts6, uint32_t *np);

/* ---- model key tables (oslam_model.c), rebuilt by the database ---- */
int oslam_build_kmap(oslamk_table *t, float d_dist, const oslamk_table *parts, int n_parts, int vote_order);
int oslam_build_union(oslam_model *m, uint32_t distinct, uint32_t *d_n_keys, uint32_t *d_overflow);
int oslam_build_uinfo(oslam_model *m);

/* gives back the scene's refinement grids (oslam_refine.c); called by oslam_scene_destroy */
void oslam_refine_release_grids(oslam_scene *s);

/* ---- votes and the scratch pool of each device (oslam_vote.c) ---- */
typedef struct scratch_pool scratch_pool;
int oslam_check_pair(const oslam_model *m, const oslam_scene *s);
/* the entry of a call that launches on device dev: binds it and locks its pool, held until oslam_pool_unlock */
int oslam_pool_enter(int dev, scratch_pool **pool);
void oslam_pool_unlock(scratch_pool *p);
int oslam_pool_reserve_counts(scratch_pool *p, size_t n_ref);
void oslam_ref_order(const uint32_t *keep, size_t n, uint32_t *order);
/* what a vote pass reports; a pass sets ms and probed and adds to the rest.  NULL where it is not wanted */
typedef struct oslam_vote_times {
    float ms;                         /* the whole pass on the stream */
    float ms_vote_kernel, ms_key_kernel;
    uint32_t launches;                /* batches */
    uint64_t probed;                  /* pairs within reach */
} oslam_vote_times;
int oslam_pool_read_hits(const scratch_pool *p, uint32_t *numbers_out, uint32_t *theta_out, uint32_t *idx_out, size_t cap,
                         size_t *n_out, uint32_t *keep_out);
int oslam_run_votes_group(scratch_pool *pool, oslam_model *const *ms, int nm, oslam_scene *s, const uint32_t *d_ref_idx,
                          const float *d_tsg, int n_ref, uint32_t fixed_gmax, uint32_t *acc_dump, oslamk_counters *cnt,
                          oslam_vote_times *t);
void oslam_vote_stats(oslam_stats *st, const scratch_pool *pool, const oslam_model *m, const oslam_scene *s,
                      const oslamk_counters *cnt, const oslam_vote_times *t);
int oslam_vote_records(scratch_pool *pool, oslam_model *m, oslam_scene *s, oslamk_counters *cnt, size_t *n_cells,
                       oslam_stats *st, int to_host);
int oslam_grow_records(oslam_model *m, uint64_t need);
/* clustering scores in the current pool (the pose stage's hook, oslam_pose.h) */
int oslam_cluster_scores_on_device(size_t n, const float *trans, const float *quat, const float *wv,
                                   const int32_t *cell, const uint32_t *hash_idx, float d_dist, int use_l1,
                                   float *score);

/* ---- pose tail (oslam_align.c) ---- */
/* what an instance call asks of one model's tail (oslam_instances.c): the resolved rule for the device and the
 * parameters for the host rule; the winners come back in an oslamk_inst_out */
typedef struct oslam_inst_req {
    oslamk_inst_args a;
    const oslam_instance_params *ip;
    float extent;
} oslam_inst_req;
size_t oslam_pose_gpu_from(const oslam_model *m);
void oslam_drop_last(oslam_model *m);
int oslam_pose_tables(oslam_model *m, oslam_scene *s);
int oslam_ensure_pose_buffers(oslam_model *m, size_t n);
/* the 64 rotations about x of the pose tail, made on first use */
const float *oslam_rotx(void);
/* req == NULL: the winner only; otherwise the instance selection too, into *sel */
int oslam_finish_after_votes(oslam_model *m, oslam_scene *s, size_t n, uint32_t gmax, int try_device, float T[16],
                             oslam_stats *stats, const oslam_inst_req *req, oslamk_inst_out *sel);

/* ---- database frame (oslam_db.c); reqs / sels [db->n] or NULL: with the instance selection of every member ---- */
int oslam_db_align_frame(oslam_db *db, oslam_scene *s, float *T_out, oslam_stats *stats, const oslam_inst_req *reqs,
                         oslamk_inst_out *sels);

/* ---- refinement (oslam_refine.c) ---- */
/* rp NULL = defaults; checks them as oslam_refine does, *out = the parameters in force */
int oslam_refine_check_params(const oslam_refine_params *rp, oslam_refine_params *out);
/* finite, rotation orthonormal to 1e-3 with determinant > 0, last row 0 0 0 1: the pose check of every stage */
int oslam_refine_check_rigid(const float T[16]);
/* members ms[0 .. n) with T_in [n][16] (all-zero = skipped) against s, one set of launches; member j's result is
 * oslam_refine's for it alone */
int oslam_refine_members(oslam_model *const *ms, size_t n, oslam_scene *s, const float *T_in, const oslam_refine_params *p,
                         float *T_out, oslam_refine_result *res);

/* ---- views and the checks every stage shares (oslam_verify.c; the arithmetic: oslam_rigid.h) ---- */
/* the model is usable and lives on the view's device */
int oslam_view_check_pair(const oslam_model *m, const oslam_view *v);
/* A list of n poses T [n][16] with their models, in two halves.  The first reads no handle: the count (hypotheses: in
 * 1..OSLAM_ARBITRATE_MAX_HYPOTHESES; otherwise any, a database's members), no NULL in ms (ms NULL: there are no
 * pointers yet) and every pose that is not all zero rigid.  The second reads them: the model of every such pose is
 * usable and on the view's device. */
int oslam_check_poses(oslam_model *const *ms, const float *T, size_t n, int hypotheses);
int oslam_check_handles(oslam_model *const *ms, const float *T, size_t n, const oslam_view *v);
/* 1 when a view of this size can be made for cam (0 otherwise, no error text): sides in 1..16384, finite intrinsics
 * with fx, fy > 0, 0 < z_min <= z_max finite; depth_scale > 0 and finite, max_jump >= 0 and finite where asked */
int oslam_view_camera_ok(const oslam_camera *cam, int width, int height, int with_depth_scale, int with_max_jump);
/* a view of this size for cam on device dev (bound by the caller) with its own z image, not yet written */
int oslam_view_new(int dev, int width, int height, const oslam_camera *cam, oslam_view **out);
/* the camera that renders a view like v */
void oslam_view_camera(const oslam_view *v, oslam_camera *cam);

/* ---- verification (oslam_verify.c) ---- */
/* vp NULL = defaults; checks them as oslam_verify does, *out = the parameters in force */
int oslam_verify_check_params(const oslam_verify_params *vp, oslam_verify_params *out);
/* *r's counts from the six class counts c[0 .. 6), and from them view_fitness, coverage and found under p */
void oslam_verify_fill_result(oslam_verify_result *r, const uint32_t *c, const oslam_verify_params *p);
/* the descriptor of one member: its cloud, the rows of T, tol = (float)((double)depth_tol * d_dist), its blocks */
void oslam_verify_set_member(oslamk_verify_member *d, const oslam_model *m, const float T[16], float depth_tol);
/* members ms[0 .. n) with T [n][16] (all-zero = skipped) against v, one set of launches; member j's result is
 * oslam_verify's for it alone */
int oslam_verify_members(oslam_model *const *ms, size_t n, const oslam_view *v, const float *T, const oslam_verify_params *p,
                         oslam_verify_result *res);

/* ---- tracking (oslam_track.c) ---- */
/* tp NULL = defaults; checks them as oslam_track does, *out = the parameters in force */
int oslam_track_check_params(const oslam_track_params *tp, oslam_track_params *out);
/* gives back the view's maps; called by oslam_view_destroy with the view's device bound */
void oslam_track_release_maps(oslam_view *v);
/* gives back the pinned record of the tracking stage; called by oslam_release_scratch */
void oslam_track_release(void);
/* the view's maps for another stage: built when they do not exist yet (enqueued on the stream, *built = 1), with the
 * view's device bound */
int oslam_track_view_maps(oslam_view *v, int *built);
/* gives back the pinned state of the camera motion stage (oslam_ego.c); called by oslam_release_scratch */
void oslam_ego_release(void);
/* ep NULL = defaults; checks them as oslam_view_egomotion does, *out = the parameters in force (oslam_ego.c) */
int oslam_ego_check_params(const oslam_egomotion_params *ep, oslam_egomotion_params *out);
/* a pyramid schedule: every stride of p is 1, 2 or 4 and names a level (its log2) below n_levels, the levels of the
 * pyramids it runs on (UINT_MAX while they cannot be read yet: the strides alone) */
int oslam_ego_check_pyramid_schedule(const oslam_egomotion_params *p, unsigned n_levels);
/* one level of an egomotion schedule: its views and the stride of its lattice over the source */
typedef struct oslam_ego_pair {
    oslam_view *src, *dst;
    unsigned lattice;
} oslam_ego_pair;
/* the schedule of p (checked) from T0 with pair[l] as level l's views, all on one device: oslam_view_egomotion's call
 * from the upload to the result (oslam_ego.c) */
int oslam_ego_run(const oslam_ego_pair *pair, const float T0[16], const oslam_egomotion_params *p, float T_out[16],
                  oslam_egomotion_result *res);
/* ---- image pyramid (oslam_pyramid.c) ---- */
/* pp NULL = defaults; checks them as oslam_pyramid_create does, *out = the parameters in force */
int oslam_pyramid_check_params(const oslam_pyramid_params *pp, oslam_pyramid_params *out);
/* ---- the volume lock (oslam_volume.c, with its place in the lock order) ---- */
void oslam_volume_lock(void);
void oslam_volume_unlock(void);
/* the bytes of one buffer of the volume, computed in size_t */
static inline size_t oslam_volume_bytes(const oslam_volume_params *p)
{
    return (size_t)p->nx * (size_t)p->ny * (size_t)p->nz * sizeof(uint32_t);
}
/* oslam_volume_integrate after its argument checks; with c (a view with colour, checked against v by the caller) the
 * colour pass follows in the same call: one more launch, *coloured = the voxels it updated (oslam_volume.c) */
int oslam_volume_integrate_views(oslam_volume *vol, const oslam_view *v, const oslam_view *c, const float T_vol_cam[16],
                                 oslam_integrate_result *res, uint32_t *coloured);
/* gives back the view's colour image; called by oslam_view_destroy with the view's device bound (oslam_colour.c) */
void oslam_colour_release_view(oslam_view *v);
/* ---- surface and mesh extraction (oslam_surface.c) ---- */
/* sp NULL = defaults; checks them as oslam_volume_surface does, *out = the parameters in force */
int oslam_surface_check_params(const oslam_surface_params *sp, oslam_surface_params *out);
/* the volume's surface in HBM as [*np][6] (NULL without points) on device *dev; the caller frees the block
 * (oslam_dev_free).  Takes the volume lock for the extraction */
int oslam_volume_surface_cloud(oslam_volume *vol, unsigned min_weight, int *dev, float **d_pts6, uint32_t *np);
/* ---- the surface of the whole map (oslam_world_surface.c) ---- */
struct oslam_world_stage;
/* a pinned staging buffer of a voxel store with room for bytes, with the store's lock held (oslam_window.c) */
int oslam_world_stage_fit(struct oslam_world_stage *st, size_t bytes);
/* sp NULL = defaults; checks them as oslam_world_surface does, before any handle is read; *out = the parameters in force */
int oslam_world_surface_check_params(const oslam_world_surface_params *sp, oslam_world_surface_params *out);
/* the map's surface in HBM as [*np][6] (NULL without points) on device *dev; the caller frees the block (oslam_dev_free).
 * p: checked parameters.  Takes the volume lock and the store's for the extraction */
int oslam_world_surface_cloud(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *p, int *dev, float **d_pts6,
                              uint32_t *np);
/* The whole map on the device for one extraction (oslam_world_surface.c): the table of brick keys and slots, the store's
 * bricks sent up and the window's words written into theirs (include/oslam.h at oslam_world_surface, "Cost").  bricks == 0
 * is an empty map, for which no device call was made.  p: checked parameters.  plane picks what the brick array holds:
 * the TSDF words, or the colour words of a colour store and a coloured volume (the caller has checked both), laid out and
 * united the same way (include/oslam.h at oslam_world_colours).  Called with the volume lock and the
 * store's held; refuses a volume the store was not made for.  On failure nothing is left to free; after success the
 * caller waits for the stream and then calls oslam_world_map_close */
typedef struct oslam_world_map {
    oslamk_brick_map m;
    uint8_t *d_map;
    uint32_t bricks, window_bricks, launches;
    int32_t anchor[3];
    int dev;
} oslam_world_map;
enum { OSLAM_MAP_TSDF = 0, OSLAM_MAP_COLOUR = 1 };
int oslam_world_map_open(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *p, int plane, void *stream,
                         oslam_world_map *out);
void oslam_world_map_close(oslam_world_map *wm);
/* the arbitration's parameter check (oslam_arbitrate.c) */
int oslam_arbitrate_check_params(const oslam_arbitrate_params *ap, oslam_arbitrate_params *out);

/* the tile of an arbitration over ms / T [H] against v under p (include/oslam.h, "Tile"): the explain stage's too */
int oslam_arbitrate_choose_tile(oslam_model *const *ms, const float *T, size_t H, const oslam_view *v,
                                const oslam_arbitrate_params *p);
/* rp NULL = defaults; checks them as oslam_render_create does, *out = the parameters in force (oslam_render.c) */
int oslam_render_check_params(const oslam_render_params *rp, oslam_render_params *out);

/* gives back the pinned record of the arbitration stage (oslam_arbitrate.c); called by oslam_release_scratch */
void oslam_arbitrate_release(void);

#endif /* OSLAM_INTERNAL_H */
