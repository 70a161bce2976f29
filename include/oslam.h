/*
 * oslam.h -- C-ABI of the MI355X-native PPF registration path
 * (liboslam_hip.so).  Plain C: opaque handles, plain pointers and sizes, every
 * function returns an int status (0 = OSLAM_OK).  Nothing here exits the
 * process (the reference's HANDLE_ERROR does, include/impl/util.hpp:18-26).
 *
 * Each entry point names the reference interface it replaces; paths are
 * relative to the reference's pcl/alignment/.  INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * Clouds are passed as two float pointers (first coordinate of the first
 * point, first component of the first normal) plus a byte stride between
 * consecutive points, so a pcl::PointCloud<pcl::PointNormal> (48-byte points,
 * xyz at +0, normal at +16) is passed without a copy:
 *     xyz = &cloud[0].x, nrm = &cloud[0].normal_x, stride_bytes = 48.
 * Tightly packed float[n][3] arrays use stride_bytes = 12.  Host pointers.
 */
#ifndef OSLAM_H
#define OSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSLAM_OK 0
#define OSLAM_E_INVALID 1     /* bad argument (NULL, n == 0, d_dist <= 0, mismatching d_dist ...) */
#define OSLAM_E_DEVICE 2      /* HIP error; see oslam_last_error() */
#define OSLAM_E_NOMEM 3
#define OSLAM_E_NO_VOTES 4    /* no scene pair matched the model: T is all zeros */
#define OSLAM_E_LIMIT 5       /* cloud exceeds an encoding limit (see oslam_model_create) */
#define OSLAM_E_PEER 6        /* multi-GPU: another rank failed; every rank abandoned the registration together */

/* Per-vote arithmetic of the alpha angle (reference src/cuda/kernel.cu:302-342). */
#define OSLAM_VOTE_EXACT 0    /* accumulator identical to the reference's: alpha from quantised angles,
                               * re-evaluated with the reference's float sequence near bin edges */
#define OSLAM_VOTE_FAST 1     /* quantised angles only (Drost's alpha_scene - alpha_model), nothing
                               * re-evaluated: a vote's bin can differ from the reference's only when the
                               * reference's alpha lies within 3.1e-5 bin of an edge, and then it is the
                               * bin across that edge.  A vector that is zero, not finite or outside
                               * 2^-40..2^40 counts as angle 0 (atan2 + pi = 0) on either side, model
                               * or scene; exact mode gives the reference's bin for those votes too */

/* Flags of the reference's CLI that reach the path (src/alignment.cpp:119-172)
 * plus this build's extensions.  oslam_params_default() fills the reference's
 * defaults. */
typedef struct oslam_params {
    unsigned ref_point_df;         /* --ref_point_df, default 1 */
    float vote_count_threshold;    /* --vote_count_threshold, default 0.4 */
    int cpu_clustering;            /* --cpu_clustering, default 0 */
    int use_l1_norm;               /* --use_l1_norm, default 0 */
    int use_averaged_clusters;     /* --use_averaged_clusters, default 0 */
    int dev;                       /* --dev: device = min(numDevices-1, dev) (src/cuda/ppf.cu:45); default 0 */
    /* extensions */
    int vote_mode;                 /* OSLAM_VOTE_EXACT (default) or OSLAM_VOTE_FAST */
    int shard_rank;                /* scene reference points r = df*(rank + world*t); default 0 */
    int shard_world;               /* default 1 */
    unsigned max_cells;            /* initial capacity of the peak-record buffer, default 1<<22; it grows (to at most
                                    * 2^28 records) when more cells than that lie above the threshold */
    unsigned pose_gpu_min;         /* peak records from which the pose tail runs on the device; 0 = default (4096).  Both
                                    * tails give identical results; tests force either one */
    int no_bucket_spread;          /* model build: skip the pass that orders every bucket for the LDS banks (A/B
                                    * measurements; the accumulators do not depend on the order) */
    unsigned scratch_gib;          /* limit of the device's hit-list pool in GiB; 0 = default (4).  A registration
                                    * whose lists need more runs in batches of reference points */
    int pose_two_sorts;            /* device pose tail: order the kept cells with two stable sorts of (code, count) pairs even
                                    * when their fields fit one packed 64-bit key (the path clouds of 2^28 points with
                                    * 2^32 votes per cell take; identical results, tests force it) */
    int vote_order;                /* how the vote kernel's work is handed out (A/B measurements and tests; the results do not
                                    * depend on it): 0 (default) largest first -- a model's keys are numbered by descending
                                    * bucket weight and the reference points of a batch go out by descending demand; 1 neither
                                    * (keys numbered in union-slot order, reference points in index order); 2 the key numbers
                                    * alone; 3 the reference points alone.  A model takes its numbering when it is built or
                                    * loaded, a database group from its first member */
    int reserved[1];
} oslam_params;

/* Counters the reference logs at debug level (model.cu:122,152,161-168;
 * util.hpp:46) plus timings; all exact integers. */
typedef struct oslam_stats {
    uint64_t num_scene_ppfs;       /* valid ordered scene pairs (reference point r, i != r) on this shard */
    uint64_t num_hits;             /* of those, pairs whose key is in the model table */
    uint64_t num_votes;            /* accumulator increments = num_nonunique_votes */
    uint64_t num_unique_votes;     /* non-empty accumulator cells */
    uint64_t num_model_keys;       /* num_bins of the model table (counts the key-0 self-pair bucket) */
    uint64_t num_top;              /* cells with count > threshold * max */
    uint32_t max_count;            /* largest cell */
    uint32_t num_emitted;          /* records the vote kernel wrote before the final filter */
    float ms_vote;                 /* scene-key, hit-sort and vote kernels of the call, HIP events on the launch stream */
    float ms_total;                /* whole oslam_align call, host clock */
    uint32_t vote_launches;        /* launches of the vote kernel (one per batch of reference points) */
    float ms_vote_kernel;          /* sum over the vote-kernel launches alone (HIP events around each) */
    float ms_key_kernel;           /* sum over the scene-key and hit-sort kernel launches */
    uint32_t wide_workgroups;      /* vote workgroups (reference point x table slice) whose 16-bit counters overflowed and
                                    * were voted again with 32-bit counters (0 unless both clouds hold large planes) */
    uint64_t num_pairs_probed;     /* of num_scene_ppfs, the pairs whose distance bin can reach a model key: they are keyed
                                    * and probed; the others cannot hit and are dropped by the distance test alone */
    uint64_t scratch_bytes;        /* size of the device's hit-list pool after this call */
    uint64_t num_entries_streamed; /* model pair entries the vote kernel read: bucket lengths summed over (run of hits, table slice) */
    uint64_t num_items;            /* (run of hits, table slice) pairs with a bucket = buckets streamed */
} oslam_stats;

/* One accumulator peak: code = s_r << 32 | m_r << 6 | alpha_idx (kernel.cu:549). */
typedef struct oslam_cell {
    uint64_t code;
    uint32_t count;
    uint32_t pad;
} oslam_cell;

typedef struct oslam_model oslam_model;
typedef struct oslam_scene oslam_scene;

/* Reference defaults (src/alignment.cpp:119-172). */
int oslam_params_default(oslam_params *p);

/* d_dist = tau_d * max bounding-box extent (src/alignment.cpp:246-253). */
int oslam_d_dist_from_cloud(const float *xyz, size_t n, size_t stride_bytes, float tau_d,
                            float *d_dist_out);

/* Model::Model (include/model.h:17-19, src/cuda/model.cu:43-82): uploads the
 * cloud, computes all M*(M-1) pair features and builds the HBM-resident hash
 * table.  Limits: 2 <= n <= 46340 (the reference's own 32-bit pair index,
 * kernel.cu:433).  params may be NULL (defaults). */
int oslam_model_create(const float *xyz, const float *nrm, size_t n, size_t stride_bytes,
                       float d_dist, const oslam_params *params, oslam_model **out);
void oslam_model_destroy(oslam_model *m);

/* Persistent model database (the reference rebuilds every model for every scene, src/cuda/ppf.cu:57-70;
 * its own comment at :64-66 asks for this): oslam_model_save writes the built table -- cloud, slice
 * tables, union table, reachable-distance bitset, pair entries, point weights -- to one file;
 * oslam_model_load maps it back into HBM without recomputing a pair.  The file is tied to the
 * table layout version and to the vote mode it was built with (a fast-mode table has no exact
 * entries); a mismatch or a damaged file is OSLAM_E_INVALID.  params (may be NULL) supplies the
 * run-time flags of the loaded model (device, clustering flags, threshold); the table fields of
 * the file win. */
int oslam_model_save(const oslam_model *m, const char *path);
int oslam_model_load(const char *path, const oslam_params *params, oslam_model **out);
/* size of a built model: points, d_dist and the bytes its table holds in HBM (any pointer may be NULL) */
int oslam_model_info(const oslam_model *m, size_t *n_points, float *d_dist, uint64_t *table_bytes);

/* Model::SetModelPointVoteWeights (include/model.h:22); weights[n], default all 1. */
int oslam_model_set_point_weights(oslam_model *m, const float *weights, size_t n);

/* Scene::Scene (include/scene.h:15-16, src/cuda/scene.cu:24-55).  d_dist must
 * equal the d_dist of the model it is aligned with (src/cuda/ppf.cu:64-67), or be 0: the
 * reference discretises the scene's pair features with d_dist when the Scene is built, here the
 * scene holds points and reference frames only, so one scene with d_dist 0 serves a database of
 * models with different d_dist (the pair keys are made per model inside oslam_align). */
int oslam_scene_create(const float *xyz, const float *nrm, size_t n, size_t stride_bytes,
                       float d_dist, unsigned ref_point_downsample_factor,
                       const oslam_params *params, oslam_scene **out);
void oslam_scene_destroy(oslam_scene *s);

/* Model::ppf_lookup + result extraction (model.cu:269-306, ppf.cu:74-93):
 * T_rowmajor receives the best model->scene pose.  stats may be NULL. */
int oslam_align(oslam_model *m, oslam_scene *s, float T_rowmajor[16], oslam_stats *stats);

/* Optional: everything oslam_align would allocate on first use for this pair (the scratch pool of the
 * device -- mapping 32 GiB takes about a second -- and the frame tables of the device pose tail), done
 * ahead of time so that the first registration is as fast as the following ones. */
int oslam_align_prepare(oslam_model *m, oslam_scene *s);

/* Model database: what the loop of src/cuda/ppf.cu:57-100 becomes when the models stay resident.  The
 * database borrows the models (destroy it before them).  Models that share d_dist, device and vote mode
 * form a group with one union table of pair keys: per frame the scene pass (pair keys, probe, hit sort)
 * runs once per group instead of once per model, and every member votes from the same hit lists with
 * its own buckets.  Models with a d_dist of their own are groups of one.  A database made with ONE
 * d_dist for all models (the scene then also needs one voxel grid only) gets the whole benefit.
 * oslam_db_align: T_out[j*16..] = pose of model j (zeros when nothing matched), stats[j] (may be NULL)
 * its counters; in a group of several, num_hits counts the pairs whose key is in ANY member and the
 * kernel times are the group's, shared out evenly. */
typedef struct oslam_db oslam_db;
int oslam_db_create(oslam_model *const *models, size_t n, oslam_db **out);
void oslam_db_destroy(oslam_db *db);
/* the same, for a caller that destroys the models right afterwards: the members do not get their own key
 * tables back (they cannot be aligned any more, only destroyed) */
void oslam_db_destroy_with_models(oslam_db *db);
int oslam_db_align(oslam_db *db, oslam_scene *s, float *T_out, oslam_stats *stats);
int oslam_db_size(const oslam_db *db, size_t *n_models, size_t *n_groups);

/* ppf_registration (include/ppf.h:9-15, src/cuda/ppf.cu:29-106): every scene
 * against every model; T_out[(i*n_models + j)*16 ..] = pose of model j in
 * scene i.  model_weights is accepted and ignored, as in the reference
 * (ppf.cu:35).  Unlike the reference this does not reset the device. */
int oslam_ppf_registration(const float *const *scene_xyz, const float *const *scene_nrm,
                           const size_t *scene_n, size_t n_scenes, const float *const *model_xyz,
                           const float *const *model_nrm, const size_t *model_n, size_t n_models,
                           size_t stride_bytes, const float *model_d_dists,
                           unsigned ref_point_downsample_factor, float vote_count_threshold,
                           int cpu_clustering, int use_l1_norm, int use_averaged_clusters, int devUse,
                           const float *model_weights, float *T_out);

/* ht_dist (include/linalg.h:7, src/cuda/linalg.cu:9-20): out = {|dt|, |angle|}. */
int oslam_ht_dist(const float A[16], const float B[16], float out[2]);

/* voxelGridDownsample (src/alignment.cpp:79-87, applied to scenes with leaf = scene_leaf_size
 * and to models with leaf = d_dist, :265-288; pcl/voxel_grid/voxel_grid.cpp:18-21): one output
 * point per occupied voxel = mean of the points (and of their normals, not renormalised) in
 * it, in ascending voxel index -- pcl::VoxelGrid's algorithm with the point order inside a
 * voxel fixed to the input order.  xyz_out / nrm_out: packed float[cap][3]; *n_out receives the
 * number of voxels (OSLAM_E_LIMIT if it exceeds cap or the voxel count overflows int32). */
int oslam_voxel_grid(const float *xyz, const float *nrm, size_t n, size_t stride_bytes, float leaf,
                     int dev, float *xyz_out, float *nrm_out, size_t cap, size_t *n_out);

/* Depth image -> scene cloud with normals: the front end of a streaming configuration (a range camera
 * feeding the PPF path; the reference takes finished clouds from KinFu, README.md:5-8, and has no code
 * for this step -- the specification is oracle/oracle_depth.c).  Pinhole camera, z along the optical
 * axis: z = raw * depth_scale, valid in [z_min, z_max]; normals from the four axis neighbours (all
 * valid and within max_jump of z), unit length, facing the camera.  Pixels without a normal are
 * dropped; the rest come out in row-major pixel order.  depth: host image, uint16 (depth_is_u16 != 0)
 * or float, width x height.  xyz_out / nrm_out: packed float[cap][3]. */
typedef struct oslam_camera {
    float fx, fy, cx, cy;          /* pixels */
    float depth_scale;             /* raw unit -> metres (0.001 for millimetre images) */
    float z_min, z_max;            /* metres */
    float max_jump;                /* metres: no normal across a larger depth step */
} oslam_camera;
int oslam_depth_to_cloud(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam,
                         int dev, float *xyz_out, float *nrm_out, size_t cap, size_t *n_out);

/* The streaming chain in one call: depth image -> points + normals -> voxel grid (leaf > 0; 0 skips
 * it) -> scene, with the full-resolution cloud staying in HBM between the stages (only the image goes
 * up and the voxel-gridded cloud comes back for the host's reference frames).  Equivalent to
 * oslam_depth_to_cloud + oslam_voxel_grid + oslam_scene_create with the same arguments.  *n_points_out
 * (may be NULL) = points of the scene.  OSLAM_E_INVALID if fewer than 2 points remain. */
int oslam_scene_from_depth(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam,
                           float leaf, float d_dist, unsigned ref_point_downsample_factor,
                           const oslam_params *params, oslam_scene **out, size_t *n_points_out);

/* PLY clouds with normals (host only): pcl::io::loadPLYFile<pcl::PointNormal>
 * (src/alignment.cpp:212,241) / pcl::PLYWriter (pcl/voxel_grid/voxel_grid.cpp:27-29).
 * Reads ascii and binary_little_endian; needs x y z and nx ny nz (or normal_x normal_y
 * normal_z).  *xyz_out, *nrm_out: malloc'd packed float[n][3], release with oslam_free. */
int oslam_ply_read(const char *path, float **xyz_out, float **nrm_out, size_t *n_out);
int oslam_ply_write(const char *path, const float *xyz, const float *nrm, size_t n, int binary);
void oslam_free(void *p);

/* ---- host stage (no GPU needed): accumulator peaks -> poses -> clustering.
 * Counterparts: trans_calc_kernel2, vote_weight_kernel, mat2transquat_kernel,
 * trans2idx_kernel, rot_clustering_kernel (src/cuda/kernel.cu:605-782),
 * Model::ClusterTransformations / ClusterTransformationsCPU (src/cuda/model.cu:202-266),
 * clusterPoses (src/transformation_clustering.cpp:62-137), extraction (src/cuda/ppf.cu:74-93).
 * xyz/nrm here are packed float[n][3]. */
void oslam_build_T_g(const float p[3], const float n[3], float T_rowmajor[16]);
void oslam_sort_cells(oslam_cell *cells, size_t n);                 /* count desc, code asc */
size_t oslam_filter_cells(oslam_cell *cells, size_t n, float vote_count_threshold, uint32_t max_count);
int oslam_pose_stage(const oslam_cell *cells, size_t n, const float *m_xyz, const float *m_nrm,
                     size_t M, const float *s_xyz, const float *s_nrm, size_t S, float d_dist,
                     int cpu_clustering, int use_l1_norm, int use_averaged_clusters,
                     const float *model_point_weights, float T_rowmajor[16], float *poses_out);

/* The other result fields of the reference's Model after ppf_lookup (include/model.h:100-113, read by
 * src/cuda/ppf.cu:74-93) for the cells oslam_last_cells returns, recomputed on the host from those cells
 * (the same arithmetic as the registration itself): trans_out [n][3] = transformation_trans (after the
 * clustering stage, i.e. averaged when use_averaged_clusters), rots_out [n][4] = transformation_rots
 * (w, x, y, z, kernel.cu:124-144), vote_counts_out [n] = the clustered scores, *max_idx_out = max_idx.
 * With cpu_clustering the reference fills cpu_transformations instead: vote_counts_out[0] = votes of the
 * winning cluster, its pose is the T of oslam_align.  s: the scene of that registration.  Any output may be
 * NULL; at most cap cells are written, *n_out = their number. */
int oslam_last_result(oslam_model *m, oslam_scene *s, float *trans_out, float *rots_out, float *vote_counts_out,
                      size_t cap, size_t *n_out, uint32_t *max_idx_out);
int oslam_pose_stage_ex(const oslam_cell *cells, size_t n, const float *m_xyz, const float *m_nrm,
                        size_t M, const float *s_xyz, const float *s_nrm, size_t S, float d_dist,
                        int cpu_clustering, int use_l1_norm, int use_averaged_clusters,
                        const float *model_point_weights, float T_rowmajor[16], float *poses_out,
                        float *trans_out, float *rots_out, float *scores_out, uint32_t *max_idx_out);

/* ---- multi-GPU: scene reference points shard across ranks (one process per GPU;
 * params.shard_rank / shard_world at oslam_scene_create), model tables replicated.  The reference
 * has no multi-GPU code (src/cuda/ppf.cu:45 picks one device); its one call does everything
 * (include/ppf.h:9-15), and so does oslam_align_multi.
 *
 * RCCL form.  oslam_comm wraps an RCCL communicator: rank 0 makes an id (oslam_comm_unique_id),
 * hands its OSLAM_COMM_ID_BYTES bytes to the other ranks by any means (MPI, a file, a
 * torch.distributed broadcast), every rank calls oslam_comm_create.  oslam_align_multi = this
 * rank's votes, all-reduce(MAX) of the vote maxima (the threshold is global, model.cu:164-170),
 * all-gather of the peak records above the global threshold -- device buffers end to end, exact
 * sizes, nothing truncated -- and the pose tail on the union; every rank returns the same pose. */
typedef struct oslam_comm oslam_comm;
#define OSLAM_COMM_ID_BYTES 128
int oslam_comm_unique_id(void *id_out);
int oslam_comm_create(const void *id, int rank, int world, int dev, oslam_comm **out);
void oslam_comm_destroy(oslam_comm *c);
int oslam_align_multi(oslam_model *m, oslam_scene *s, oslam_comm *c, float T_rowmajor[16], oslam_stats *stats);
/* Failure is collective: when one rank cannot go on between two collectives (no memory, too many
 * peaks, a failed kernel) an error word travels with the next collective and EVERY rank returns --
 * the failing one with its own code, the others with OSLAM_E_PEER; nobody is left waiting.  A
 * collective that fails itself aborts the communicator (ncclCommAbort): the handle then refuses
 * further calls (OSLAM_E_DEVICE) and a new one has to be made.
 *
 * Loopback communicator: `world` emulated ranks that share ONE device inside one process (one
 * thread per rank calls oslam_align_multi with its own model, scene shard and handle out[r]).  The
 * collectives become device-to-device copies between pthread barriers (which time out instead of
 * hanging).  It runs the same exchange code as RCCL does -- that is its purpose: the N > 1 state
 * machine can be executed, and its failure paths injected, on a box with one GPU. */
int oslam_comm_create_loopback(int world, int dev, oslam_comm **out /* [world] */);
int oslam_comm_info(const oslam_comm *c, int *rank, int *world, int *broken);
/* gives the communicator up without waiting for anybody (ncclCommAbort): for a rank that cannot take part in an
 * exchange its peers have entered or will enter.  The handle refuses every later call; peers that use the
 * loopback transport are released with an error, RCCL peers stay in their collective until they abort too. */
int oslam_comm_abort(oslam_comm *c);
/* test tap: the next exchange on this handle fails locally at `stage` (1 = after the votes, 2 = while
 * selecting the survivors, 3 = while growing the record buffer), as an allocation failure would.
 * oslam_db_align_multi honours stage 1 (after this rank's registrations); either call clears the tap */
int oslam_comm_inject_failure(oslam_comm *c, int stage);

/* A database split by MODEL instead of by reference point (SURVEY 8e's alternative; what the scenes x models
 * loop of src/cuda/ppf.cu:57-100 becomes on several GPUs when the database is large): model j of n_total lives
 * on rank j % world, `db` holds this rank's models in that order (j = rank, rank + world, ...; may be NULL on a
 * rank without models), `s` is the WHOLE scene (no reference-point shard).  Every rank registers its models
 * (oslam_db_align), then one all-gather of 17 floats per model through the communicator gives every rank all
 * poses: T_out[j*16..] for j < n_total, found_out[j] (may be NULL) = 1 when model j produced a pose, 0 when
 * nothing matched.  No exchange on the vote path. */
int oslam_db_align_multi(oslam_db *db, oslam_scene *s, oslam_comm *c, size_t n_total, float *T_out, int *found_out,
                         oslam_stats *stats_local);

/* Host-buffer form of the same exchange, for callers with their own transport (and the CPU tests
 * over gloo).  oslam_align_local runs this rank's votes and reports the number of peak records
 * above the LOCAL threshold in *n_out and the local maximum; the records stay with the model.  It
 * copies them to cells_out when they fit cap; when they do not, it copies the cap strongest and
 * returns OSLAM_E_LIMIT -- never a silent cut (cap 0 with cells_out NULL just asks for the
 * numbers and returns OSLAM_OK).  After the maxima have been exchanged, oslam_local_peaks hands
 * out the records above threshold * global_max (fewer); OSLAM_E_LIMIT with the needed number in
 * *n_out when cap is too small, call again.  Every rank, or rank 0, then calls
 * oslam_align_finish on the gathered union. */
int oslam_align_local(oslam_model *m, oslam_scene *s, oslam_cell *cells_out, size_t cap,
                      size_t *n_out, uint32_t *local_max_out, oslam_stats *stats);
int oslam_local_peaks(oslam_model *m, uint32_t global_max, oslam_cell *cells_out, size_t cap, size_t *n_out);
int oslam_align_finish(oslam_model *m, oslam_scene *s, const oslam_cell *cells, size_t n,
                       uint32_t global_max, float T_rowmajor[16], oslam_stats *stats);

/* ---- pose refinement and presence score (after oslam_align / oslam_db_align; the reference has no such stage,
 * Drost's method and SLAM++ follow the vote with ICP).  A voting pose is the centre of an accumulator bin (12 degree
 * angle bins, translation quantised by d_dist); this stage refines it by point-to-plane ICP against the scene cloud
 * and scores it by the share of model points that find a scene point near them.  Everything runs on the device of
 * the model and scene, on the library stream (oslam_set_stream).  Poses are row-major, model -> scene.
 *
 * Correspondence of model point i (p, n) under a float32 pose T = [R | t] at radius r:
 *     p'x = ((R00*px + R01*py) + R02*pz) + t0, likewise y, z; n' the same expression without t (all float32).
 *     A scene point (q, nq) qualifies when, with d = q - p', (dx*dx + dy*dy) + dz*dz <= r*r (r*r rounded to float)
 *     and (n'x*nqx + n'y*nqy) + n'z*nqz >= min_normal_dot.  The correspondence is the qualifying point with the
 *     smallest d*d; ties go to the lowest scene index.  The device reproduces this bit for bit.
 * Step (Gauss-Newton on the point-to-plane residual, radius max_corr_dist * d_dist of the model):
 *     c = the model centroid (mean of its points in double) transformed by the current pose, rounded to float;
 *     r_i = nq . (p'_i - q_i), J_i = [(p'_i - c) x nq, nq]; A = sum J^T J, b = -sum J^T r, summed in float per
 *     workgroup of 256 model points (fixed order) and in double across workgroups (index order).  Solve
 *     (A + mu I) x = b, mu = 1e-6 trace(A) / 6, by Cholesky in double; x = (omega, v).  Fewer than 6 correspondences
 *     (or a failed factorisation) stop the member with its pose kept.  Otherwise T <- [dR | c - dR c + v] T with
 *     dR = Rodrigues(omega), then the rotation is re-orthonormalised by Gram-Schmidt over its columns x, y, z.
 *     The pose stays in double between iterations; each iteration's correspondences use its float32 rounding.
 *     An applied step counts as an iteration; the member has converged when |omega| < stop_rot and
 *     |v| < stop_trans * d_dist, and stops at max_iterations.
 * Score: the correspondences at radius inlier_dist * d_dist are the inliers; fitness = inliers / model points,
 *     rmse = sqrt(sum d*d / inliers) (0 without inliers).  fitness_in is the score at T_in.  found = fitness >=
 *     min_fitness.  Model point weights do not enter.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers, parameters that are not
 * finite, max_corr_dist or inlier_dist <= 0, inlier_dist > max_corr_dist, max_iterations > 1000, and a T_in that is
 * not finite or not rigid (rotation orthonormal to 1e-3 with determinant > 0, last row 0 0 0 1) are OSLAM_E_INVALID.
 * The scene's d_dist may be 0 (a database scene); each model uses its own d_dist.
 * Cost: the scene gets a dense uniform grid (cell edge >= the largest correspondence radius of the call, enlarged so
 * that the grid has at most 2^24 cells), built on the device and cached on the scene (at most 4 grids, freed with it).
 * Kernels enqueued per call (res->launches): at most 2 * max_iterations + 2, plus 5 when the scene grid has to be
 * built; the same for 1 member and for 100.  Host synchronisations: at most 1 + max_iterations / 4 (an "all members
 * done" word is read after every 4th iteration; the call ends early when it is set). */
typedef struct oslam_refine_params {
    unsigned max_iterations;   /* default 30 */
    float max_corr_dist;       /* correspondence radius in units of the model's d_dist, default 2.0 */
    float min_normal_dot;      /* gate on (R n_model) . n_scene, default 0.8 */
    float inlier_dist;         /* radius of the score, in units of d_dist, default 0.5 (<= max_corr_dist) */
    float min_fitness;         /* found = fitness >= min_fitness; default 0.3 (on the seeded scenes of
                                * tests/test_refine_host.py a present model scores 0.33-0.60 after refinement, an
                                * absent one at most 0.25) */
    float stop_rot;            /* converged when |omega| < stop_rot (rad) ... default 1e-5 */
    float stop_trans;          /* ... and |v| < stop_trans * d_dist, default 1e-4 */
    int reserved[4];
} oslam_refine_params;

typedef struct oslam_refine_result {
    float fitness_in;          /* score at the input pose */
    float fitness;             /* inliers / model points at the returned pose */
    float rmse;                /* point-to-point RMS over the inliers, scene units */
    uint32_t inliers, correspondences, iterations;   /* correspondences: of the last step (radius max_corr_dist) */
    int32_t converged, found;
    uint32_t launches;         /* kernels this call enqueued (the whole call, shared by all members) */
    float ms_total;            /* whole call, host clock */
} oslam_refine_result;

int oslam_refine_params_default(oslam_refine_params *p);
/* rp may be NULL (defaults).  T_out receives the refined pose (T_in when the member stopped at once). */
int oslam_refine(oslam_model *m, oslam_scene *s, const float T_in[16], const oslam_refine_params *rp,
                 float T_out[16], oslam_refine_result *res);
/* Every member of the database in one set of launches: T_in / T_out [n][16], res [n] (n = members, in the order of
 * oslam_db_create).  A member whose T_in is all zeros (nothing matched in oslam_db_align) is skipped: T_out zeros,
 * found 0, iterations 0; the call still returns OSLAM_OK.  Member j's results equal oslam_refine of model j alone
 * bit for bit. */
int oslam_db_refine(oslam_db *db, oslam_scene *s, const float *T_in /* [n][16] */,
                    const oslam_refine_params *rp, float *T_out, oslam_refine_result *res /* [n] */);
/* test tap: idx_out[M] = scene index of each model point's correspondence under T at `radius` (scene units), -1 =
 * none */
int oslam_refine_correspondences(oslam_model *m, oslam_scene *s, const float T[16], float radius,
                                 float min_normal_dot, int32_t *idx_out);

/* ---- verification against a depth image: visibility-aware presence (after oslam_refine; Drost-style pipelines
 * re-score their hypotheses view by view after ICP).  A depth frame shows one side of an object, so the share of all
 * model points near the scene cloud (oslam_refine's fitness) cannot tell a present object from an absent one that
 * fits a part of it.  The image can: a model point that faces the camera should appear at its pixel's depth, and a
 * pixel that lies farther than the point contradicts the pose (the camera saw through the object).
 *
 * A view holds the depth image on the device as float z.  It shares the camera frame of oslam_depth_to_cloud (the
 * camera at the origin looking along +z, so the clouds of oslam_scene_from_depth are in the same coordinates), with
 * the same conventions: z = raw * depth_scale in float, valid in [z_min, z_max]; max_jump is remembered for the normal
 * map of the tracking stage (oslam_track) and not used by verification.  A view is independent of any scene: a point-cloud scene with a known sensor can be verified as well.
 *
 * Rule.  Model point i is (p, n); T is a float32 row-major model -> scene (camera) pose.  p' and n' are computed
 * exactly as oslam_refine does: p'x = ((R00*px + R01*py) + R02*pz) + t0, likewise y and z; n' the same without t.
 * tol = (float)((double)depth_tol * d_dist) with the model's d_dist.  Each point gets exactly one class, tested in
 * this order:
 *   0 BACK       (n'x*p'x + n'y*p'y) + n'z*p'z >= 0 (the surface faces away from the camera)
 *   1 OUT        p'z outside [z_min, z_max], or the pixel fu = floorf(((p'x*fx)/p'z + cx) + 0.5f), fv likewise with
 *                fy and cy, outside the image (0 <= fu < width, 0 <= fv < height, tested in float)
 *   2 SUPPORTED  some valid pixel z_o of the (2 window + 1)^2 pixels around (fu, fv), clipped to the image, has
 *                fabsf(z_o - p'z) <= tol
 *   3 OCCLUDED   otherwise some valid pixel of the window has z_o < p'z - tol (something nearer covers the point)
 *   4 CONFLICT   otherwise some valid pixel of the window exists (all lie farther: the camera saw through the object)
 *   5 UNKNOWN    no valid pixel in the window
 * Scores (float32 divisions of the counts converted to float; 0 when the denominator is 0):
 *   view_fitness = supported / (supported + conflict)   is what the camera saw consistent with the object?
 *   coverage = supported / (supported + occluded + conflict)   does the visible evidence cover it?  (A small absent
 *     model placed inside a present object has its facing points on the observed surface or behind it: a high
 *     view_fitness, a low coverage.)
 *   found = supported >= min_supported && view_fitness >= min_view_fitness && coverage >= min_coverage.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers, parameters that are
 * not finite, depth_tol <= 0, window > 3, ratios outside [0, 1] and a T that is not rigid (the test of oslam_refine)
 * are OSLAM_E_INVALID; so are a model and a view on different devices.
 * Cost: building a view uploads the image and runs one kernel (k_view_z).  A call enqueues one memset, one kernel
 * (k_verify: every member in one grid) and one copy back, with one host wait: launches == 1 for 1 member and for 100.
 * Integer counters only: the results are deterministic. */
typedef struct oslam_view oslam_view;
int oslam_view_create(const void *depth, int depth_is_u16, int width, int height, const oslam_camera *cam, int dev,
                      oslam_view **out);
int oslam_view_destroy(oslam_view *v);

#define OSLAM_VERIFY_BACK 0
#define OSLAM_VERIFY_OUT 1
#define OSLAM_VERIFY_SUPPORTED 2
#define OSLAM_VERIFY_OCCLUDED 3
#define OSLAM_VERIFY_CONFLICT 4
#define OSLAM_VERIFY_UNKNOWN 5

typedef struct oslam_verify_params {
    float depth_tol;           /* in units of the model's d_dist, default 1.0 */
    unsigned window;           /* half-width of the pixel window, 0..3, default 1 */
    float min_view_fitness;    /* default 0.92 } calibrated on the CPU on seeded depth frames with a 10-model database */
    float min_coverage;        /* default 0.5  } (tests/test_verify_host.py): present >= 0.935 / 0.509, absent <= 0.899 */
    unsigned min_supported;    /* default 50   } / 0.495; supported does not separate (present >= 116, absent up to 144):
                                *                it is a floor against a handful of chance agreements */
    int reserved[4];
} oslam_verify_params;

typedef struct oslam_verify_result {
    uint32_t back, out, supported, occluded, conflict, unknown;   /* they sum to the model's points */
    float view_fitness, coverage;
    int32_t found;
    uint32_t launches;         /* kernels this call enqueued (the whole call, shared by all members) */
    float ms_total;            /* whole call, host clock */
} oslam_verify_result;

int oslam_verify_params_default(oslam_verify_params *p);
/* vp may be NULL (defaults). */
int oslam_verify(oslam_model *m, const oslam_view *v, const float T[16], const oslam_verify_params *vp,
                 oslam_verify_result *res);
/* Every member in one set of launches: T [n][16] in oslam_db_create order, res [n].  A member whose T is all zeros is
 * skipped (zeros, found 0) and the call still returns OSLAM_OK.  Member j equals oslam_verify of model j bit for bit
 * (launches and ms_total aside). */
int oslam_db_verify(oslam_db *db, const oslam_view *v, const float *T, const oslam_verify_params *vp,
                    oslam_verify_result *res);
/* test tap: class_out[M] = the class of each model point (OSLAM_VERIFY_BACK .. OSLAM_VERIFY_UNKNOWN) */
int oslam_verify_classes(oslam_model *m, const oslam_view *v, const float T[16], const oslam_verify_params *vp,
                         uint8_t *class_out);

/* ---- every instance of a model in a scene (after the votes; the reference keeps only the best pose,
 * model.cu:292-295 / ppf.cu:74-93).  Single device only: oslam_align_multi / oslam_db_align_multi have no instance form.
 *
 * Candidates: the poses the clustering stage produces for the registration.
 *   Default clustering (also use_l1_norm, use_averaged_clusters): every kept cell's pose (oslam_last_cells order) with
 *     its translation replaced by the clustering-stage translation -- exactly as oslam_align builds its T -- scored by
 *     its clustered score (oslam_last_result's vote_counts).  Fewer than two kept cells give no candidate.
 *   cpu_clustering: the clusters of the greedy clustering, each with its pose (made as oslam_align makes the winner's)
 *     and its vote total as the score (as float); candidate index = the cluster's head (a kept-cell index).
 *   Candidate order: score descending, then candidate index ascending.
 * Same instance: with c = the model centroid (mean of its points in double, rounded to float) and E = the model's
 *   extent (its largest bounding-box side, as oslam_d_dist_from_cloud with tau 1), poses A and B are the same instance
 *   when both hold:
 *     p = ((R0*cx + R1*cy) + R2*cz) + t per row in float; d2 = (dx*dx + dy*dy) + dz*dz < sep2, where
 *     sep2 = float((double)min_separation * E, squared in double);
 *     and, unless max_angle == (float)pi, sum_ij A_ij*B_ij over the 3x3 blocks (row-major, in float from 0) >=
 *     float(1 + 2 cos((double)max_angle)).  max_angle == (float)pi (the default) makes it a translation-only test.
 * Selection: walk the candidates in order; accept one that is not the same instance as any accepted before; stop after
 *   max_instances acceptances, or at the first candidate whose score is < min_score_ratio * score(instance 0) (float).
 *   When instance 0's pose is all zeros (the (0,0,0) code) nothing is returned.  Hence: instance 0's pose is bit for
 *   bit the T of oslam_align for the same model, scene and params, and *n_out == 0 exactly when oslam_align returns an
 *   all-zero T or OSLAM_E_NO_VOTES (the same error code is returned then).  The pose tail runs on the device or the host
 *   as for oslam_align (on the device one more kernel, k_pose_instances, after the winner); the result is the same.
 * Refinement (rp != NULL): every accepted instance is refined with oslam_refine semantics in one set of launches;
 *   instance j's T and refine equal oslam_refine(m, s, T_vote_j, rp) bit for bit except launches and ms_total.  Then,
 *   in acceptance order, an instance that is the same instance (same rule, refined poses) as an earlier kept one is
 *   dropped -- two candidates that converged onto one object -- and then those with found == 0 unless keep_not_found.
 * Output: out[0 .. *n_out) in acceptance order.  oslam_last_cells / oslam_last_result afterwards report what they
 *   report after oslam_align.
 * Arguments are checked before any handle is read: NULL pointers, max_instances 0 or above OSLAM_MAX_INSTANCES,
 *   cap < max_instances, min_separation not finite or negative, max_angle outside [0, (float)pi], min_score_ratio
 *   outside [0, 1] are OSLAM_E_INVALID; the refinement parameters are checked as oslam_refine checks them.
 * Defaults: max_instances 8, min_separation 0.5, max_angle pi, min_score_ratio 0.5 (not tuned by a sweep).  Observed
 *   on one MI355X: on the seeded 2- and 3-copy scenes of tests/test_gpu_instances.py and tools/bench_configs.py
 *   instances, the second and third copies' winning candidates scored 0.77-0.97 of the best one and their centroids lay
 *   2 E and more apart; refined, every copy lay within 1e-3 E of its ground truth.
 * Cost (device tail): one more launch per model, k_pose_instances (one workgroup): 125 ms at 1.2e7 kept cells and 16
 *   rounds with min_score_ratio 0, immeasurable next to the rest at the 4e3-1.5e4 cells of the bench registrations. */
#define OSLAM_MAX_INSTANCES 64
typedef struct oslam_instance_params {
    unsigned max_instances;    /* 1..OSLAM_MAX_INSTANCES, default 8 */
    float min_separation;      /* centroid distance in units of the model's extent, default 0.5 */
    float max_angle;           /* radians, [0, pi], default pi (translation only) */
    float min_score_ratio;     /* [0, 1], default 0.5 */
    int keep_not_found;        /* keep refined instances with found == 0 */
    int reserved[4];
} oslam_instance_params;

typedef struct oslam_instance {
    float T[16];               /* refined pose when rp != NULL, else = T_vote */
    float T_vote[16];          /* the candidate's pose from the clustering stage */
    float score;               /* its clustered score (greedy clustering: cluster votes) */
    uint32_t candidate;        /* its index in the candidate order above (kept cell, or greedy head) */
    oslam_refine_result refine;   /* zeros when not refined */
} oslam_instance;

int oslam_instance_params_default(oslam_instance_params *p);
/* out[cap], cap >= max_instances */
int oslam_align_instances(oslam_model *m, oslam_scene *s, const oslam_instance_params *ip,
                          const oslam_refine_params *rp /* NULL: no refinement */, oslam_instance *out, size_t cap,
                          size_t *n_out, oslam_stats *stats);
/* out [n_models][cap], n_out [n_models], stats [n_models] (may be NULL): member j equals oslam_align_instances of
 * model j alone bit for bit (ms fields aside); a member without votes gets n_out 0 and the call goes on, as in
 * oslam_db_align.  One frame: the device tails of a group in flight together, then one refinement over every
 * instance of every member. */
int oslam_db_align_instances(oslam_db *db, oslam_scene *s, const oslam_instance_params *ip,
                             const oslam_refine_params *rp, oslam_instance *out, size_t cap, size_t *n_out,
                             oslam_stats *stats);
/* The selection on the host, no device: T [n][16] and scores [n] indexed by candidate index (any order of scores);
 * idx_out[cap] receives the accepted candidate indices in acceptance order. */
int oslam_select_instances(const float *T, const float *scores, size_t n, const float centroid[3], float extent,
                           const oslam_instance_params *ip, uint32_t *idx_out, size_t cap, size_t *n_out);

/* ---- arbitration: hypotheses that claim the same pixels of the depth image (after oslam_verify).  oslam_verify judges
 * every hypothesis on its own, so two database members whose facing sides coincide within the tolerance are both found
 * at one place.  No per-hypothesis threshold separates them; a comparison does: where both explain the image, which
 * one explains it better?
 *
 * Input: a view and H hypotheses (model, T), any mix of models and of several poses of one model, 1 <= H <=
 * OSLAM_ARBITRATE_MAX_HYPOTHESES.  A T of all zeros is a skipped hypothesis.  A caller that wants only verified
 * hypotheses to compete passes the others as zeros (oslam_db_detect does).
 * Claims.  Every model point of hypothesis h gets the class of oslam_verify (the same float sequence, window and
 *   tol = (float)((double)depth_tol * d_dist) with its model's d_dist).  A SUPPORTED point claims the tile of its pixel,
 *   t = (fv / tile) * tiles_x + fu / tile (integers, tiles_x = ceil(width / tile)), with its residual r = the smallest
 *   fabsf(z_o - p'z) over the valid pixels of its window (r <= tol), quantised to x = r * (65535.0f / tol) in float,
 *   q = x < 65535.0f ? (uint32_t)x : 65535.  Per (h, t): cnt = the claiming points, sum = the sum of their q.
 *   Integers: the table does not depend on the order of the points.  A model of 2^24 points or more is OSLAM_E_LIMIT.
 * Tile.  params.tile in pixels, 4..128; 0 (the default) chooses one for the call: with d_max = the largest d_dist of
 *   the hypotheses that are not skipped, c = the model centroid of the instance rule (oslam_align_instances),
 *   z_c = ((R20*cx + R21*cy) + R22*cz) + t2 in float and z_near = the smallest z_c > 0 of them,
 *   tile = ceil((((double)tile_spacing * d_max) * fx) / z_near), clamped to [4, 128]; 128 when no z_c is positive.
 *   About two point spacings in the image: with sparser tiles two hypotheses of the same surface hardly ever meet.
 * Ownership.  Among the live claimants of a tile (cnt >= 1) the owner has the smallest mean residual, compared exactly
 *   as sum_a * cnt_b < sum_b * cnt_a in 64-bit integers; ties go to the lower hypothesis index.  claimed(h) = tiles with
 *   cnt_h >= 1, owned(h) = those it owns, share(h) = (float)owned / (float)claimed.
 * Elimination.  Live at the start: every hypothesis that is not skipped and has claimed >= max(min_tiles, 1).  Repeat:
 *   ownership among the live ones; the loser is the live hypothesis with the smallest share (ties: the larger index);
 *   when share(loser) < min_owned_share it is suppressed -- suppressed_by = the other live hypothesis that owns most of
 *   the loser's claimed tiles (ties: the lower index) -- and no longer live; otherwise stop.  At most H rounds.
 *   A hypothesis that was never live has kept 0, suppressed_by -1, owned 0, share 0.
 * Result per hypothesis: claimed; owned and share at its elimination (kept ones: at the last round); mean_residual =
 *   (float)((((double)sum of its q / (double)its SUPPORTED points) / 65535.0) * (double)tol), 0 without claims; kept;
 *   suppressed_by (-1: not suppressed).  Per call: tile (as used), rounds (ownership computations), launches, ms_total.
 *   Only SUPPORTED points claim: the hidden part of an object behind another is OCCLUDED and claims nothing, so two
 *   real objects side by side or one behind the other both keep their own tiles but for a seam.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers, H == 0 or above the
 *   maximum, parameters that are not finite, depth_tol <= 0, window > 3, tile not 0 and outside 4..128, tile_spacing
 *   <= 0, min_owned_share outside [0, 1] and a T that is neither all zeros nor rigid (the test of oslam_refine) are
 *   OSLAM_E_INVALID; so are a model and a view on different devices.  A claims table above 256 MiB (H * tiles * 8 B)
 *   is OSLAM_E_LIMIT before anything is launched.
 * Cost: one memset, two kernels (k_claim: every hypothesis in one grid; k_arbitrate: one workgroup, the whole
 *   elimination) and one copy back of a 32-byte record per hypothesis, one host wait: launches == 2 for 2 hypotheses
 *   and for 400.  Integer counters only: the results are deterministic.
 * Defaults (calibration table: tests/test_arbitrate_host.py): tile 0, tile_spacing 2, min_tiles 4 (a floor against a
 *   handful of chance agreements, not calibrated), min_owned_share 0.52: the middle of the gap between the present
 *   model (>= 0.629) and its suppressed near twin (<= 0.421) on the frames where the rule separates them.  On one
 *   calibration frame in six it does not: the twin's pose fits better there and the present model is suppressed. */
#define OSLAM_ARBITRATE_MAX_HYPOTHESES 1024
typedef struct oslam_arbitrate_params {
    float depth_tol;           /* as oslam_verify_params, default 1.0 */
    unsigned window;           /* as oslam_verify_params, default 1 */
    unsigned tile;             /* pixels, 4..128; 0 (default): chosen from tile_spacing */
    float tile_spacing;        /* tile width in point spacings (d_dist) at the nearest hypothesis, default 2.0 */
    unsigned min_tiles;        /* a hypothesis with fewer claimed tiles does not take part, default 4 */
    float min_owned_share;     /* [0, 1]: the loser is suppressed below this share, default 0.52 */
    int reserved[4];
} oslam_arbitrate_params;

typedef struct oslam_arbitrate_result {
    uint32_t claimed, owned;
    float share, mean_residual;
    int32_t kept, suppressed_by;
    uint32_t tile, rounds;     /* the whole call, shared by all hypotheses */
    uint32_t launches;         /* kernels this call enqueued */
    float ms_total;            /* whole call, host clock */
} oslam_arbitrate_result;

int oslam_arbitrate_params_default(oslam_arbitrate_params *p);
/* models [H], T [H][16], res [H]; ap may be NULL (defaults).  When every hypothesis is skipped nothing is launched. */
int oslam_arbitrate(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                    const oslam_arbitrate_params *ap, oslam_arbitrate_result *res);
/* hypothesis j = member j of the database with T[j] (zeros: skipped); equals oslam_arbitrate on the same list */
int oslam_db_arbitrate(oslam_db *db, const oslam_view *v, const float *T, const oslam_arbitrate_params *ap,
                       oslam_arbitrate_result *res);
/* test tap: the table after k_claim, cnt_out [H][n_tiles] and sum_out [H][n_tiles] with n_tiles = ceil(width / tile) *
 * ceil(height / tile) of the tile in force (*tile_out); cap = the entries each array holds (OSLAM_E_INVALID when
 * H * n_tiles > cap; *n_tiles_out is set either way) */
int oslam_arbitrate_claims(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                           const oslam_arbitrate_params *ap, uint32_t *cnt_out, uint64_t *sum_out, size_t cap,
                           uint32_t *tile_out, size_t *n_tiles_out);
/* test tap: the elimination (k_arbitrate) alone over a table the caller gives, so that exact ties and large counts can
 * be put before it: cnt [H][n_tiles] (each below 2^24), sum [H][n_tiles] (each below 2^40), skipped [H] (non-zero: a
 * skipped hypothesis), packed into the words k_claim writes, on device 0.  res [H] as oslam_arbitrate fills it with
 * tol = 1 (mean_residual = (sum of q / points) / 65535) and tile 0; *rounds_out = rounds.  The checks of
 * oslam_arbitrate: NULL pointers, H == 0 or above the maximum, n_tiles == 0, min_owned_share not finite or outside
 * [0, 1] and an entry that does not fit its field are OSLAM_E_INVALID, a table above 256 MiB is OSLAM_E_LIMIT, before
 * any device call; when every hypothesis is skipped nothing is launched. */
int oslam_arbitrate_table(const uint32_t *cnt, const uint64_t *sum, const uint8_t *skipped, size_t H, size_t n_tiles,
                          unsigned min_tiles, float min_owned_share, oslam_arbitrate_result *res, uint32_t *rounds_out);

/* ---- the whole chain for a database frame in one call: oslam_db_align_instances (with refinement) -> the
 * verification of every instance (oslam_verify semantics, one set of launches) -> arbitration over all instances, those
 * that verification did not find passed as skipped -> the detections that are found and kept, ordered by (model,
 * instance).  It composes the stages: a detection's T, verify and arbitrate equal what the three calls return for the
 * same lists bit for bit (launches and ms fields aside).  The scene and the view are the same frame: the view in the
 * camera frame of the scene's cloud (oslam_scene_from_depth and oslam_view_create of one image).
 * dp may be NULL: the defaults of every stage, except that instances.keep_not_found is 1 -- a depth frame shows one side
 * of an object, refine's fitness stays below its threshold there and verification is the judge of
 * presence.  out [cap]; when more than cap detections are kept the call returns
 * OSLAM_E_LIMIT with *n_out = their number and out untouched. */
typedef struct oslam_detect_params {
    oslam_instance_params instances;
    oslam_refine_params refine;
    oslam_verify_params verify;
    oslam_arbitrate_params arbitrate;
    int reserved[4];
} oslam_detect_params;

typedef struct oslam_detection {
    uint32_t model, instance;  /* database member, and its index in the member's oslam_db_align_instances list */
    float T[16];               /* the refined pose */
    oslam_verify_result verify;
    oslam_arbitrate_result arbitrate;
} oslam_detection;

int oslam_detect_params_default(oslam_detect_params *p);
int oslam_db_detect(oslam_db *db, oslam_scene *s, const oslam_view *v, const oslam_detect_params *dp,
                    oslam_detection *out, size_t cap, size_t *n_out);

/* ---- tracking across depth frames: projective ICP against the image itself (after oslam_db_detect; KinFu's data
 * association).  A detection's pose is carried from frame to frame at a cost that does not depend on the database: no
 * scene cloud, no voxel grid, no neighbour grid and no votes.  Each model point looks at one pixel.
 *
 * Normals on the view.  A view gains a per-pixel vertex and normal map on the device, built on first use by one kernel
 * (k_view_normals) and kept with the view; a view that is never tracked on costs what it did.  The point and the normal
 * of a pixel are exactly what oslam_depth_to_cloud produces for it with the view's camera (max_jump included): the
 * back-projection, the four axis neighbours valid and within max_jump, the cross product normalised and turned to face
 * the camera, no normal for a zero or non-finite cross product -- bit for bit, so the clouds of oslam_scene_from_depth
 * and the tracker see one geometry.
 * Correspondence of model point i (p, n) under the float32 pose T: p' and n' exactly as oslam_refine and oslam_verify
 *   compute them.  The point takes part only when it is neither BACK nor OUT by oslam_verify's tests; its pixel is
 *   oslam_verify's (fu, fv); q and nq are that pixel's vertex and normal.  The correspondence exists when the pixel has
 *   a normal, (dx*dx + dy*dy) + dz*dz <= r*r with d = q - p' and r = max_corr_dist * d_dist (float, r*r rounded to
 *   float), and (n'x*nqx + n'y*nqy) + n'z*nqz >= min_normal_dot.  One candidate pixel per point, no search: the image
 *   is dense where the model cloud is sparse.
 * Step, convergence and pose bookkeeping are oslam_refine's with these correspondences: the same residual and Jacobian
 *   about the transformed centroid, the same 29 sums (float per block of 256 consecutive model points through the fixed
 *   tree, double across blocks in index order), the same damped Cholesky in double, Rodrigues step and Gram-Schmidt,
 *   "fewer than 6 correspondences (or a failed factorisation) stop the hypothesis with its pose kept", stop_rot and
 *   stop_trans.
 * Judgement.  At the final pose every hypothesis is classed and scored exactly as oslam_verify would be with
 *   params.verify: res->verify equals oslam_verify(model, view, T_out) bit for bit (launches and ms_total aside, which
 *   are this call's), res->found = res->verify.found.
 * Input: H hypotheses (model, T_prev) as in oslam_arbitrate, several instances of one model being several entries,
 *   1 <= H <= OSLAM_ARBITRATE_MAX_HYPOTHESES.  An all-zero T_prev is skipped: T_out zeros, result zeros, found 0.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers, H == 0 or above the
 *   maximum, parameters that are not finite, max_corr_dist <= 0, max_iterations > 1000, a negative stop criterion, the
 *   verify parameters as oslam_verify checks them and a T_prev that is neither all zeros nor rigid (the test of
 *   oslam_refine) are OSLAM_E_INVALID; so are a model and a view on different devices.
 * Cost: one kernel (k_track) and one host wait for the whole call, at any iteration count: one workgroup per hypothesis
 *   runs every iteration itself (per iteration: its model's blocks of 256 points, each with the transform, the
 *   projection and one gather of vertex and normal; the block sums in the fixed order, no float atomics; the blocks in
 *   double in index order; one thread solves the 6x6 system and publishes the new float32 pose through LDS), then
 *   classes and counts for the judgement and writes one record per hypothesis, which is copied to pinned memory.
 *   res->launches == 1 for 1 hypothesis and for 50; 2 on the first call on a view (k_view_normals).  The results are
 *   deterministic. */
typedef struct oslam_track_params {
    unsigned max_iterations;   /* default 10 */
    float max_corr_dist;       /* correspondence radius in units of the model's d_dist, default 2.0 */
    float min_normal_dot;      /* gate on (R n_model) . n_pixel, default 0.8 */
    float stop_rot;            /* as oslam_refine_params, default 1e-5 */
    float stop_trans;          /* as oslam_refine_params, default 1e-4 */
    oslam_verify_params verify;   /* the judgement at the final pose, defaults of oslam_verify */
    int reserved[4];
} oslam_track_params;

typedef struct oslam_track_result {
    oslam_verify_result verify;   /* oslam_verify at T_out */
    uint32_t iterations, correspondences;   /* correspondences: of the last step */
    int32_t converged, found;  /* found = verify.found */
    uint32_t launches;         /* kernels this call enqueued (the whole call, shared by all hypotheses) */
    float ms_total;            /* whole call, host clock */
} oslam_track_result;

int oslam_track_params_default(oslam_track_params *p);
/* models [H], T_prev / T_out [H][16], res [H] (may be NULL); tp may be NULL (defaults) */
int oslam_track(oslam_model *const *models, const float *T_prev, size_t H, const oslam_view *v,
                const oslam_track_params *tp, float *T_out, oslam_track_result *res);
/* hypothesis h = member member[h] of the database (an index below its size) with T_prev[h]; equals oslam_track on the
 * same list */
int oslam_db_track(oslam_db *db, const uint32_t *member, const float *T_prev, size_t H, const oslam_view *v,
                   const oslam_track_params *tp, float *T_out, oslam_track_result *res);
/* test taps.  The maps of a view (built when they do not exist yet), width * height entries in row-major pixel order:
 * nrm_out [h*w][3] / vtx_out [h*w][3] (zeros where the pixel has no normal), has_normal_out [h*w] 0 or 1 */
int oslam_view_normals(oslam_view *v, float *nrm_out, uint8_t *has_normal_out);
int oslam_view_vertices(oslam_view *v, float *vtx_out);
/* pixel_out[M] = v * width + u of each model point's correspondence under T, -1 = none */
int oslam_track_correspondences(oslam_model *m, const oslam_view *v, const float T[16], float max_corr_dist,
                                float min_normal_dot, int32_t *pixel_out);

/* ---- a tracker over the stages: identity across frames.  A host-side object with no kernel of its own.
 * One oslam_tracker_step does, in this order:
 *   1. oslam_db_track once over all live tracks from their last poses;
 *   2. arbitration (oslam_arbitrate, params.arbitrate) over the tracks that were found, the others passed as skipped:
 *      two tracks that slid onto one object must not both live; a suppressed track counts as not found;
 *   3. a track that was found: its pose becomes T_out, hits + 1, misses = 0;
 *   4. a track that was not found: its pose is kept, misses + 1, and it is deleted once misses > max_misses;
 *   5. the search, when scene != NULL and either no track lives or frame % detect_every == 0 (frame counts the steps of
 *      this tracker from 0): oslam_db_detect on the scene and view (params.detect), then oslam_tracker_update.
 *   Every live track's age goes up by 1 per step after its birth.  Output: the live tracks ordered by id (tracks born in
 *   this step included, with age 0 and the detection's pose); when more than cap live, OSLAM_E_LIMIT with *n_out = their
 *   number.  *searched (may be NULL) says whether this frame voted.
 * oslam_tracker_update associates and gives birth, on the host alone: a detection belongs to a live track of the same
 *   model when the two are the same instance by the test of oslam_select_instances (the transformed centroids within
 *   assoc_min_separation * extent and, unless assoc_max_angle == (float)pi, the rotation test); the nearest such track
 *   (smallest d2 of the centroids, in float) wins, ties to the lower id.  A matched detection changes nothing: the
 *   tracked pose is the fresher one.  An unmatched detection starts a track with the next id (hits 1, misses 0, found 1);
 *   ids are never reused.  Detections are handled in list order, so a second detection can match a track the first one
 *   started.
 * A tracker borrows its database.  oslam_tracker_create_shapes makes one from the models' shapes alone (centroid [n][3]
 *   and extent [n] of the instance rule) for hosts without a device: oslam_tracker_update and oslam_tracker_tracks work,
 *   oslam_tracker_step is OSLAM_E_INVALID. */
typedef struct oslam_tracker oslam_tracker;
typedef struct oslam_tracker_params {
    oslam_track_params track;
    oslam_detect_params detect;
    oslam_arbitrate_params arbitrate;   /* over the tracked poses (step 2) */
    unsigned max_misses;       /* default 2 */
    unsigned detect_every;     /* frames between two searches, >= 1, default 10 */
    float assoc_min_separation;   /* as oslam_instance_params.min_separation, default 0.5 */
    float assoc_max_angle;     /* as oslam_instance_params.max_angle, default pi (translation only) */
    int reserved[4];
} oslam_tracker_params;

typedef struct oslam_track_state {
    uint32_t id, model;        /* model: database member */
    float T[16];
    uint32_t age, hits, misses;
    int32_t found;             /* in the last step (a birth counts as found) */
    oslam_track_result track;  /* of the last step; zeros for a track born in it */
} oslam_track_state;

int oslam_tracker_params_default(oslam_tracker_params *p);
/* p may be NULL (defaults) */
int oslam_tracker_create(oslam_db *db, const oslam_tracker_params *p, oslam_tracker **out);
int oslam_tracker_create_shapes(const float *centroid /* [n][3] */, const float *extent /* [n] */, size_t n,
                                const oslam_tracker_params *p, oslam_tracker **out);
void oslam_tracker_destroy(oslam_tracker *t);
/* host only: fold a detection list into the tracks (association + birth); used by _step, exported for tests */
int oslam_tracker_update(oslam_tracker *t, const oslam_detection *det, size_t n);
/* the live tracks ordered by id; OSLAM_E_LIMIT with *n_out = their number when cap is too small */
int oslam_tracker_tracks(const oslam_tracker *t, oslam_track_state *out, size_t cap, size_t *n_out);
/* one frame: scene may be NULL (no search this frame) */
int oslam_tracker_step(oslam_tracker *t, oslam_scene *scene, const oslam_view *v, oslam_track_state *out, size_t cap,
                       size_t *n_out, int *searched);

/* ---- camera motion between two depth views: dense projective ICP of one whole image against another (KinFu's camera
 * tracking, frame to frame).  It gives the camera's motion once per frame, independent of the database; the stages
 * above assume a camera that stands still.
 *
 * T_out is the float32 row-major rigid transform that takes a point in the source camera's coordinates to the
 * destination camera's.  With src = the previous frame and dst = the current one a static world point keeps its
 * identity, and a static object's pose in the new frame is T_out * T_old.
 * Levels.  Up to OSLAM_EGOMOTION_MAX_LEVELS levels {stride, max_iterations}, run in order (a level with max_iterations
 *   0 is passed over); the default is KinFu's coarse-to-fine schedule, strides 4, 2, 1 with 4, 5 and 10 iterations.  A
 *   level selects the source pixels with u % stride == 0 && v % stride == 0, numbered row-major over that lattice:
 *   index i is the pixel (u, v) = ((i % lw) * stride, (i / lw) * stride) with lw = ceil(width / stride) and
 *   n = lw * ceil(height / stride) indices.  Levels subsample the source only; the destination is always the
 *   full-resolution map.  A coarse level buys time, not a wider convergence basin: every level looks at the one pixel a
 *   source point projects to, and the gates are the same at every level.  Image pyramids are oslam_pyramid_egomotion's
 *   (below): there a level halves both images.
 * Correspondence of a selected source pixel.  Its record in the source's map (the maps of oslam_track, built on first
 *   use) is (p, n); it takes part only when it has a normal.  p' and n' under the float32 pose T exactly as
 *   oslam_refine, oslam_verify and oslam_track compute them: p'x = ((T0*px + T1*py) + T2*pz) + T3 and so on, n' without
 *   the translation.  p'z must lie within [z_min, z_max] of dst; the pixel in dst is oslam_verify's (fu, fv) with the
 *   destination's intrinsics, fu = floorf(((p'x * fx) / p'z + cx) + 0.5f), range-checked in float.  q, nq are that
 *   pixel's record in the destination's map.  The correspondence exists when the pixel has a normal,
 *   (dx*dx + dy*dy) + dz*dz <= r*r with d = q - p' and r = max_corr_dist in metres (a view has no d_dist; r*r rounded
 *   to float), and (n'x*nqx + n'y*nqy) + n'z*nqz >= min_normal_dot.  One candidate pixel, no search and no BACK test.
 * Step.  oslam_refine's Gauss-Newton step with these correspondences and the model centroid cm = (0, 0, 0), so that
 *   the pivot is the source camera's centre in the destination frame: the residual nq . (p' - q), the same 29 sums, the
 *   same damped Cholesky in double, Rodrigues step and Gram-Schmidt.  The sums: float over each block of 256
 *   consecutive lattice indices through the fixed tree (per 64 indices v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1,
 *   an index without a correspondence adds 0; then the four 64s as ((s0 + s1) + s2) + s3), then double.  The grouping of
 *   the double additions depends on the level and the image size only, never on which workgroup finished first: with
 *   nb = ceil(n / 256) blocks, chunk = ceil(nb / 256) and G = ceil(nb / chunk) slots, slot g is the sum of its blocks
 *   g * chunk .. min((g + 1) * chunk, nb) - 1 added in ascending order to 0.0; strand j (0..7) is the sum of the slots
 *   j, j + 8, j + 16, ... added in ascending order to 0.0; the sum is ((((((s0 + s1) + s2) + s3) + s4) + s5) + s6) + s7.
 *   The convergence test, |omega| < stop_rot (radians) and |v| < stop_trans (metres), ends a level, not the call: the
 *   next level starts from the float32 pose it left (inside a level the pose is carried in double), so a call with the
 *   levels A then B equals a call with A followed by a call with B from its T_out, bit for bit.  Fewer than 6 correspondences or a failed factorisation end the call with
 *   the pose as it then stands.
 * Result: iterations per level (steps taken); correspondences and rmse = sqrtf((float)(S[28] / S[27])) of the last step
 *   of the call (0 without a correspondence); overlap = (float)c / (float)s of the last step of the level with the
 *   smallest stride that evaluated a step (the later of equal strides), c = its correspondences and s = its selected
 *   source pixels that have a normal (0 when s is 0); converged = the last level that ran ended by its convergence
 *   test; ok = overlap >= min_overlap; launches, ms_total.
 * src == dst (the same handle) returns the identity at once: no device call, iterations 0, converged 1, overlap 1,
 *   ok = 1 >= min_overlap, whatever T_init is.
 * Arguments are checked before any handle is read or any device call is made: NULL src, dst or T_out, parameters that
 *   are not finite, n_levels outside 1..3, a stride outside 1..16, an iteration count above 1000, max_corr_dist <= 0, a
 *   negative stop criterion, min_overlap outside [0, 1] and a T_init that is not rigid (the test of oslam_refine) are
 *   OSLAM_E_INVALID; so are two views on different devices.
 * Cost: one kernel launch per scheduled iteration (k_ego_step, at most 256 workgroups of 256 threads; the last
 *   workgroup to arrive adds the partial sums in the order above, solves and leaves the pose for the next launch; no
 *   workgroup waits for another, no float atomics), all enqueued back to back, a launch whose level is over or whose
 *   call is done returning at once; one memset, one host wait and one copy of the result record into pinned memory.
 *   res->launches == the scheduled iterations (19 by default), plus 1 for each view whose maps did not exist yet.  Two
 *   calls give the same bits.  Egomotion calls of one process take turns, on every device: they share one pinned
 *   state, and its lock is held from the upload to the end of the host wait.  The lock of the views' maps (the tracking
 *   stage's) is taken inside it, never the other way round.
 * Defaults (calibration table: tests/test_camera_host.py, a camera that turns 3 degrees and moves 3 cm per frame
 *   before a room 5.4 m away, three seeds).  min_normal_dot is KinFu's cos(20 degrees).  max_corr_dist is 0.30 m and
 *   NOT KinFu's 0.10 m: at that motion a point moves 0.28 m between frames, 0.10 m shuts out the surfaces that tell a
 *   turn from a step sideways and the result slides by 0.22 .. 0.29 m; 0.20, 0.30 and 0.50 m all follow the camera to
 *   0.012 degrees and 0.8 mm per frame.  On one image pair the gate has to admit the motion itself (the pyramid's calibration: DESIGN.md 7j).  stop_rot
 *   1e-5, stop_trans 1e-5 m.  min_overlap 0.75: consecutive frames reach an overlap of 0.832 .. 0.935, a jump of 7 .. 9
 *   frames (21 .. 27 degrees) 0.000 .. 0.672.  The overlap measures shared surface, not identity: frames of a similar
 *   room (the same floor, a wall 0.4 m further) reach 0.274 .. 0.875 and are not told apart. */
#define OSLAM_EGOMOTION_MAX_LEVELS 3
typedef struct oslam_egomotion_level {
    unsigned stride;           /* 1..16 */
    unsigned max_iterations;   /* 0..1000 */
} oslam_egomotion_level;

typedef struct oslam_egomotion_params {
    unsigned n_levels;         /* 1..3, default 3 */
    oslam_egomotion_level level[OSLAM_EGOMOTION_MAX_LEVELS];   /* default {4, 4}, {2, 5}, {1, 10} */
    float max_corr_dist;       /* metres, default 0.30 */
    float min_normal_dot;      /* default 0.93969262 (cos 20 degrees) */
    float stop_rot;            /* radians, default 1e-5 */
    float stop_trans;          /* metres, default 1e-5 */
    float min_overlap;         /* [0, 1], default 0.75 */
    int reserved[4];
} oslam_egomotion_params;

typedef struct oslam_egomotion_result {
    uint32_t iterations[OSLAM_EGOMOTION_MAX_LEVELS];
    uint32_t correspondences;  /* of the last step */
    float rmse;                /* of the last step, metres */
    float overlap;
    int32_t converged, ok;
    uint32_t launches;         /* kernels this call enqueued */
    float ms_total;            /* whole call, host clock */
} oslam_egomotion_result;

int oslam_egomotion_params_default(oslam_egomotion_params *p);
/* T_init may be NULL (identity), ep may be NULL (defaults), res may be NULL */
int oslam_view_egomotion(oslam_view *src, oslam_view *dst, const float T_init[16], const oslam_egomotion_params *ep,
                         float T_out[16], oslam_egomotion_result *res);
/* test tap: pixel_out[w*h of src] = v*width+u in dst of each source pixel's correspondence under T at stride 1, -1 = none */
int oslam_view_egomotion_correspondences(oslam_view *src, oslam_view *dst, const float T[16],
                                         const oslam_egomotion_params *ep, int32_t *pixel_out);

/* ---- the tracker under a moving camera.  oslam_tracker_step_cam is oslam_tracker_step with a step 0 before the
 * tracking call: when T_cam != NULL (the camera's motion from the previous frame to this one, source camera to
 * destination camera: oslam_view_egomotion(previous view, this view)) every live track's pose T becomes
 * float32(double(T_cam) * double(T)), each element as ((a0*b0 + a1*b1) + a2*b2) (+ a3 for the translation) in double; an
 * element whose value does not change keeps its bits, so T_cam = identity gives oslam_tracker_step bit for bit, as
 * T_cam == NULL does.  The tracker also accumulates the camera's pose in the frame of its first step's camera (the
 * world): T_world_cam <- T_world_cam * T_cam^-1 in double, the inverse as [R^T | -(R^T t)]; a track's world pose is
 * T_world_cam * T.  oslam_tracker_camera returns its float32 rounding.  The tracker does not own views: the caller
 * computes T_cam and passes NULL when the result's ok is 0 (the prediction is then "where it was").  NULL t, v or n_out
 * and a T_cam that is not rigid (the test of oslam_refine) are OSLAM_E_INVALID before anything changes.
 * oslam_tracker_predict is step 0 alone, on the host (exported for tests; it also works on a tracker made from
 * shapes). */
int oslam_tracker_step_cam(oslam_tracker *t, oslam_scene *scene, const oslam_view *v, const float T_cam[16],
                           oslam_track_state *out, size_t cap, size_t *n_out, int *searched);
int oslam_tracker_predict(oslam_tracker *t, const float T_cam[16]);
int oslam_tracker_camera(const oslam_tracker *t, float T_world_cam[16]);

/* ---- fusion: depth views into a TSDF volume, and the volume ray-cast back into a view (KinFu's map).  A ray-cast view
 * is a genuine oslam_view: oslam_view_egomotion, oslam_track, oslam_verify and oslam_arbitrate take it as they take a
 * depth view, which gives frame-to-model camera tracking (oslam_volume_track) and clouds of the fused surface as one
 * pose sees it (oslam_view_to_cloud); oslam_volume_surface below gives the whole of it.  The restatement in numpy is tests/volume_ref.py; device and restatement agree bit for bit.
 *
 * T_vol_cam is everywhere the camera's pose in the volume frame: float32 row-major, camera coordinates -> volume
 * coordinates, rigid by the test of oslam_refine.  Its inverse T is formed on the host in double as [R^T | -(R^T t)],
 * -(R^T t)_a = -((R0a*t0 + R1a*t1) + R2a*t2), and rounded to float.
 * Storage.  One 32-bit word per voxel, int16 q | uint16 w << 16, x fastest, then y, then z; F = (float)q / 32767.0f; a
 *   new value is stored as q = (int)rintf(F * 32767.0f) (round to nearest even).  A fresh or reset volume is all zero:
 *   w = 0 reads as "never seen".
 * Integration of view V at T_vol_cam, for voxel (i, j, k): the centre g_x = origin_x + ((float)i + 0.5f) * voxel (y, z
 *   alike); p' = T g as oslam_refine computes it, p'x = ((T0*gx + T1*gy) + T2*gz) + T3; skipped unless p'z > 0 (a NaN
 *   fails); the pixel is oslam_verify's, fu = floorf(((p'x * fx) / p'z + cx) + 0.5f) with V's intrinsics, range-checked
 *   in float; z_o = V's z there, skipped unless z_o > 0; sdf = z_o - p'z; skipped unless sdf >= -mu;
 *   f = fminf(1.0f, sdf / mu); F' = ((F * (float)w) + f) / (float)(w + 1); w' = min(w + 1, max_weight).  sdf is the
 *   projective distance along the optical axis, the residual oslam_verify uses, NOT KinFu's distance along the ray: the
 *   zero crossing is the same, the band is thinner by the cosine towards the image's corners.  A skipped voxel is
 *   neither read nor written; a voxel belongs to one thread; no float atomics; two calls give the same bits.
 * Ray cast at T_vol_cam = M (rows M0..M11) with camera cam and size width x height, for pixel (u, v):
 *   d = (((float)u - cx) / fx, ((float)v - cy) / fy, 1), not normalised: the ray parameter t is the camera-frame z and a
 *   vertex is (dx * t, dy * t, t).  In the volume frame o = (M3, M7, M11) and Dx = (M0*dx + M1*dy) + M2 (y, z alike); the
 *   point at t is Px = ox + Dx * t.  Interval: [tn, tf] starts as [z_min, z_max]; per axis a with lo = origin_a + voxel
 *   and hi = origin_a + (float)(n_a - 1) * voxel (the box shrunk by one voxel): D_a == 0 misses unless lo <= o_a <= hi,
 *   otherwise ta = (lo - o_a) / D_a, tb = (hi - o_a) / D_a, tn = fmaxf(tn, fminf(ta, tb)), tf = fminf(tf, fmaxf(ta, tb));
 *   no hit unless tn <= tf.  Samples t_k = tn + (float)k * step, k = 0, 1, ... while t_k <= tf, step = 0.5f * mu in t (t
 *   is z and the truncation is along z, so no 1 / |d|).  A sample is the word of the voxel floorf((P_a - origin_a) *
 *   inv_voxel) per axis, inv_voxel = 1.0f / voxel; a coordinate outside the volume reads as w = 0.  A sample with w = 0
 *   forgets the previous sample; (F_prev > 0, F < 0) is a front-face crossing between t_prev and t_k;
 *   (F_prev < 0, F > 0) ends the ray without a hit.
 *   Trilinear F at a volume-frame point: c_a = (P_a - origin_a) * inv_voxel - 0.5f, b_a = floorf(c_a), f_a = c_a - b_a;
 *   all of 0 <= b_a <= n_a - 2 and all 8 corners with w > 0, or there is no value; lerp(p, q, f) = p * (1.0f - f) + q * f
 *   along x, then y, then z.  At a crossing Ft, Ftdt = the trilinear F at t_prev and t_k (no value: no hit);
 *   t* = t_prev - (step * Ft) / (Ftdt - Ft); no hit unless Ftdt - Ft < 0, t_prev <= t* <= t_k and z_min <= t* <= z_max.
 *   The pixel's z is t*.  Normal: g_a = F(P* + voxel e_a) - F(P* - voxel e_a) with P* the point at t*, six trilinear
 *   reads that all need a value; len = sqrtf((gx*gx + gy*gy) + gz*gz) must satisfy 0 < len <= 3.0e38f (the test of
 *   oslam_depth_to_cloud); n = g / len; into the camera frame by R^T, n'x = (M0*nx + M4*ny) + M8*nz; the pixel has a
 *   normal only when (n'x * vx + n'y * vy) + n'z * t* < 0: the gradient of a front crossing faces the camera, one that
 *   does not is a defect of the data and is not flipped.
 *   The result is an oslam_view the caller owns (oslam_view_destroy): its z image holds t* (0 without a hit), its maps
 *   exist from the start (x y z 1 | nx ny nz 0 where the pixel has a normal, zeros elsewhere), max_jump is cam's,
 *   depth_scale is ignored.
 * oslam_volume_track is host glue: ray-cast at T_vol_cam_prev with the frame's own camera and size,
 *   oslam_view_egomotion(src = the frame, dst = the ray-cast view, identity, ep), T_vol_cam_out =
 *   float32(double(T_vol_cam_prev) * double(T)) with the element order of oslam_tracker_step_cam; the egomotion result
 *   comes back as it is (launches + 1 for the ray cast).  It does not integrate: the caller does when ok is 1.
 * oslam_view_to_cloud compacts the pixels of a view that have a normal, in row-major order, through the flag, scan and
 *   compact path of oslam_depth_to_cloud: for a depth view it returns what oslam_depth_to_cloud returns for the same
 *   image and camera bit for bit, for a ray-cast view the fused surface seen from that pose.  OSLAM_E_LIMIT with
 *   *n_out = the number of points when cap is too small.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers, parameters that are not
 *   finite or lie outside the ranges below, a T_vol_cam that is not rigid, a camera oslam_view_create would refuse and a
 *   size outside 1..16384 are OSLAM_E_INVALID; so are a volume and a view on different devices.  The allocation is
 *   computed in size_t (512^3 voxels are 512 MiB).
 * Cost: integrate = one memset of the counter, k_tsdf_integrate, one copy back, one host wait; raycast = the same with
 *   k_tsdf_raycast.  Calls on volumes take turns (one lock, held to the end of the host wait).
 * The volume frame is fixed, the window of voxels the volume holds is not: oslam_volume_shift below moves it by whole
 *   voxels, and every call above reads the origin that goes with the window.
 * Out of scope: the along-ray distance, masking tracked objects out of the integration, several GPUs;
 *   oslam_tracker keeps taking T_cam from the caller. */
typedef struct oslam_volume oslam_volume;
typedef struct oslam_volume_params {
    unsigned nx, ny, nz;      /* voxels per side, each 16..512 and a multiple of 8; default 256^3 */
    float voxel;              /* metres, > 0; default 0.02 */
    float origin[3];          /* volume-frame position of the corner of voxel (0,0,0); default the volume centred before
                                 the camera: (-nx/2, -ny/2, 0) voxels */
    float mu;                 /* truncation distance in metres, >= 2 voxels; default 4 voxels (KinFu's order).  Across
                                 surfaces seen at a grazing angle the projective band is thinner than mu, and a trilinear
                                 read needs all 8 corners seen: in the calibration room 4 voxels leave the
                                 frame-to-model overlap at 0.65, below oslam_view_egomotion's min_overlap of 0.75; 8
                                 voxels track there.  Choose mu for the scene */
    unsigned max_weight;      /* 1..65535, default 128 (KinFu's) */
    int reserved[4];
} oslam_volume_params;

typedef struct oslam_integrate_result {
    uint32_t updated;          /* voxels the call updated */
    uint32_t launches;
    float ms_total;            /* whole call, host clock */
} oslam_integrate_result;

typedef struct oslam_raycast_result {
    uint32_t hits;             /* pixels with a hit */
    uint32_t normals;          /* pixels with a normal */
    uint32_t launches;
    float ms_total;
} oslam_raycast_result;

int oslam_volume_params_default(oslam_volume_params *p);
int oslam_volume_create(const oslam_volume_params *p, int dev, oslam_volume **out);
int oslam_volume_destroy(oslam_volume *vol);
int oslam_volume_reset(oslam_volume *vol);
/* res may be NULL */
int oslam_volume_integrate(oslam_volume *vol, const oslam_view *v, const float T_vol_cam[16], oslam_integrate_result *res);
int oslam_volume_raycast(oslam_volume *vol, const float T_vol_cam[16], const oslam_camera *cam, int width, int height,
                         oslam_view **view_out, oslam_raycast_result *res);
/* ep may be NULL (defaults), ego_res may be NULL */
int oslam_volume_track(oslam_volume *vol, oslam_view *v, const float T_vol_cam_prev[16], const oslam_egomotion_params *ep,
                       float T_vol_cam_out[16], oslam_egomotion_result *ego_res);
int oslam_view_to_cloud(oslam_view *v, float *xyz_out, float *nrm_out, size_t cap, size_t *n_out);
/* test taps: the whole volume, tsdf_q_out and weight_out [nz][ny][nx]; the view's maps [h][w][8] and z [h][w] (z_out may
 * be NULL) */
int oslam_volume_voxels(oslam_volume *vol, int16_t *tsdf_q_out, uint16_t *weight_out);
int oslam_view_maps(oslam_view *v, float *maps_out, float *z_out);

/* ---- depth image pyramids and coarse-to-fine camera tracking over them (KinFu's pyrDown and its three-level ICP).  A
 * pyramid is up to three views of one image: level 0 is the caller's view, level k + 1 is level k at half the
 * resolution.  A coarser level is a genuine oslam_view: oslam_verify, oslam_track, oslam_arbitrate, oslam_view_egomotion
 * and oslam_volume_integrate take it unchanged.  At half resolution the same motion is half as many pixels and the one
 * pixel a source point projects to stands for four, which is what widens the convergence basin of the projective
 * correspondence.  The restatement in numpy is tests/pyramid_ref.py; device and restatement agree bit for bit.
 *
 * Size and camera.  Level k is w x h with camera (fx, fy, cx, cy, z_min, z_max, max_jump).  Level k + 1 is
 *   w' = (w + 1) / 2 by h' = (h + 1) / 2; its pixel (u, v) is centred on pixel (2u, 2v) of level k, which always exists.
 *   Its camera is fx * 0.5f, fy * 0.5f, cx * 0.5f, cy * 0.5f (all exact in float), z_min and z_max unchanged, and
 *   max_jump * 2.0f: the pixel spacing doubles, so the same slope gives twice the depth step between neighbours.
 * Depth (KinFu's pyrDown).  c = z[2v][2u]; c == 0 (invalid) gives 0.  Otherwise the 5 x 5 window dy = -2..2 (outer),
 *   dx = -2..2 (inner), clipped to the image, is walked from sum = 0.0f, cnt = 0: a pixel takes part iff z > 0 and
 *   fabsf(z - c) <= depth_band, and then does sum += z in float, in that row-major order, and cnt++ (the centre always
 *   takes part).  The output is fminf(fmaxf(sum / (float)cnt, z_min), z_max).  No fused multiply-add anywhere; the
 *   division is the correctly rounded one.  depth_band is in metres; the default 0.09 is KinFu's 3 x 30 mm.
 * Maps.  A coarser level starts without maps; it gets its vertex and normal map on first use as every depth view does,
 *   from its own z image, its camera and its max_jump.  That holds for the pyramid of a ray-cast view too: level 0
 *   keeps the normals of the TSDF gradient, the coarser levels take theirs from z differences of the down-sampled t*.
 * oslam_pyramid_create borrows base as level 0 (the caller keeps it alive and destroys it after the pyramid) and owns
 *   the rest: n_levels - 1 launches of k_pyr_down back to back, one host wait.  oslam_pyramid_level returns a borrowed
 *   view, level 0 is base itself.  oslam_pyramid_destroy does not destroy base.
 * oslam_pyramid_egomotion is oslam_view_egomotion with a pair of views per schedule level.  ep->level[i].stride must be
 *   1, 2 or 4 and names pyramid level log2(stride) of both pyramids (a level either lacks is OSLAM_E_INVALID); that level
 *   of the schedule runs oslam_view_egomotion's step with the level-k views as source and destination over the stride-1
 *   lattice of the level-k source, so the default schedule {4, 4}, {2, 5}, {1, 10} is KinFu's: levels 2, 1, 0.
 *   Everything else is oslam_view_egomotion's, under the same lock: the gates in metres (the same at every level), the
 *   sums, the solve, the convergence test that ends a level, the float32 hand-over of the pose between levels, the
 *   result fields (overlap from the level with the smallest stride that evaluated a step), one memset, one host wait,
 *   one pinned copy; launches == the scheduled iterations plus 1 for every level view whose maps did not exist yet (a
 *   level with max_iterations 0 builds none).  src == dst returns the identity at once.  The call equals the chain of
 *   oslam_view_egomotion(level k of src, level k of dst, T, {n_levels 1, {1, its iterations}}) calls in schedule order,
 *   each from the previous T_out, bit for bit in T_out and iterations; correspondences, rmse and overlap are those of
 *   the chain's last call that evaluated a step.
 * oslam_volume_track_pyramid is host glue as oslam_volume_track is: ray-cast at T_vol_cam_prev with the camera and size
 *   of the frame's level 0, a pyramid of the ray-cast view with pp (NULL: the defaults),
 *   oslam_pyramid_egomotion(src = frame, dst = that pyramid, identity, ep), the pose product of oslam_volume_track; the
 *   ray-cast view and its pyramid are freed.  launches counts the ray cast and the down-sampling launches too.  It does
 *   not integrate.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers, n_levels outside 1..3, a
 *   depth_band that is not finite or <= 0, a k beyond the pyramid, the parameter checks of oslam_view_egomotion, a stride
 *   other than 1, 2, 4 and a T that is not rigid are OSLAM_E_INVALID; so are pyramids (or a volume and a pyramid) on
 *   different devices.
 * Out of scope: resizing the ray cast's TSDF normals instead of recomputing them
 *   from z, per-level gates, feeding oslam_tracker or a volume's own stepping from the pyramid (callers opt in through
 *   these calls), several GPUs. */
typedef struct oslam_pyramid oslam_pyramid;
typedef struct oslam_pyramid_params {
    unsigned n_levels;         /* 1..3 including the base, default 3 */
    float depth_band;          /* metres, > 0, default 0.09 */
    int reserved[4];
} oslam_pyramid_params;

int oslam_pyramid_params_default(oslam_pyramid_params *p);
/* pp may be NULL (defaults) */
int oslam_pyramid_create(oslam_view *base, const oslam_pyramid_params *pp, oslam_pyramid **out);
int oslam_pyramid_destroy(oslam_pyramid *pyr);
int oslam_pyramid_level(oslam_pyramid *pyr, unsigned k, oslam_view **view_out);
/* T_init may be NULL (identity), ep may be NULL (defaults), res may be NULL */
int oslam_pyramid_egomotion(oslam_pyramid *src, oslam_pyramid *dst, const float T_init[16],
                            const oslam_egomotion_params *ep, float T_out[16], oslam_egomotion_result *res);
/* pp and ep may be NULL (defaults), ego_res may be NULL */
int oslam_volume_track_pyramid(oslam_volume *vol, oslam_pyramid *frame, const float T_vol_cam_prev[16],
                               const oslam_pyramid_params *pp, const oslam_egomotion_params *ep,
                               float T_vol_cam_out[16], oslam_egomotion_result *ego_res);

/* ---- a bilateral filter of a view's depth image (KinFu's first step on every frame).  Every stage that looks at a
 * depth image takes its vertices and normals from raw z differences of the four axis neighbours, so depth noise of a
 * few millimetres turns the normals by tens of degrees and the camera tracker loses its correspondences.
 * The filter smooths z within a surface and leaves depth steps alone.  Its result is a genuine oslam_view: oslam_verify,
 * oslam_track, oslam_view_egomotion, oslam_pyramid_create and oslam_volume_integrate take it unchanged.  The restatement
 * in numpy is tests/bilateral_ref.py; device and restatement agree bit for bit in the z image and both counters.
 *
 * All arithmetic is float32 without fused multiply-add, grouped as written.
 * Constants, computed once on the host: inv_s = (float)(1.0 / ((double)sigma_space * (double)sigma_space)) and
 *   inv_r = (float)(1.0 / ((double)sigma_depth * (double)sigma_depth)).  R = radius.
 * Depth.  c = z[v][u]; c == 0 (invalid) gives 0.  Otherwise the (2R + 1)^2 window dy = -R..R (outer), dx = -R..R
 *   (inner), clipped to the image, is walked from sd = 0.0f, sw = 0.0f, taps = 0.  For the pixel z = z[v + dy][u + dx]:
 *   it takes part only if z > 0; then d = z - c and t = (float)(dx * dx + dy * dy) * inv_s + (d * d) * inv_r, and it takes
 *   part only if t < 9.0f; then w = G[(int)(t * 32.0f)], sd += w * d, sw += w, taps++, in that row-major order.  The centre
 *   always takes part with d = 0 and t = 0, so sw > 0.  The sum runs over the differences d, not over the depths: at
 *   6 m a float32 depth has 0.5 um of resolution left, a difference of a few centimetres has all of its bits.
 *   The output is fminf(fmaxf(c + sd / sw, z_min), z_max) with the correctly rounded division.  The valid pixels of the
 *   output are exactly those of the input.
 * Table.  G[i] = (float)exp(-0.5 * (i + 0.5) / 32) for i = 0..287 (csrc/oslam_gauss_table.h, written by
 *   tools/gen_gauss_table.py as bit patterns): one fixed Gaussian sampled at the midpoints of bins of 1/32, independent of
 *   both sigmas because t is already in units of sigma squared.  t < 9 is the 3-sigma cut; t * 32 is exact in float and
 *   below 288, so the index never leaves the table.  The table, not expf, is what lets device and numpy agree bit for bit.
 *   oslam_gauss_table is a host-only tap on the compiled-in table for the tests.
 * Output view.  It has v's size, camera and max_jump and is owned by the caller (oslam_view_destroy).  It starts without
 *   maps and gets its vertex and normal map on first use from its own z image, as a masked view or a pyramid level does.
 *   That holds for a ray-cast input too: its filtered copy takes its normals from z differences, not the TSDF gradient.
 * Result.  valid counts the output pixels with z > 0; taps is the integer sum of taps over all pixels (at 640 x 480 and
 *   R = 8 at most 88 780 800 < 2^27), the order-free check of the gate; launches == 1.
 * Cost: one memset of the counters, k_bilateral, one small copy back, one host wait.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers (bp and res may be NULL), a
 *   radius outside 1..OSLAM_BILATERAL_MAX_RADIUS and a sigma that is not finite or <= 0 (or so small that 1 / sigma^2
 *   is not a finite float) are OSLAM_E_INVALID.  *out is NULL on every failure.
 * Out of scope: a noise model that grows with z^2, filtering inside oslam_scene_from_depth, feeding oslam_tracker or a
 *   pyramid from the filter automatically (callers pass a filtered view), any default of another params struct, several
 *   GPUs. */
#define OSLAM_BILATERAL_MAX_RADIUS 8
typedef struct oslam_bilateral_params {
    unsigned radius;           /* half-width of the window in pixels, 1..OSLAM_BILATERAL_MAX_RADIUS, default 6 */
    float sigma_space;         /* pixels, > 0, default 4.5 */
    float sigma_depth;         /* metres, > 0, default 0.03; at least twice the depth noise (calibration: DESIGN.md 7s) */
    int reserved[4];
} oslam_bilateral_params;
typedef struct oslam_bilateral_result {
    uint32_t valid;            /* output pixels with z > 0 */
    uint32_t taps;             /* window pixels that took part, summed over the image */
    uint32_t launches;
    float ms_total;
} oslam_bilateral_result;

int oslam_bilateral_params_default(oslam_bilateral_params *p);
/* bp may be NULL (defaults), res may be NULL */
int oslam_view_bilateral(const oslam_view *v, const oslam_bilateral_params *bp, oslam_view **out,
                         oslam_bilateral_result *res);
/* *w_out = G[i], i in 0..287 */
int oslam_gauss_table(unsigned i, float *w_out);

/* ---- hypotheses rendered into a labelled depth view, and views masked by it.  The image a set of hypotheses
 * (model, T) would produce in a given camera: a z image and, per pixel, the index of the hypothesis in front.  With it a
 * view can be split into the static background and the tracked objects before oslam_volume_integrate and
 * oslam_view_egomotion see it, which both treat every pixel as static world.  The models are clouds, so the render is a
 * point splat, not a mesh raster.  The restatement in numpy is tests/render_ref.py; device and restatement agree bit
 * for bit in both images, every counter and the masked view.
 *
 * Hypothesis h is (models[h], T + 16 h): T float32, row-major, model to camera; 1 <= H <= OSLAM_ARBITRATE_MAX_HYPOTHESES;
 *   an all-zero T is a skipped hypothesis (drawn 0, pixels 0; the labels keep the caller's indices).
 * Splat, for model point i of hypothesis h, in float32 without fused multiply-add:
 *   p' = (R p + t), n' = R n by oslam_verify's sequence (the one of refine, verify and track).
 *   Unless keep_back, the point is dropped when (n'x p'x + n'y p'y) + n'z p'z >= 0: oslam_verify's BACK.
 *   The point is dropped when p'z lies outside [z_min, z_max] or its centre pixel (fu, fv), oslam_verify's rounding
 *   floorf(((p'x fx) / p'z + cx) + 0.5f), lies outside the image: oslam_verify's OUT.  A point whose centre falls just
 *   outside the image draws nothing even where its splat would reach in; the mask's dilate covers that seam.
 *   Half-width: rho = (float)((double)footprint * d_dist) with the model's d_dist, kf = floorf((rho * fx) / p'z + 0.5f),
 *   k = kf < (float)max_splat ? (int)kf : max_splat.
 *   The point draws every pixel of [fu - k, fu + k] x [fv - k, fv + k], clipped to the image, at its own depth p'z: a
 *   splat is a fronto-parallel square, whatever the normal says.  drawn counts the points that got this far.
 *   A pixel keeps the smallest key (uint64)bits(p'z) << 32 | h of the points that drew it (p'z > 0: its bits order as the
 *   value does): the nearest point wins, at bit-equal z the lower hypothesis index.  The result does not depend on the
 *   order of points or hypotheses beyond that rule.
 * Resolve: a pixel nobody drew has z = 0 (invalid) and label -1; otherwise z is the float of the key's high word and the
 *   label its low word.  pixels[h] counts the pixels labelled h.  Every counter is an integer sum.
 * The z image lands in a genuine oslam_view with the caller's camera (depth_scale is not used; max_jump limits its normal
 *   map): every stage that takes a view takes the render.  oslam_render_view lends that view (borrowed, as
 *   oslam_pyramid_level's; oslam_render_destroy gives it back); its vertex and normal maps are built on first use.  The
 *   render also keeps tol[h] = (float)((double)depth_tol * d_dist), oslam_verify's tolerance, for the mask.
 * oslam_db_render is oslam_render_create with models[h] = the database's member[h].
 * Cost, the same for 1 hypothesis and for 1024: one upload, one memset, k_render_splat and k_render_resolve, one small
 *   copy back, one host wait; launches == 2, the kernels.  When every hypothesis is skipped the render is empty (z all
 *   0, labels all -1), k_render_splat is not launched and launches == 1.
 *
 * oslam_view_mask: pixel (u, v) of the observed view v with depth z_o is an object pixel iff z_o > 0 and some pixel
 *   (x, y) of the (2 dilate + 1)^2 window around it, clipped to the image, has a label l >= 0 (with only >= 0: l == only)
 *   and fabsf(z_o - z_r(x, y)) <= tol[l].  That mirrors oslam_verify's SUPPORTED: an occluder in front of the object
 *   stays background, and so does a surface seen through a wrong pose.  OSLAM_MASK_REMOVE writes object ? 0 : z_o,
 *   OSLAM_MASK_KEEP object ? z_o : 0, into a new view with v's camera and max_jump that the caller owns
 *   (oslam_view_destroy).  valid_in counts z_o > 0, object_pixels the object pixels, valid_out the valid pixels of the
 *   output: the two modes partition valid_in.  One memset, k_view_mask, one copy back, one host wait; launches == 1.
 * oslam_view_info returns the camera (depth_scale 1) and size of any view: the camera to render for it.
 * Arguments are checked before any handle is read or any device call is made: NULL pointers (rp, mp and res may be
 *   NULL), H outside 1..OSLAM_ARBITRATE_MAX_HYPOTHESES, parameters that are not finite, footprint <= 0, max_splat above
 *   OSLAM_RENDER_MAX_SPLAT, depth_tol <= 0, a camera or size oslam_view_create would refuse (or a max_jump it would), a T
 *   that is neither all zero nor rigid, a mode other than the two, dilate above 8 and only below -1 are OSLAM_E_INVALID.
 *   Then the handles: models on different devices, a member index outside the database, an only beyond the render's
 *   hypotheses, and a view and a render that differ in device, size, or bit for bit in fx, fy, cx, cy, z_min or z_max
 *   are OSLAM_E_INVALID too.
 * Out of scope: points whose centre is off-image, splats tilted by their normals, mesh rasterisation, colour, any change
 *   to oslam_verify, oslam_arbitrate, oslam_track or oslam_tracker (verification against the model's own z-buffer is
 *   what this makes possible), several GPUs. */
#define OSLAM_RENDER_MAX_SPLAT 8
typedef struct oslam_render_params {
    float footprint;           /* splat radius in units of the model's d_dist, > 0, default 0.75 (calibration: DESIGN.md 7p) */
    unsigned max_splat;        /* cap of the pixel half-width, 0..OSLAM_RENDER_MAX_SPLAT, default 8 */
    float depth_tol;           /* as oslam_verify_params: in units of d_dist, > 0, default 1.0; kept per hypothesis for the mask */
    int keep_back;             /* 0 (default): points that face away are not drawn */
    int reserved[4];
} oslam_render_params;
typedef struct oslam_render_result {   /* per hypothesis */
    uint32_t drawn;            /* model points that were splatted */
    uint32_t pixels;           /* pixels whose label is this hypothesis */
    uint32_t launches;         /* of the whole call */
    float ms_total;            /* of the whole call */
} oslam_render_result;
typedef struct oslam_render oslam_render;

int oslam_render_params_default(oslam_render_params *p);
/* rp may be NULL (defaults), res [H] may be NULL */
int oslam_render_create(oslam_model *const *models, const float *T, size_t H, const oslam_camera *cam, int width,
                        int height, const oslam_render_params *rp, oslam_render **out, oslam_render_result *res);
int oslam_db_render(oslam_db *db, const uint32_t *member, const float *T, size_t H, const oslam_camera *cam, int width,
                    int height, const oslam_render_params *rp, oslam_render **out, oslam_render_result *res);
int oslam_render_view(oslam_render *r, oslam_view **view_out);
/* labels_out [height * width], -1 = nothing drawn */
int oslam_render_labels(oslam_render *r, int32_t *labels_out);
int oslam_render_destroy(oslam_render *r);
int oslam_view_info(const oslam_view *v, oslam_camera *cam_out, int *width_out, int *height_out);

#define OSLAM_MASK_REMOVE 0    /* the static background: object pixels become invalid */
#define OSLAM_MASK_KEEP 1      /* the objects alone */
#define OSLAM_MASK_MAX_DILATE 8
typedef struct oslam_mask_params {
    int mode;                  /* OSLAM_MASK_REMOVE (default) or OSLAM_MASK_KEEP */
    unsigned dilate;           /* half-width of the window in pixels, 0..OSLAM_MASK_MAX_DILATE, default 2 */
    int32_t only;              /* -1 (default): every label; otherwise that hypothesis alone */
    int reserved[4];
} oslam_mask_params;
typedef struct oslam_mask_result {
    uint32_t valid_in, object_pixels, valid_out, launches;
    float ms_total;
} oslam_mask_result;

int oslam_mask_params_default(oslam_mask_params *p);
/* mp may be NULL (defaults), res may be NULL */
int oslam_view_mask(const oslam_view *v, const oslam_render *r, const oslam_mask_params *mp, oslam_view **out,
                    oslam_mask_result *res);

/* ---- hypotheses judged against their own z-buffers and arbitrated by their conflict rates.  oslam_verify asks whether
 * a model's points find support in the image, oslam_arbitrate compares depth residuals tile by tile and so follows the
 * poses.  This stage turns the question around: does the image show what the hypothesis says the camera must see, pixel
 * by pixel over its whole silhouette?  A hypothesis that predicts surface where the camera saw through to the wall pays
 * for every such pixel.  It complements oslam_verify (a hypothesis hidden behind an occluder scores well here and is
 * rejected by verify's coverage) and uses oslam_arbitrate's elimination.  The restatement in numpy is
 * tests/explain_ref.py; device and restatement agree bit for bit in every integer and every float field.
 *
 * All arithmetic is float32 without fused multiply-add, grouped as written, unless stated.
 * Input: a view v and H hypotheses (models[h], T + 16 h), 1 <= H <= OSLAM_ARBITRATE_MAX_HYPOTHESES.  An all-zero T is a
 *   skipped hypothesis: every counter of it is 0 and it is never live.
 * Solo z image.  Z_h is exactly the z image oslam_render_create produces for the one-element list {(models[h], T_h)} in
 *   v's camera and size with the call's footprint, max_splat and keep_back: the same transform, BACK and OUT tests,
 *   centre pixel and half-width k, a fronto-parallel square at the point's depth, the nearest point wins.  Alone, the key
 *   needs no label: the unsigned minimum of bits(p'z), empty = all ones, resolved to 0.  drawn[h] is the render's count.
 *   tol_h = (float)((double)depth_tol * d_dist) of its model, as everywhere.
 * Class of pixel (x, y) with Z_h > 0 and z_o the view's z there, tested in this order: UNKNOWN if z_o == 0; AGREE if
 *   fabsf(z_o - Z_h) <= tol_h; OCCLUDED if z_o < Z_h; THROUGH otherwise.  An AGREE pixel has the residual
 *   x = fabsf(z_o - Z_h) * (65535.0f / tol_h), r = x < 65535.0f ? (uint32_t)x : 65535: oslam_arbitrate's quantisation.
 * Per hypothesis: pixels, agree, occluded, through, unknown (integers, pixels their sum); resid_sum (uint64, the sum of
 *   r); explained = (float)agree / (float)(agree + through), 0 when the denominator is 0; visible = (float)agree /
 *   (float)(agree + occluded + through), 0 likewise; mean_residual = (float)((((double)resid_sum / (double)agree) /
 *   65535.0) * (double)tol_h), 0 when agree is 0; conflict_q = (uint32_t)((65535 * (uint64_t)through) / (agree +
 *   through)), 0 when agree == 0: the conflict rate through / (agree + through) in 16 bits.
 * Claims.  An AGREE pixel claims tile t = (y / tile) * tiles_x + x / tile.  cnt[h][t] is the number of claiming pixels,
 *   sum[h][t] = cnt[h][t] * conflict_q[h].  tile in pixels is 4..128; 0 (the default) chooses oslam_arbitrate's automatic
 *   tile from tile_spacing, by the same function.  A tile holds at most 128^2 pixels, so cnt < 2^24 and sum < 2^40 as
 *   k_arbitrate's words require.
 * Elimination.  oslam_arbitrate's, unchanged, over this table.  Because sum / cnt is the hypothesis's one conflict rate in
 *   every tile, a tile belongs to the live claimant that explains its own silhouette best; ties go to the lower index,
 *   so a bit-identical duplicate of a hypothesis is suppressed by its first copy.  Liveness, min_tiles, the loser,
 *   suppressed_by, rounds, and share / owned at elimination are as documented for oslam_arbitrate.
 * Rectangle.  A hypothesis's z-buffer covers a rectangle of the image that contains everything it can draw, from its
 *   model's bounding sphere (centre: the model's double mean under T; radius: the largest distance of a model point
 *   from the mean): the four extreme combinations of x, y and z projected, padded by max_splat + 2 pixels and clipped to
 *   the image; the whole image when the sphere reaches z <= 0; empty when it lies outside [z_min, z_max].  It is a
 *   container, not part of the rule: no result depends on it.  Every write is checked against it; a point that would
 *   fall outside is not written, and the call fails with OSLAM_E_DEVICE.  oslam_explain_rect is that arithmetic alone,
 *   on the host, without a device: rect_out = x0, y0, width, height (a width of 0: empty).
 * Arguments are checked before any handle is read or any device call is made, as oslam_render_create and oslam_arbitrate
 *   check the fields they share: NULL pointers (ep may be NULL), H outside 1..OSLAM_ARBITRATE_MAX_HYPOTHESES, parameters
 *   that are not finite, footprint <= 0, max_splat above OSLAM_RENDER_MAX_SPLAT, depth_tol <= 0, tile not 0 and outside
 *   4..128, tile_spacing <= 0, min_owned_share outside [0, 1], a T that is neither all zero nor rigid are
 *   OSLAM_E_INVALID.  Then the handles: a model and the view on different devices.  A claims table above 256 MiB
 *   (H * tiles * 8 B), or z-buffers above 256 MiB in total, is OSLAM_E_LIMIT before anything is launched.
 * Cost, the same for 1 hypothesis and for 1024: one upload, two memsets, k_explain_splat, k_explain_score,
 *   k_explain_claims and k_arbitrate, one copy back of a 32-byte record per hypothesis and stage, one host wait;
 *   launches == 4.  When every hypothesis is skipped nothing is launched.  Integer sums and minima only: every result is
 *   the same on every run and for every order of the hypotheses' points.
 * Defaults: footprint, max_splat and keep_back are the render's, tile, tile_spacing and min_tiles the arbitration's,
 *   depth_tol 1.0.  min_owned_share is the arbitration's 0.52: it lies inside the gap the calibration table shows between
 *   the present model (first-round share 1.000) and its suppressed near twin (at most 0.116); the table is in
 *   tests/test_explain_host.py.  The thin margin of the rule is the gap of the conflict rates themselves, 0.031 to 0.064.
 * Out of scope: any change to oslam_db_detect or oslam_tracker (folding this stage into them is the follow-up), tilted
 *   splats, normals, colour, several GPUs. */
typedef struct oslam_explain_params {
    float footprint;           /* as oslam_render_params, default 0.75 */
    unsigned max_splat;        /* as oslam_render_params, default 8 */
    int keep_back;             /* as oslam_render_params, default 0 */
    float depth_tol;           /* in units of d_dist, > 0, default 1.0 */
    unsigned tile;             /* as oslam_arbitrate_params, default 0 (automatic) */
    float tile_spacing;        /* as oslam_arbitrate_params, default 2.0 */
    unsigned min_tiles;        /* as oslam_arbitrate_params, default 4 */
    float min_owned_share;     /* [0, 1]: the loser is suppressed below this share, default 0.52 */
    int reserved[4];
} oslam_explain_params;

typedef struct oslam_explain_result {  /* per hypothesis */
    uint32_t drawn;            /* model points that were splatted */
    uint32_t pixels;           /* pixels of its z image: agree + occluded + through + unknown */
    uint32_t agree, occluded, through, unknown;
    uint64_t resid_sum;        /* the sum of the AGREE pixels' quantised residuals */
    float explained, visible, mean_residual;
    uint32_t conflict_q;
    uint32_t claimed, owned;
    float share;
    int32_t kept, suppressed_by;
    uint32_t tile, rounds;     /* the whole call, shared by all hypotheses */
    uint32_t launches;         /* kernels this call enqueued */
    float ms_total;            /* whole call, host clock */
} oslam_explain_result;

int oslam_explain_params_default(oslam_explain_params *p);
/* models [H], T [H][16], res [H]; ep may be NULL (defaults) */
int oslam_explain(oslam_model *const *models, const float *T, size_t H, const oslam_view *v, const oslam_explain_params *ep,
                  oslam_explain_result *res);
/* hypothesis j = member j of the database with T[j] (zeros: skipped); equals oslam_explain on the same list */
int oslam_db_explain(oslam_db *db, const oslam_view *v, const float *T, const oslam_explain_params *ep,
                     oslam_explain_result *res);
/* the rectangle alone, no device: centre [3] and radius of the model's bounding sphere in the model frame */
int oslam_explain_rect(const double centre[3], double radius, const float T[16], const oslam_camera *cam, int width,
                       int height, unsigned max_splat, int rect_out[4]);
/* test tap: the solo z image of hypothesis h expanded to the full image, z_out [height * width] */
int oslam_explain_z(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                    const oslam_explain_params *ep, size_t h, float *z_out);
/* test tap: the table after k_explain_claims, as oslam_arbitrate_claims returns its own */
int oslam_explain_claims(oslam_model *const *models, const float *T, size_t H, const oslam_view *v,
                         const oslam_explain_params *ep, uint32_t *cnt_out, uint64_t *sum_out, size_t cap,
                         uint32_t *tile_out, size_t *n_tiles_out);

/* ---- the fused surface of a whole volume as a cloud and as a scene (KinFu's fetchCloud plus fetchNormals): every zero
 * crossing of the TSDF along a voxel edge becomes a point with a normal, in the volume frame.  The restatement in numpy
 * is tests/surface_ref.py; device and restatement agree bit for bit, order included.
 *
 * Storage and F = (float)q / 32767.0f are oslam_volume_integrate's.  All arithmetic is float32, grouped as written.
 * Seen.  A voxel is seen iff w >= min_weight.
 * Crossings.  For voxel (i, j, k) and axis a in the order x, y, z the neighbour is (i+1, j, k), (i, j+1, k) or
 *   (i, j, k+1).  The edge exists only if the neighbour's index is below n_a: the last voxel of a row has no +x edge
 *   and does not read the first voxel of the next row.  With q0, q1 the two stored int16 and both voxels seen, the edge
 *   is a crossing iff (q0 < 0) != (q1 < 0): an integer test in which zero counts as positive, so a surface that passes
 *   exactly through a voxel centre is found once, on the edge whose other end is negative.
 * Point.  F0 = (float)q0 / 32767.0f, F1 alike; t = F0 / (F0 - F1) (the denominator is not 0 when the signs differ);
 *   the voxel centre is g_b = origin_b + ((float)idx_b + 0.5f) * voxel; P_a = g_a + t * voxel and P_b = g_b on the two
 *   other axes.
 * Normal.  g_b = F(P + voxel e_b) - F(P - voxel e_b) with the trilinear read of oslam_volume_raycast unchanged: all
 *   eight corners need w > 0 (min_weight does not enter it) and 0 <= b_a <= n_a - 2.  All six reads must have a value;
 *   len = sqrtf((gx*gx + gy*gy) + gz*gz) must satisfy 0 < len <= 3.0e38f; n = g / len.  The TSDF grows towards free
 *   space, so n is the outward normal; there is no camera and hence no facing test.  A crossing without a normal is
 *   counted (result.crossings) and dropped.
 * Order.  Ascending 3 * (i + nx * (j + ny * k)) + a.  Two calls give the same bits; there are no float atomics.
 * oslam_volume_surface: xyz_out and nrm_out [cap][3] are both given or both NULL; both NULL needs cap == 0 and only
 *   counts.  *n_out = the number of points in every case that reached the device; OSLAM_E_LIMIT when outputs are given
 *   and cap is below it (nothing is written, the result is filled).  sp NULL = defaults, res may be NULL.
 * oslam_scene_from_volume: extraction -> voxel grid (leaf > 0; 0 skips) -> scene, the cloud never leaving HBM; leaf,
 *   d_dist, ref_point_downsample_factor, params and n_points_out as in oslam_scene_from_depth, except that the scene
 *   lives on the volume's device (params->dev is not read).  It equals oslam_scene_create over oslam_voxel_grid over
 *   oslam_volume_surface.
 * oslam_volume_set_voxels is the inverse of oslam_volume_voxels, tsdf_q and weight [nz][ny][nx]: it restores a saved
 *   map and is the tests' way to any volume.
 * Arguments are checked before any handle is read or any device call is made: NULL vol, n_out or out, a min_weight
 *   outside 1..65535, one output without the other, NULL outputs with cap > 0, leaf or d_dist below 0 (or NaN) and a
 *   factor of 0 are OSLAM_E_INVALID.
 * Cost: one memset of the totals, k_surface_count and k_surface_scan, one copy back and host wait for the number of
 *   points, then k_surface_emit into a block of exactly that size and one more wait.  Device memory besides the output:
 *   one counter per workgroup of 1024 voxels.  Calls take turns with the other calls on volumes. */
typedef struct oslam_surface_params {
    unsigned min_weight;      /* 1..65535, default 1: a voxel is seen from this weight on */
    int reserved[7];
} oslam_surface_params;

typedef struct oslam_surface_result {
    uint32_t crossings;        /* sign changes along edges between seen voxels */
    uint32_t points;           /* crossings that have a normal: what the call returns */
    uint32_t launches;
    float ms_total;            /* whole call, host clock */
} oslam_surface_result;

int oslam_surface_params_default(oslam_surface_params *p);
int oslam_volume_surface(oslam_volume *vol, const oslam_surface_params *sp, float *xyz_out, float *nrm_out, size_t cap,
                         size_t *n_out, oslam_surface_result *res);
int oslam_scene_from_volume(oslam_volume *vol, const oslam_surface_params *sp, float leaf, float d_dist,
                            unsigned ref_point_downsample_factor, const oslam_params *params, oslam_scene **out,
                            size_t *n_points_out);
int oslam_volume_set_voxels(oslam_volume *vol, const int16_t *tsdf_q, const uint16_t *weight);

/* ---- the fused surface of a whole volume as a triangle mesh by marching cubes (KinFu's marching cubes).  The
 * restatement in numpy is tests/mesh_ref.py; device and restatement agree bit for bit, order included.
 *
 * Storage, F and "seen iff w >= min_weight" are oslam_volume_surface's.  All arithmetic is float32, grouped as written
 * there.
 * Vertices.  Vertex v is the v-th crossing of oslam_volume_surface's rule in its order: every edge between two seen
 *   voxels with (q0 < 0) != (q1 < 0), ascending 3 * voxel + axis, whether or not it has a normal.  Its position is that
 *   rule's P, bit for bit; its normal comes from the same six trilinear reads, and a crossing without a normal keeps
 *   its vertex and gets (0, 0, 0).  So the number of vertices equals oslam_surface_result.crossings, and the vertices
 *   with a non-zero normal, in order, are exactly oslam_volume_surface's points and normals.  With nrm_out == NULL the
 *   normals are not computed at all.
 * Cubes.  Cube (i, j, k) exists for i <= nx-2, j <= ny-2, k <= nz-2 and is full iff all eight corners are seen.  Corner
 *   c = dx + 2*dy + 4*dz is voxel (i+dx, j+dy, k+dz); case = sum((q_c < 0) << c), the integer test, so zero counts as
 *   positive.  Cubes that are not full emit nothing.  Every edge of a full cube joins two seen voxels, so every vertex
 *   a triangle needs exists.  A vertex next to unseen voxels or on the volume's border may be referenced by no
 *   triangle: that is legal, and the unreferenced vertices are not dropped.
 * Cube edges.  e = 4*a + m runs along axis a; m holds the two other offsets in axis order (x: dy + 2*dz, y: dx + 2*dz,
 *   z: dx + 2*dy).  Its global id is 3 * lin(start voxel) + a, oslam_volume_surface's key; 512^3 voxels keep it inside
 *   uint32.
 * Table.  tools/gen_mc_table.py derives csrc/oslam_mc_table.h: for each case and each of the six faces it counts the
 *   sign changes round the face.  Two changes give one segment between the two crossing edges; four changes (the
 *   ambiguous face) give two segments, each joining the two face edges that meet at a NEGATIVE corner.  The rule reads
 *   only the face's four signs, so both cubes at a face agree and the mesh is closed wherever the cubes are full.
 *   Every crossing edge lies on two faces, so the segments close into disjoint loops.  A segment is walked from A to
 *   B so that (B - A) x f, f the face's outward normal, points from the segment towards the negative ends of the two
 *   edges it joins: the single negative corner 0 gives x-edge -> y-edge -> z-edge, and triangle normals point towards
 *   growing F, outwards, like the vertex normals.  A loop is rotated to start at its smallest cube-edge number from
 *   which no fan diagonal lies in a face of the cube, and fanned, (v0, v_i, v_i+1); loops are ordered by their smallest
 *   edge number.  (A diagonal inside an ambiguous face could be laid by the cube behind the face as well, which gives an
 *   edge of four triangles; such an apex exists for every loop, and 18 loops of the table do not start at their smallest
 *   edge because of it.)  At most OSLAM_MC_MAX_TRI = 5 triangles per case.
 * Triangles.  Ascending linear index of the cube's corner voxel, then the row's order; a triangle is three uint32
 *   vertex indices in the row's order.  A corner value of exactly 0 gives t = 0 and hence zero-area triangles: they are
 *   kept, the topology matters more than the area.
 * Determinism.  Two calls give the same bytes; there are no float atomics.
 * oslam_volume_mesh: xyz_out [v_cap][3] and tri_out [t_cap][3] are both given or both NULL; both NULL needs both caps 0
 *   and only counts; nrm_out [v_cap][3] is optional alongside xyz_out.  *nv_out and *nt_out = the numbers of vertices
 *   and triangles in every case that reached the device; OSLAM_E_LIMIT when outputs are given and either cap is below
 *   its count (nothing is written, the result is filled).  A triangle corner whose edge has no vertex (it cannot happen
 *   under the rule above; the kernel checks it like the index checks of the other stages) fails the call with
 *   OSLAM_E_DEVICE and nothing is written.  mp NULL = defaults, res may be NULL.
 * Arguments are checked before any handle is read or any device call is made: NULL vol, nv_out or nt_out, one of
 *   xyz_out and tri_out without the other, nrm_out without xyz_out, NULL outputs with a cap > 0 and a min_weight outside
 *   1..65535 are OSLAM_E_INVALID.
 * Cost: one memset of the totals, k_mesh_count and two runs of k_surface_scan, one copy back and host wait for the two
 *   counts, then k_mesh_vertices and k_mesh_triangles into blocks of exactly those sizes and one more wait.  Device
 *   memory besides the outputs: two counters per workgroup of 1024 voxels and one uint32 edge id per vertex.  Calls
 *   take turns with the other calls on volumes.
 * oslam_ply_write_mesh writes the vertex element as oslam_ply_write writes it (nrm is needed: pass zeros where there are
 *   no normals), then `element face nt` with `property list uchar int vertex_indices`; an index >= nv is
 *   OSLAM_E_INVALID.  oslam_ply_read reads such a file's vertices back and skips the faces.
 * oslam_mc_table_row is a host-only tap on the compiled-in table for the tests: edges_out [15] gets 3 * *n_tri_out
 *   cube-edge numbers.
 * Out of scope: merging or decimating triangles, dropping unreferenced vertices on the device, smoothing, a
 *   min_weight for the normal's corners, one mesh of the live surface and of what oslam_volume_leaving handed over,
 *   several GPUs. */
typedef struct oslam_mesh_params {
    unsigned min_weight;      /* 1..65535, default 1: a voxel is seen from this weight on */
    int reserved[7];
} oslam_mesh_params;

typedef struct oslam_mesh_result {
    uint32_t vertices;         /* crossings: equals oslam_surface_result.crossings */
    uint32_t triangles;
    uint32_t cubes;            /* full cubes with a case other than 0 and 255 */
    uint32_t launches;
    float ms_total;            /* whole call, host clock */
} oslam_mesh_result;

int oslam_mesh_params_default(oslam_mesh_params *p);
int oslam_volume_mesh(oslam_volume *vol, const oslam_mesh_params *mp, float *xyz_out, float *nrm_out, size_t v_cap,
                      uint32_t *tri_out, size_t t_cap, size_t *nv_out, size_t *nt_out, oslam_mesh_result *res);
int oslam_ply_write_mesh(const char *path, const float *xyz, const float *nrm, size_t nv, const uint32_t *tri, size_t nt,
                         int binary);
int oslam_mc_table_row(unsigned mc_case, uint8_t *edges_out, unsigned *n_tri_out);

/* ---- the shifting window: the volume follows the camera by whole voxels and hands over the surface that leaves it
 * (large-scale KinFu's shifting volume).  The volume frame stays the first camera's, so no pose changes meaning; only
 * the window of voxels the volume holds moves.  Integration, ray cast, surface and mesh read the window's origin and
 * are otherwise unchanged.  The restatement in numpy is tests/shift_ref.py; device and restatement agree bit for bit.
 *
 * State.  A volume keeps origin0, the origin it was created with, and an integer window offset off[3] in voxels,
 *   initially 0.  Its origin is derived from the offset, never accumulated: origin_a = origin0_a when off_a == 0 (the
 *   stored float itself, so a -0.0f keeps its sign), otherwise origin_a = origin0_a + (float)off_a * voxel in float32,
 *   one multiply, then one add, not fused.  Shifting out and back gives the created origin bit for bit;
 *   oslam_volume_reset restores off = 0.  A volume that was never shifted behaves bit for bit as one without this section.
 * oslam_volume_shift moves the window by s = shift: the new word at (i, j, k) is the old word at (i + s_x, j + s_y,
 *   k + s_z) when that voxel exists and 0 ("never seen") otherwise; then off += s.  |s_a| >= n_a on any axis clears
 *   everything and is legal.  |s_a| and |off_a + s_a| must stay within 2^20, so that (float)off_a is exact: beyond it
 *   the call returns OSLAM_E_INVALID and nothing changes.  A zero shift returns at once with launches = 0 and kept = 0.
 *   res (may be NULL): offset[3] after the call, kept = the voxels with w > 0 after the shift.
 *   Cost: the words are copied into a second buffer of the volume's size and the two are swapped (in place a workgroup
 *   would read what another has overwritten).  The second buffer is allocated by the first shift that is not zero and
 *   freed by oslam_volume_destroy; when that allocation fails the call returns OSLAM_E_NOMEM and nothing changes.  One
 *   memset of the counter, k_tsdf_shift, one copy back, one host wait.
 * oslam_volume_window is a tap: the current offset and origin.
 * oslam_volume_leaving does not change the volume.  It returns the part of oslam_volume_surface's output that a shift
 *   by `shift` would lose.  Voxel (i, j, k) stays iff 0 <= i - s_x < nx, and likewise for y and z; otherwise it leaves.
 *   A crossing (start voxel, axis a) is leaving iff its start voxel or its neighbour along a leaves: an edge from a
 *   staying voxel into a leaving one has no +a edge after the shift, it would be lost to both sides, so it leaves.
 *   Points, normals and their order are exactly oslam_volume_surface's, restricted to the leaving crossings;
 *   res->crossings counts the leaving crossings and res->points those with a normal; cap, n_out, OSLAM_E_LIMIT and the
 *   count-only call work as there.  So oslam_volume_surface's crossings before a shift are the leaving ones plus the
 *   crossings after it, none lost and none twice.  The caller extracts before it shifts: the normals still read the
 *   voxels that are about to go.  Normals next to the new border are lost or rounded differently after the shift (a
 *   trilinear read needs its eight corners, and the origin is another float): positions carry over, normals do not.
 *   |s_a| is within 2^20 as for oslam_volume_shift.  Cost: oslam_volume_surface's, with k_leave_count and k_leave_emit
 *   (oslam_surface.hip: the bodies of k_surface_count and k_surface_emit, compiled with the leaving mask).
 * oslam_volume_follow is host arithmetic only: it decides a shift and launches nothing.  In double, from the float
 *   inputs: c = t + lookahead * (R02, R12, R22) (the camera's position plus its optical axis), centre_a = origin_a + 0.5 *
 *   n_a * voxel with the window's current origin, d_a = (c_a - centre_a) / voxel.  If |d_a| <= threshold on every axis
 *   the shift is 0; otherwise s_a = granule * (int)rint(d_a / granule) on every axis, clamped to +-n_a.  fp NULL =
 *   oslam_follow_params_default: lookahead = 0.5 * nz * voxel (the default volume at the identity pose has d = 0),
 *   threshold = min(nx, ny, nz) / 4 voxels, granule = 8.  These are policy parameters, not measurements: how far ahead
 *   of the camera the window is centred, how far it may lag and in what steps it moves is the caller's to choose.
 * Arguments are checked before any handle is read or any device call is made: NULL vol, shift, offset_out, origin_out,
 *   T_vol_cam, shift_out or fp (of oslam_follow_params_default), fields that are not finite, lookahead < 0,
 *   threshold < 0, a granule outside 1..64, a T that is not rigid and the surface arguments oslam_volume_surface
 *   refuses are OSLAM_E_INVALID.  Every call takes the lock the other calls on volumes take.
 * Out of scope: merging what left with the live surface into one mesh, several GPUs, any change to
 *   oslam_tracker.  Reloading what left when the window returns is the voxel store's, below (oslam_volume_shift_world). */
typedef struct oslam_shift_result {
    int32_t offset[3];         /* the window's offset after the call, voxels */
    uint32_t kept;             /* voxels with w > 0 after the shift */
    uint32_t launches;
    float ms_total;            /* whole call, host clock */
} oslam_shift_result;

typedef struct oslam_follow_params {
    float lookahead;           /* metres along the optical axis from the camera to the point the window is centred on, >= 0 */
    float threshold;           /* voxels that point may lie off the window's centre on any axis before the window moves, >= 0 */
    int granule;               /* the window moves by multiples of this many voxels, 1..64 */
    int reserved[5];
} oslam_follow_params;

int oslam_volume_shift(oslam_volume *vol, const int shift[3], oslam_shift_result *res);
int oslam_volume_window(oslam_volume *vol, int offset_out[3], float origin_out[3]);
int oslam_volume_leaving(oslam_volume *vol, const int shift[3], const oslam_surface_params *sp, float *xyz_out, float *nrm_out,
                         size_t cap, size_t *n_out, oslam_surface_result *res);
int oslam_follow_params_default(const oslam_volume *vol, oslam_follow_params *fp);
int oslam_volume_follow(oslam_volume *vol, const float T_vol_cam[16], const oslam_follow_params *fp, int shift_out[3]);

/* ---- the voxel store: the voxels that leave the shifting window are kept on the host and come back when the window
 * returns (the other half of large-scale KinFu's shifting volume).  The window and the store together hold every seen
 * voxel exactly once.  Words are 32-bit integers and every statement here is exact; the restatement in numpy is
 * tests/reload_ref.py.  A volume that never meets a store behaves bit for bit as one without this section.
 *
 * Global coordinate.  The window voxel (i, j, k) of a volume with offset off has g = (i + off_x, j + off_y, k + off_z).
 *   By the limits of oslam_volume_shift |g_a| <= 2^20 + 512.
 * A store (oslam_world) is a host-side map from g to words, made for one (voxel, origin0[3]): oslam_world_create checks
 *   that they are finite and voxel > 0, oslam_world_params_of fills them from a volume (max_bytes 0).  A volume whose
 *   voxel and created origin do not have the same float bits is refused by oslam_volume_shift_world with
 *   OSLAM_E_INVALID.  The store needs no device.
 * Seen.  A word is seen iff word >> 16 != 0 (w > 0, k_tsdf_shift's kept).  Only seen words are stored: a word with w == 0
 *   and q != 0 that leaves is dropped and comes back as 0.
 * Who leaves, who enters.  Voxel (i, j, k) leaves under the shift s iff not (0 <= i - s_x < nx and likewise for y and
 *   z): oslam_volume_leaving's rule.  New voxel (i, j, k) enters iff its source (i + s_x, j + s_y, k + s_z) does not exist
 *   in the old window.
 * oslam_volume_shift_world(vol, world, s, res):
 *   1. every seen leaving voxel goes into the store under its g; a key already present (the caller seeded the store, or
 *      shares it between volumes) is overwritten by the leaving word;
 *   2. the window moves exactly as oslam_volume_shift moves it: the same words, off and derived origin;
 *   3. every store entry whose g lies in the entering region is removed from the store and written to its voxel, which
 *      the plain shift left at 0;
 *   4. res (may be NULL): offset[3] after the call, kept = the voxels with w > 0 after all of that, stored = the seen
 *      leaving voxels, reloaded = the entries taken from the store.
 *   |s_a| >= n_a is legal: everything leaves and the whole new window enters.  A zero shift returns at once with
 *   launches = 0 and kept = stored = reloaded = 0.  The limits on s and off are oslam_volume_shift's.
 *   So, with no integration in between, the set {seen voxels of the window by g} u {store} does not change over any
 *   sequence of such shifts and its two parts are disjoint; any path of shifts that returns to an earlier offset restores
 *   the window's seen words bit for bit and leaves the store as it was then.
 *   Failure.  Every error is found before k_tsdf_shift is launched, and then neither the volume, the window nor the store
 *   has changed: NULL arguments and a shift or an offset beyond 2^20 (OSLAM_E_INVALID), an incompatible store
 *   (OSLAM_E_INVALID), the store's max_bytes exceeded by the bricks the leaving voxels need (OSLAM_E_LIMIT), a failed
 *   host or device allocation (OSLAM_E_NOMEM).  The order: pack and copy down; create the bricks the leaving records
 *   need, empty; collect the entering records without changing the store; copy them up, launch k_tsdf_shift and
 *   k_tsdf_unpack; after the host wait write the leaving words into the store, clear the reloaded ones, free the bricks
 *   that became empty and swap the buffers.  A failure after the bricks were created removes them again.
 *   Cost.  launches = 2 (k_tsdf_pack_count and the scan of its counts) + 1 when something seen leaves (k_tsdf_pack_emit)
 *   + 1 (k_tsdf_shift) + 1 when something is reloaded (k_tsdf_unpack): 5 with records on both sides, 3 with none; one
 *   more on a volume with colour, whose colours are shifted too (oslam_volume_integrate_colour below).  Host
 *   waits: one for the pack's total, which sizes the records' buffer and their copy; one for that copy when something
 *   seen leaves (the bricks are created from the records, before the shift is launched); one for k_tsdf_shift and
 *   k_tsdf_unpack.  The records' staging buffers are pinned, kept with the store and grown on demand: after the first
 *   shifts a call allocates no host memory beyond new bricks.
 * The store: bricks of 8 x 8 x 8 words keyed by floor(g_a / 8) (an arithmetic shift: g may be negative) in an
 *   open-addressing table that grows; a brick carries its number of seen words and is freed when that reaches 0.
 *   max_bytes bounds bricks plus table (0 = 1 GiB): a call that would exceed it returns OSLAM_E_LIMIT and changes
 *   nothing.  The store has its own lock, taken inside the lock of the calls on volumes and never the other way round.
 * oslam_world_put stores n words under g [n][3]; unseen words are skipped, a later record of the same g wins, |g_a| beyond
 *   2^20 + 512 is OSLAM_E_INVALID.  oslam_world_box reads the box lo <= g < hi densely into words_out
 *   [hz - lz][hy - ly][hx - lx], 0 where nothing is stored; take != 0 also removes what it read.  lo_a <= hi_a and both
 *   within 2^21 in size, otherwise OSLAM_E_INVALID; a box of more than 2^27 voxels is OSLAM_E_LIMIT.
 *   oslam_world_stats_get: stored voxels, bricks, bytes of bricks plus table, and the bounding box of the stored g (hi
 *   exclusive, all 0 when empty).  oslam_world_clear empties the store.  oslam_volume_reset does not touch a store.
 * oslam_volume_pack is a test tap and changes nothing: the records {lin, word} that k_tsdf_pack_count and
 *   k_tsdf_pack_emit make for this shift, lin = (k * ny + j) * nx + i of the old window, ascending.  cap == 0 counts only
 *   (the outputs may be NULL); more records than cap is OSLAM_E_LIMIT with the count in *n_out and nothing written.
 * Colour.  A store keeps colour when it is created with oslam_world_params.colour = 1 (oslam_world_params_of writes 0:
 *   the store of before, bit for bit: 2064 bytes per brick, the same stats, the same launches).  A colour store's bricks
 *   carry a second array of 512 colour words (4112 bytes per brick; bytes, max_bytes and the rollback count that): a
 *   voxel's colour word r | g << 8 | b << 16 | wc << 24 is stored under its g, as it is, whenever its TSDF word is stored.
 *   That means seen voxels only, whatever their wc; the colour of an unseen voxel that leaves is dropped.  The bricks are
 *   created with both arrays, so storing still cannot fail.  The restatement in numpy is tests/reload_colour_ref.py.
 *   oslam_world_has_colour: 1 for a colour store, 0 otherwise (NULL included).  oslam_world_put_colour is oslam_world_put
 *   with the colour word of every record (colours [n]); OSLAM_E_INVALID on a plain store.  On a colour store plain
 *   oslam_world_put stores colour 0 (a later record wins, colour included).  oslam_world_box_colour is oslam_world_box with
 *   a second dense output for the colour words, 0 where nothing is stored; take removes word and colour; oslam_world_box's
 *   limits; OSLAM_E_INVALID on a plain store.  Plain oslam_world_box on a colour store reads the words.
 *   The shift.  With a coloured volume and a colour store every leaving record takes its voxel's colour word along, and
 *   every reloaded record brings its colour word back, into the colour buffer that the shift of the colours wrote and
 *   that is swapped in with it.  A colour store with a volume without colour is OSLAM_E_INVALID before any device call,
 *   with nothing changed.  A coloured volume through a plain store behaves as before: the colours move with the window,
 *   what leaves loses its colour and what is reloaded comes back with wc = 0.
 *   The invariant, extended: with no integration in between, a path of shifts that returns to an earlier offset restores
 *   the colour words of the window's seen voxels bit for bit and leaves the store as it was.  Colour words of unseen
 *   voxels behave as their TSDF words do under the plain shift: kept while they stay in the window, 0 once they have left.
 *   Cost.  A record crosses the host link as 12 bytes instead of 8: the colours are gathered behind k_tsdf_pack_emit into
 *   the block that holds the records (k_pack_colours, one thread per record, by the record's lin) and go down in the
 *   records' copy; on the way up they ride in the records' copy too and are scattered behind the colours' k_tsdf_shift
 *   (k_unpack_colours).  The pinned staging buffers are sized for it.  The number of host waits does not grow.  launches
 *   = the count above for a coloured volume (one more than for a volume without colour) + 1 when something seen leaves +
 *   1 when something is reloaded: 8 with records on both sides, 4 with none.  Failure changes nothing, as above, for both
 *   buffers and the store.
 *   oslam_volume_pack_colour is oslam_volume_pack with the records' colour words (colour_out [cap]), as a colour store
 *   gets them; OSLAM_E_INVALID on a volume without colour.
 * Out of scope: store files on disk, colour in the hand-over list of oslam_volume_leaving, several GPUs, any change to
 *   oslam_tracker.  (The one surface of store plus window is oslam_world_surface below, their one mesh oslam_world_mesh,
 *   the colour at their points oslam_world_colours.) */
typedef struct oslam_world oslam_world;
typedef struct oslam_world_params {
    float voxel;               /* the voxel size of the volumes the store serves, metres */
    float origin0[3];          /* their created origin */
    uint64_t max_bytes;        /* bound on bricks plus table, 0 = 1 GiB */
    int colour;                /* 1 = a colour store: every brick keeps a colour word next to each TSDF word; 0 = none */
    int reserved[3];
} oslam_world_params;

typedef struct oslam_world_stats {
    uint64_t voxels, bricks, bytes;
    int32_t lo[3], hi[3];      /* bounding box of the stored g, hi exclusive; all 0 when empty */
} oslam_world_stats;

typedef struct oslam_reload_result {
    int32_t offset[3];         /* the window's offset after the call, voxels */
    uint32_t kept;             /* voxels with w > 0 after the shift and the reload */
    uint32_t stored;           /* seen voxels that left, now in the store */
    uint32_t reloaded;         /* entries taken from the store into the window */
    uint32_t launches;
    float ms_total;            /* whole call, host clock */
} oslam_reload_result;

int oslam_world_params_of(const oslam_volume *vol, oslam_world_params *p);
int oslam_world_create(const oslam_world_params *p, oslam_world **out);
int oslam_world_destroy(oslam_world *w);
int oslam_world_clear(oslam_world *w);
int oslam_world_stats_get(oslam_world *w, oslam_world_stats *out);
int oslam_world_put(oslam_world *w, const int32_t *g, const uint32_t *words, size_t n);
int oslam_world_box(oslam_world *w, const int32_t lo[3], const int32_t hi[3], uint32_t *words_out, int take);
int oslam_volume_shift_world(oslam_volume *vol, oslam_world *w, const int shift[3], oslam_reload_result *res);
int oslam_volume_pack(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, size_t cap, size_t *n_out);
int oslam_world_has_colour(const oslam_world *w);
int oslam_world_put_colour(oslam_world *w, const int32_t *g, const uint32_t *words, const uint32_t *colours, size_t n);
int oslam_world_box_colour(oslam_world *w, const int32_t lo[3], const int32_t hi[3], uint32_t *words_out, uint32_t *colours_out,
                           int take);
int oslam_volume_pack_colour(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, uint32_t *colour_out,
                             size_t cap, size_t *n_out);

/* ---- the surface of the whole map: voxel store plus window as one cloud, extracted on the device from sparse
 * 8 x 8 x 8 bricks with no dense box anywhere.  The restatement in numpy is tests/world_surface_ref.py; device and
 * restatement agree bit for bit, order and keys included.
 *
 * The map.  G(g) is a 32-bit word for every global voxel coordinate g.  Inside the window's box (off <= g < off + n) it is
 *   the window's word, seen or not; elsewhere it is the store's word, or 0 where the store has nothing.  A store entry
 *   inside the window's box is ignored (there is none after oslam_volume_shift_world alone; a caller's oslam_world_put can
 *   make one).  With vol == NULL the map is the store alone.
 * The frame.  An anchor A[3] in voxels picks it: by default the window's offset when a volume is given and 0 otherwise;
 *   the caller may set it (anchor_set != 0), |A_a| <= 2^20.  O = origin(A), derived exactly as oslam_volume_shift derives
 *   an origin from an offset: origin0_a itself where A_a == 0, otherwise origin0_a + (float)A_a * voxel, one multiply,
 *   then one add, not fused.  A voxel's index is r = g - A, a signed int, |r_a| < 2^22.
 * Crossings, points, normals are oslam_volume_surface's with idx = r, origin = O and "outside the volume" replaced by
 *   "G is 0 there":
 *   Crossings.  Every voxel has its three +axis edges; there is no last-voxel rule, because there is no box.  Both ends
 *     must be seen (w >= min_weight), with the integer sign test (q0 < 0) != (q1 < 0).
 *   Point.  P_b = O_b + ((float)r_b + 0.5f) * voxel, plus t * voxel on the edge's axis, t = F0 / (F0 - F1).
 *   Normal.  oslam_volume_surface's six trilinear reads with the arithmetic unchanged in grouping: g = (p - O_b) *
 *     inv_voxel - 0.5f with inv_voxel = 1.0f / voxel, b = floorf(g); the range test on bx, by, bz becomes "finite and
 *     |b| < 2^22"; the eight corners are read from G at A + b + (0|1), each needing w > 0.  A crossing without a normal
 *     is counted (result.crossings) and dropped.
 * Equality with a dense volume.  Take a dense oslam_volume with the same voxel and created origin, at offset A, whose
 *   words are G over a box that contains every seen voxel of the map with a margin of at least 3 voxels on every side.
 *   Then oslam_volume_surface returns the same crossings, the same number of them, and bit-identical points and normals.
 *   With the default anchor a crossing whose stencil lies inside the window has the bits oslam_volume_surface gives it.
 * Order.  Bricks ascend by key (bz, by, bx) with b = floor(g / 8); inside a brick the order is 3 * (i + 8 * (j + 8 * k))
 *   + a.  Two calls give the same bits; there are no float atomics.  key_out (may be NULL; needs the other outputs)
 *   int32 [cap][4] holds (g_x, g_y, g_z, a) of every returned point: sorting by (g_z, g_y, g_x, a) gives the dense
 *   volume's order.
 * oslam_world_surface: the output conventions are oslam_volume_surface's: xyz_out and nrm_out both or neither, both NULL
 *   needs cap == 0 and only counts; OSLAM_E_LIMIT comes with *n_out and the result filled in and nothing written.
 *   Refused before any device call with OSLAM_E_INVALID: NULL w or n_out, a min_weight outside 1..65535, an anchor beyond
 *   2^20, a volume whose voxel or created origin bits are not the store's (as oslam_volume_shift_world refuses it).  A map
 *   of more than 2^22 bricks is OSLAM_E_LIMIT.  The lock of the calls on volumes is taken, then the store's, as
 *   everywhere; neither the store nor the volume changes.  params.dev is read only when vol == NULL.
 * oslam_world_bricks is device-free: the brick keys floor(g / 8) of the store as keys_out [cap][3], ascending by
 *   (bz, by, bx).  cap == 0 counts only (keys_out may be NULL); more bricks than cap is OSLAM_E_LIMIT with the count in
 *   *n_out and nothing written.  A test tap, and what the surface call uses.
 * oslam_scene_from_world is oslam_scene_from_volume's chain with this extraction at its head, the cloud never leaving
 *   HBM: it equals oslam_scene_create over oslam_voxel_grid over oslam_world_surface.  The scene lives on the volume's
 *   device, or on sp->dev without a volume (params->dev is not read).
 * Cost.  Host: the store's brick keys are collected and sorted and united with the keys of the aligned bricks that the
 *   window's box overlaps (its offset need not be a multiple of 8).  The device holds a table (packed 64-bit key, slot),
 *   ascending, and an array of [512]-word bricks: the store's go up through the store's pinned buffer together with the
 *   table in one copy, window-only bricks are zeroed by one memset, and k_brick_window writes the window's words into the
 *   bricks it overlaps, so they never cross the host link.  A brick the window fills with nothing seen stays in the table
 *   and yields nothing.  Then k_brick_count, one k_surface_scan per 2^17 bricks, one copy back and host wait for the
 *   totals, k_brick_emit into a block of exactly the points' size and one more wait.  Device memory is freed before
 *   return on every path.
 * Out of scope: colours written by the extraction itself (oslam_world_colours below colours the points afterwards), store
 *   files on disk, several GPUs.  (The mesh of the whole map is oslam_world_mesh below.) */
typedef struct oslam_world_surface_params {
    unsigned min_weight;       /* 1..65535, default 1: a voxel is seen from this weight on */
    int anchor_set;            /* 0: the window's offset, or 0 without a volume */
    int32_t anchor[3];
    int dev;                   /* read only when vol == NULL */
    int reserved[6];
} oslam_world_surface_params;

typedef struct oslam_world_surface_result {
    uint32_t crossings;        /* sign changes along edges between seen voxels of the map */
    uint32_t points;           /* crossings that have a normal: what the call returns */
    uint32_t bricks;           /* table entries: the store's bricks united with the window's */
    uint32_t window_bricks;    /* aligned bricks the window's box overlaps */
    uint32_t launches;
    int32_t anchor[3];         /* the anchor in force */
    float ms_total;            /* whole call, host clock */
} oslam_world_surface_result;

int oslam_world_surface_params_default(oslam_world_surface_params *p);
int oslam_world_surface(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, float *xyz_out, float *nrm_out,
                        int32_t *key_out, size_t cap, size_t *n_out, oslam_world_surface_result *res);
int oslam_world_bricks(oslam_world *w, int32_t *keys_out, size_t cap, size_t *n_out);
int oslam_scene_from_world(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, float leaf, float d_dist,
                           unsigned ref_point_downsample_factor, const oslam_params *params, oslam_scene **out,
                           size_t *n_points_out);

/* ---- the mesh of the whole map: voxel store plus window as one marching-cubes mesh, extracted on the device from the
 * sparse 8 x 8 x 8 bricks of oslam_world_surface with no dense box anywhere.  The restatement in numpy is
 * tests/world_mesh_ref.py; device and restatement agree bit for bit, order included.
 *
 * Map, frame, anchor and "seen" are oslam_world_surface's, word for word: the map G(g) with "a store entry inside the
 *   window's box is ignored" and the store alone for vol == NULL; the anchor A, |A_a| <= 2^20, by default the window's
 *   offset or 0; O = origin(A) and r = g - A; a voxel is seen iff w >= min_weight.
 * Vertices.  Vertex v is the v-th crossing of oslam_world_surface's rule in its order, with or without a normal: bricks
 *   ascending by (bz, by, bx), inside a brick 3 * (i + 8 * (j + 8 * k)) + a.  Its position is that rule's P; its normal
 *   comes from the same six trilinear reads, and a crossing without a normal keeps its vertex and gets (0, 0, 0).  So the
 *   number of vertices equals oslam_world_surface_result.crossings, and the vertices with a non-zero normal, in order, are
 *   oslam_world_surface's points, normals and keys bit for bit.  With nrm_out == NULL the six reads are not made.
 * Cubes.  Every global voxel g is the corner of a cube; there is no box, so there is no last-cube rule.  A cube is full iff
 *   all eight G(g + (dx, dy, dz)) are seen.  Corner numbering, the integer sign test, the edge numbering e = 4 * a + m, the
 *   table and its row order are oslam_volume_mesh's.  Cubes that are not full emit nothing, so a cube next to an absent
 *   brick is silent, and the vertices on its edges stay in the output, unreferenced.
 * Triangles.  Table entries ascend; inside a brick the cube's corner voxel ascends by i + 8 * (j + 8 * k); then the row's
 *   order.  A triangle is three uint32 vertex indices; zero-area triangles are kept.
 * Equality with a dense volume.  Take oslam_world_surface's dense volume: the same voxel and created origin, at offset A,
 *   whose words are G over a box that holds every seen voxel of the map with a margin of at least 3.  oslam_volume_mesh on
 *   it gives the same vertices bit for bit, by that rule's argument.  With each vertex index mapped to its key (g_x, g_y,
 *   g_z, a) the triangles are the same triples of keys in the same rotation, and sorted (stably) by the cube's (g_z, g_y,
 *   g_x) they stand in the dense volume's order.
 * Determinism.  Two calls give the same bytes; there are no float atomics.
 * oslam_world_mesh: the parameters are oslam_world_surface's.  The output conventions are oslam_volume_mesh's: xyz_out
 *   [v_cap][3] and tri_out [t_cap][3] are both given or both NULL; both NULL needs both caps 0 (and no nrm_out or key_out)
 *   and only counts; nrm_out [v_cap][3] and key_out int32 [v_cap][4] = (g_x, g_y, g_z, a), one row per vertex, are optional
 *   alongside xyz_out.  *nv_out and *nt_out = the numbers of vertices and triangles in every case that reached the
 *   device; OSLAM_E_LIMIT when outputs are given and either cap is below its count, with the counts and the result filled
 *   in and nothing written.  A triangle corner whose edge has no vertex (it cannot happen under the rule; the kernel
 *   checks it like its index checks) fails the call with OSLAM_E_DEVICE and nothing written.
 *   Refused before any device call with OSLAM_E_INVALID, in oslam_world_surface's order: NULL w, nv_out or nt_out, one of
 *   xyz_out and tri_out without the other, NULL outputs with a cap > 0 or with nrm_out or key_out, a min_weight outside
 *   1..65535, an anchor beyond 2^20, a volume whose voxel or created origin bits are not the store's.  OSLAM_E_LIMIT also
 *   for a map of more than 2^22 bricks and for a vertex or triangle total beyond uint32 (the chunks' sums are added in 64
 *   bits on the host; *nv_out and *nt_out hold the totals, the result's fields their limit).  The lock of the calls on
 *   volumes is taken, then the store's; neither the store nor the volume changes; device memory is freed before return on
 *   every path; an empty store without a volume returns zero counts without a device call.
 * Cost.  The map goes up as for oslam_world_surface.  k_wmesh_count writes two counters per table entry, each array is
 *   scanned in chunks of 2^17 entries; one copy back and host wait; k_wmesh_vertices and k_wmesh_triangles write into
 *   blocks of exactly the two totals; one more wait.  A triangle corner's vertex lies in the brick of its edge's start
 *   voxel, this one or a +x/+y/+z neighbour: its index is that entry's first vertex plus the rank of 3 * (voxel in the
 *   brick) + a among the entry's at most 1536 ids, found by binary search.  Device memory besides the map and the outputs:
 *   those two counters and one uint32 id per vertex; nothing proportional to the number of voxels.
 * Out of scope: colours written by the extraction itself (oslam_world_colours below colours the vertices afterwards),
 *   merging or decimating triangles, dropping unreferenced vertices, store files on disk, several GPUs. */
typedef struct oslam_world_mesh_result {
    uint32_t vertices;         /* crossings: equals oslam_world_surface_result.crossings */
    uint32_t triangles;
    uint32_t cubes;            /* full cubes with a case other than 0 and 255 */
    uint32_t bricks;           /* table entries: the store's bricks united with the window's */
    uint32_t window_bricks;    /* aligned bricks the window's box overlaps */
    uint32_t launches;
    int32_t anchor[3];         /* the anchor in force */
    float ms_total;            /* whole call, host clock */
} oslam_world_mesh_result;

int oslam_world_mesh(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, float *xyz_out, float *nrm_out,
                     int32_t *key_out, size_t v_cap, uint32_t *tri_out, size_t t_cap, size_t *nv_out, size_t *nt_out,
                     oslam_world_mesh_result *res);

/* ---- the whole map ray-cast back into a view: voxel store plus window seen from a pose, marched on the device through
 * the sparse 8 x 8 x 8 bricks of oslam_world_surface with no dense box anywhere.  The result is a genuine oslam_view, so
 * whatever takes a ray-cast view of the window (oslam_view_egomotion, oslam_track, oslam_verify, oslam_arbitrate,
 * oslam_view_to_cloud) can look at what the store keeps, without shifting the window back.  The restatement in numpy is
 * tests/world_raycast_ref.py; device and restatement agree byte for byte.
 *
 * The rule is oslam_volume_raycast's, float sequence and grouping unchanged, with four substitutions.
 * Map and frame.  G(g), the anchor A, O = origin(A) and r = g - A are oslam_world_surface's, word for word: inside the
 *   window's box G is the window's word, elsewhere the store's or 0; a store entry inside the window's box is ignored; with
 *   vol == NULL the map is the store alone.  The default anchor is the window's offset, or 0 without a volume; the
 *   caller may set it, |A_a| <= 2^20.  origin becomes O, voxel and inv_voxel = 1.0f / voxel are the store's, mu is
 *   params.mu, or the volume's when that is 0.  The trilinear read is oslam_world_surface's: c_a = (P_a - O_a) *
 *   inv_voxel - 0.5f, b = floorf(c), the range test "finite and |b_a| < 2^22", the eight corners G at A + b + (0|1), each
 *   needing w > 0.
 * Box.  The dense rule takes its interval from the volume's box; here it comes from a box B = [box_lo, box_hi) in global
 *   voxels: by default the bounding box of the map's bricks, 8 * (the least brick coordinate) to 8 * (the greatest + 1)
 *   per axis, the bricks the window's box overlaps included; otherwise the caller's (box_set != 0).  With r_lo = box_lo_a
 *   - A_a and r_hi = box_hi_a - A_a: lo = O_a + (float)(r_lo + 1) * voxel and hi = O_a + (float)(r_hi - 1) * voxel, each
 *   one convert, one multiply and one add, not fused.  The slab test, tn, tf, t_k = tn + (float)k * step and step = 0.5f *
 *   mu are unchanged.  A box is needed although the map has none: the samples hang on tn, so two calls see the same
 *   samples only under the same box.
 * Sample.  The word is G at A_a + floorf((P_a - O_a) * inv_voxel) per axis, under the range test "finite and below 2^22
 *   in size", made in float before the conversion; it is 0 (w = 0) otherwise.  Samples are not confined to B.
 * Step bound.  The march runs while t_k <= tf and k < 65536.  A call with (double)(z_max - z_min) / (double)step >= 65535
 *   is refused with OSLAM_E_LIMIT, so the bound never ends a ray.
 * The crossing, t*, the six-read gradient, the normal into the camera frame and its facing test are unchanged, and so are
 *   the view's records: the z image, the 32-byte map records x y z 1 | nx ny nz 0, max_jump from cam.  The view is the
 *   caller's (oslam_view_destroy), on the volume's device or on params.dev.
 * Three pins.  (a) Dense.  Take a dense oslam_volume with the same voxel, created origin and mu, at offset A = box_lo with
 *   sides box_hi - box_lo, holding G over B, and let the map have no seen voxel outside B: oslam_volume_raycast gives the
 *   same z image and maps byte for byte, and the same hits and normals.  (b) Window alone.  With an empty store, the
 *   default anchor and B the window's box the call equals oslam_volume_raycast(vol, ...) byte for byte.  (c) Walk.  Fuse
 *   frames, ray-cast the volume, shift it away through a store with no integration in between: this call with anchor =
 *   the old offset and B = the old window's box gives the bytes the volume gave.
 * Refused before any device call, with nothing written, OSLAM_E_INVALID: NULL w, T_vol_cam, cam or view_out; a pose that
 *   is not rigid; a camera oslam_view_create would refuse; a size outside 1..16384; an anchor beyond 2^20; a box with
 *   hi_a - lo_a < 2 or a corner beyond 2^20 + 520 in size; a mu that is not finite, is negative or, when set, lies below 2
 *   voxels; mu == 0 without a volume; a volume whose voxel or created-origin bits are not the store's.  OSLAM_E_LIMIT: the
 *   step bound above, and a map of more than 2^22 bricks.  An empty map (no store bricks, no volume) returns a view of
 *   zeros with launches == 0.  The lock of the calls on volumes is taken, then the store's; neither changes; device memory
 *   other than the view is freed on every path.
 * Device side.  The map goes up as for oslam_world_surface.  k_brick_raycast runs one thread per pixel in k_tsdf_raycast's
 *   32 x 8 tiles; every read goes through the table, and a lane keeps the brick of its last sample (key and slot, "absent"
 *   included), which only memoises the search.  No LDS, no scratch, no float atomic; hits and normals are counted by
 *   ballots; two calls give the same bytes.  One launch besides the map's (k_brick_window with a volume), one host wait.
 * oslam_world_track is oslam_volume_track's glue with this ray cast at its head: the map is ray-cast at T_vol_cam_prev with
 *   the frame's own camera and size, then oslam_view_egomotion and the product as there; launches + the ray cast's.  A map
 *   without a volume goes to the view's device (rp->dev is not read).  Under pin (b) it equals oslam_volume_track bit for
 *   bit.  It integrates nothing.
 * Out of scope: a map kept on the device between calls (every call sends the store's bricks up again), skipping absent
 *   bricks by jumping k, integration into bricks, several GPUs. */
typedef struct oslam_world_raycast_params {
    int anchor_set;            /* 0: the window's offset, or 0 without a volume */
    int32_t anchor[3];
    int box_set;               /* 0: the bounding box of the map's bricks */
    int32_t box_lo[3], box_hi[3];   /* global voxels, hi exclusive */
    float mu;                  /* 0 = the volume's; needed (> 0) without a volume */
    int dev;                   /* read only when vol == NULL */
    int reserved[6];
} oslam_world_raycast_params;

typedef struct oslam_world_raycast_result {
    uint32_t hits;             /* pixels with a hit */
    uint32_t normals;          /* pixels with a normal */
    uint32_t bricks;           /* table entries: the store's bricks united with the window's */
    uint32_t window_bricks;    /* aligned bricks the window's box overlaps */
    uint32_t launches;
    int32_t anchor[3], box_lo[3], box_hi[3];   /* in force */
    float ms_total;            /* whole call, host clock */
} oslam_world_raycast_result;

int oslam_world_raycast_params_default(oslam_world_raycast_params *p);
/* vol, rp (defaults) and res may be NULL */
int oslam_world_raycast(oslam_world *w, oslam_volume *vol, const oslam_world_raycast_params *rp, const float T_vol_cam[16],
                        const oslam_camera *cam, int width, int height, oslam_view **view_out, oslam_world_raycast_result *res);
/* vol, rp, ep (defaults) and ego_res may be NULL */
int oslam_world_track(oslam_world *w, oslam_volume *vol, const oslam_world_raycast_params *rp, oslam_view *v,
                      const float T_vol_cam_prev[16], const oslam_egomotion_params *ep, float T_vol_cam_out[16],
                      oslam_egomotion_result *ego_res);

/* ---- normals for clouds and meshes that come without them.  Every entry into the recognition path takes points and
 * normals; the reference made them outside its program (matlab/compute_normals.m for meshes, PCL for scans).  Two entry
 * points, because the two kinds of input need different sign rules: a cloud seen from somewhere (oslam_cloud_normals, on
 * the device) and a closed mesh (oslam_mesh_normals, on the host).  The restatement in numpy is tests/normals_ref.py; the
 * device agrees with it bit for bit.
 *
 * oslam_cloud_normals: the rule.  It does not depend on the order in which neighbours are met (the cells of the grid
 * hold their points in an order that differs from run to run).  For point i with finite coordinates:
 *   1. Neighbours.  Every point j, i included, with d = p_j - p_i and d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius, all in
 *      float32 with this grouping (the refinement's correspondence test has the same form).  A non-finite coordinate
 *      fails the test by itself: such a point is nobody's neighbour and gets no normal.
 *   2. Moments as whole numbers.  q_a = (int32) rintf(d_a * scale), scale = 16384.0f / radius (float32, made once by the
 *      host).  Summed in int64: the count n, Sq_a (x y z) and Sqq_ab in the order xx xy xz yy yz zz.  These ten integers
 *      are what oslam_cloud_normal_moments returns per point ([n][10]: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz).
 *   3. Covariance in double, about the neighbours' mean, from the ten integers converted with round-to-nearest:
 *      a_ab = Sqq_ab / n - (Sq_a / n) * (Sq_b / n), in exactly this operation order.
 *   4. Principal axes.  OSLAM_NORMALS_SWEEPS cyclic Jacobi sweeps in double over the pairs (p, q) = (0,1), (0,2), (1,2),
 *      from V = I, with + - * / sqrt and comparisons only.  A pair whose a_pq is exactly 0 is skipped; otherwise
 *      theta = (a_qq - a_pp) / (2 * a_pq), t = sign(theta) / (|theta| + sqrt(theta*theta + 1)) (sign(0) = +1),
 *      c = 1 / sqrt(t*t + 1), s = t * c; h = t * a_pq, a_pp -= h, a_qq += h, a_pq = 0; with r the third index
 *      (a_rp, a_rq) = (c*a_rp - s*a_rq, s*a_rp + c*a_rq); every row k of V: (v_kp, v_kq) = (c*v_kp - s*v_kq,
 *      s*v_kp + c*v_kq).  The count is fixed (no convergence test that could differ between lanes): 4 is the smallest
 *      count after which one more sweep changes no float32 output on the calibration clouds (the fourth
 *      sweep still changes 20 to 809 outputs per cloud, the fifth, sixth and seventh change none).
 *      lmin, lmid, lmax = the diagonal sorted by comparisons; the normal is the column of V under the smallest diagonal
 *      element (lowest index on a tie), divided in double by sqrt((x*x + y*y) + z*z), then rounded to float32.
 *      curvature = (float)(lmin / ((a_00 + a_11) + a_22)), or 0 when that sum is 0.
 *   5. Validity.  n >= min_neighbours and lmid > (double)line_ratio * lmax: coincident or collinear neighbours have no
 *      normal.  An invalid point gets normal (0, 0, 0), curvature 0 and valid 0.
 *   6. Sign.  With orient = 1 the normal is negated when (nx*(vx - px) + ny*(vy - py)) + nz*(vz - pz) < 0, evaluated in
 *      double with the unrounded normal, v = viewpoint and p = p_i converted to double.  An exact 0 keeps the sign.
 * xyz: host points with stride_bytes between them (12 = packed, 48 = pcl::PointNormal); nrm_out packed float[n][3],
 * curvature_out float[n] and valid_out uint8[n] may be NULL.  n >= 1.  The neighbourhood grid is the refinement stage's
 * (edge = radius, enlarged by the same rule when the cell count would pass 2^24; res->edge is the edge in force), then one
 * kernel with one thread per grid position.  The call holds the device's lock like every call that launches, returns
 * OSLAM_E_DEVICE without a device and OSLAM_E_INVALID for NULL xyz / nrm_out / params, n == 0 or above 2^31 - 1,
 * stride_bytes < 12, a radius that is not > 0 and finite, min_neighbours < 3, a non-finite viewpoint and a line_ratio
 * that is not >= 0 and finite.  A refused call writes nothing.
 *
 * oslam_mesh_normals (host): for every triangle (a, b, c) in order, (p_b - p_a) x (p_c - p_a) in double is added to its
 * three vertices (area weighting); each sum is divided by sqrt((x*x + y*y) + z*z) and rounded to float32.  Counter-
 * clockwise triangles seen from outside give outward normals.  A vertex whose sum is zero or not finite (unreferenced,
 * only degenerate triangles) gets (0, 0, 0) and valid 0.  An index >= nv fails the call with OSLAM_E_INVALID and writes
 * nothing.  valid_out may be NULL.  The reference does not say how MATLAB's vertexNormal weights faces: this rule is the
 * library's own.
 *
 * oslam_ply_read_mesh (host): ascii and binary_little_endian; the vertex element first with x y z, normals only when
 * nx ny nz (or normal_x normal_y normal_z) are all there (*nrm_out = NULL otherwise); the face element's list property
 * vertex_indices or vertex_index with any integer count and index type; polygons with more than 3 corners become the
 * fans (0, k, k+1), fewer than 3 corners are dropped; an index outside the vertices is OSLAM_E_INVALID.  A file without
 * faces gives *nt_out = 0 and *tri_out = NULL.  Other elements and properties are skipped.  The arrays are malloc'd,
 * release with oslam_free.  oslam_ply_read is unchanged: it still needs normals and skips faces.
 * Out of scope: handing the device-resident normals to oslam_scene_create without the host round trip, k-nearest
 * neighbourhoods, a sign propagation for viewpoint-free clouds, oslam_pcl.hpp. */
#define OSLAM_NORMALS_SWEEPS 4
typedef struct oslam_normals_params {
    float radius;              /* no default: must be > 0 and finite, in the cloud's units */
    unsigned min_neighbours;   /* 5; at least 3; the point itself counts */
    float viewpoint[3];        /* 0 0 0 */
    int orient;                /* 1 = towards the viewpoint, 0 = leave the solver's sign */
    float line_ratio;          /* 0.01: valid needs lmid > line_ratio * lmax */
    int reserved[4];
} oslam_normals_params;

typedef struct oslam_normals_result {
    uint32_t n_valid;
    uint32_t n_cells;          /* cells of the neighbourhood grid */
    float edge;                /* its edge: the radius (times 1 + 1e-4), or larger when the cell cap enlarged it */
    uint32_t launches;
    float ms_total;            /* whole call, host clock */
    float ms_grid, ms_kernel;  /* the grid build and the normals kernel on the stream (device events) */
} oslam_normals_result;

int oslam_normals_params_default(oslam_normals_params *p);
int oslam_cloud_normals(const float *xyz, size_t n, size_t stride_bytes, const oslam_normals_params *np, int dev,
                        float *nrm_out, float *curvature_out, uint8_t *valid_out, oslam_normals_result *res);
/* test tap: the ten integers of step 2 per point, moments_out int64[n][10] */
int oslam_cloud_normal_moments(const float *xyz, size_t n, size_t stride_bytes, const oslam_normals_params *np, int dev,
                               int64_t *moments_out);
int oslam_mesh_normals(const float *xyz, size_t nv, size_t stride_bytes, const uint32_t *tri, size_t nt, float *nrm_out,
                       uint8_t *valid_out);
int oslam_ply_read_mesh(const char *path, float **xyz_out, float **nrm_out, uint32_t **tri_out, size_t *nv_out,
                        size_t *nt_out);

/* ---- the dominant planes of a view, found and removed on the device.  In an indoor frame almost all of the scene is
 * floor and wall; KinFu-based object pipelines (SLAM++) take the supporting planes away before they look for objects.
 * oslam_view_planes finds up to OSLAM_PLANES_MAX planes of a view and labels their pixels, oslam_view_remove_planes returns
 * the view without them or with them alone.  The restatement in numpy is tests/planes_ref.py; device and restatement agree
 * bit for bit, and two calls give the same bytes: every gate is a float32 expression with the grouping written here
 * (the build's -ffp-contract=off keeps the operations apart) and every sum is a whole number, so nothing depends on the
 * order of pixels, waves or workgroups.
 *
 * Inputs per pixel: the view's z image and its vertex and normal maps (oslam_view_maps' [h][w][8], built when absent).  The
 *   point of a valid pixel (z > 0) is p = ((((float)u - cx) * z) / fx, (((float)v - cy) * z) / fy, z), the vertex map's
 *   value bit for bit where the pixel has a normal (has == 1).  A pixel is free when it is valid and carries no label yet.
 * Rounds r = 0 .. max_planes - 1 peel one plane each:
 *   1. Candidates.  The 256 nodes of a 16 x 16 lattice: node (a, b), index 16 b + a, is pixel u = ((2a + 1) * w) / 32,
 *      v = ((2b + 1) * h) / 32 in integer division.  A node is a candidate of this round when its pixel is free and has a
 *      normal; its plane is the pixel's own normal n0 with d0 = -((n0x*p0x + n0y*p0y) + n0z*p0z).  On small images nodes
 *      coincide; duplicates stay.
 *   2. Score.  count[c] = the free pixels with a normal that pass fabsf(((n0x*px + n0y*py) + n0z*pz) + d0) <= dist_tol and
 *      (n0x*nx + n0y*ny) + n0z*nz >= min_normal_dot; 0 for a node that is no candidate.  The winner is the candidate with
 *      the largest count, the lowest index on a tie.  The search ends when no node is a candidate or the winner's count is
 *      below min_pixels (0 = w * h / 50 in integer division); everything found so far stands.
 *   3. Refit.  Over the winner's inliers (the pixels its count counted), moments as whole numbers as in oslam_cloud_normals:
 *      f_a = (p_a - p0_a) * scale in float32 with the winner's point p0 and scale = 16.0f / dist_tol (float32, made once by
 *      the host); a pixel with some fabsf(f_a) > 131072 (2^17) is left out of the fit, and of the fit only: it was counted
 *      and it can be labelled.  Otherwise q_a = (int32) rintf(f_a) and ten int64 sums: n, Sq_a (x y z), Sqq_ab (xx xy xz yy
 *      yz zz).  No sum can overflow: |q_a| <= 2^17, so a product is at most 2^34 and a sum over w * h <= 2^28 pixels at
 *      most 2^62 < 2^63.  The covariance in double in oslam_cloud_normals' operation order (its step 3), its
 *      OSLAM_NORMALS_SWEEPS Jacobi sweeps (step 4), the normal = the column under the smallest diagonal element (lowest
 *      index on a tie) divided by its length.  Fewer than 3 pixels in the fit, or lmid <= (double)0.01f * lmax (a strip:
 *      the normals stage's line_ratio), end the search like a low count.  Centroid c_a = (double)p0_a + (Sq_a / n) /
 *      (double)scale; the normal is negated when (nx*cx + ny*cy) + nz*cz > 0, then d = -((nx*cx + ny*cy) + nz*cz); both
 *      are rounded to float32.  support = n, rms = (float)(sqrt(max(lmin, 0)) / (double)scale), candidate = the winner's
 *      index.
 *   4. Label.  Every free pixel, with or without a normal, gets label r when fabsf(((nx*px + ny*py) + nz*pz) + d) <=
 *      dist_tol with the float32 plane of step 3 and, if it has a normal n, (nx*n_x + ny*n_y) + nz*n_z >= label_min_dot.
 *      pixels counts them.  A pixel without a normal is labelled by distance alone: the frame's depth edges belong to the
 *      planes as much as their interiors.
 * Cost: two memsets, four kernels per round enqueued for every r < max_planes whatever the image holds (a `done` word in
 *   the call's device block is set where the search ends; every later kernel reads it and leaves at once), one copy back,
 *   one host wait.  launches == 4 * max_planes, plus 1 when the view's maps had to be built.
 * oslam_planes keeps the labels on the device.  oslam_planes_get copies the plane records (OSLAM_E_LIMIT and *n_out when
 *   cap is too small), oslam_planes_labels the label image [h][w] (-1 = none), oslam_planes_rounds is the test tap: the
 *   counts [max_planes][256] and moments [max_planes][10] of every round as the device left them (zero for a round that
 *   did not run; the round that ended the search by its count keeps its counts); either may be NULL.
 * oslam_view_remove_planes: a pixel is a plane pixel iff z > 0 and its label l >= 0 (with only >= 0: l == only).
 *   OSLAM_MASK_REMOVE writes plane ? 0 : z, OSLAM_MASK_KEEP plane ? z : 0 into a new view with v's camera and max_jump
 *   that the caller owns (oslam_view_destroy); every stage takes it unchanged.  valid_in counts z > 0, object_pixels the
 *   plane pixels, valid_out the valid pixels of the output.  One memset, one kernel, one copy back; launches == 1.
 * Checks, before any device call: NULL v / out / p (pp and res may be NULL), a dist_tol that is not finite and > 0 (or so
 *   small that 16 / dist_tol is no finite float), a min_normal_dot or label_min_dot outside [-1, 1], max_planes 0 or above
 *   OSLAM_PLANES_MAX, a mode other than the two, only < -1; then the handles: a planes object of another device or image
 *   size than the view, only >= n_planes: all OSLAM_E_INVALID.  OSLAM_E_DEVICE without a device.  A refused call writes
 *   nothing but *out = NULL.
 * Known limit: the normals of the reduced view are made again from the reduced image, so a kept pixel that touches a
 *   removed one loses its normal (DESIGN.md has the share on the calibration room).
 * Connected regions of what the planes leave: oslam_view_segments, below.
 * Out of scope: merging planes across frames, planes of a cloud that has no image,
 *   folding the stage into oslam_db_detect or the tracker, a "stands on the plane" constraint for hypotheses. */
#define OSLAM_PLANES_MAX 8
typedef struct oslam_planes_params {
    float dist_tol;            /* metres, > 0, default 0.02 (calibration: DESIGN.md 7za) */
    float min_normal_dot;      /* the score's and the fit's normal gate, default 0.9 */
    float label_min_dot;       /* the label's normal gate, default 0 */
    unsigned max_planes;       /* 1..OSLAM_PLANES_MAX, default 4 */
    unsigned min_pixels;       /* 0 (default) = w * h / 50 */
    int reserved[4];
} oslam_planes_params;
typedef struct oslam_plane {
    float normal[3], d;        /* n . p + d = 0, n . centroid <= 0: the normal faces the camera */
    uint32_t support;          /* the fit's n */
    uint32_t pixels;           /* labelled */
    uint32_t candidate;        /* the winner's lattice index */
    float rms;                 /* of the fit, metres */
} oslam_plane;
typedef struct oslam_planes_result {
    uint32_t n_planes, valid_in, labelled, launches;
    float ms_total;
} oslam_planes_result;
typedef struct oslam_planes oslam_planes;

int oslam_planes_params_default(oslam_planes_params *p);
int oslam_view_planes(oslam_view *v, const oslam_planes_params *pp, oslam_planes **out, oslam_planes_result *res);
int oslam_planes_get(const oslam_planes *p, oslam_plane *planes_out, size_t cap, size_t *n_out);
int oslam_planes_labels(oslam_planes *p, int32_t *labels_out);
int oslam_planes_rounds(oslam_planes *p, uint32_t *counts_out, int64_t *moments_out);
int oslam_view_remove_planes(const oslam_view *v, const oslam_planes *p, int mode, int32_t only, oslam_view **out,
                             oslam_mask_result *res);
int oslam_planes_destroy(oslam_planes *p);

/* ---- the connected regions of a view, on the device.  With the supporting planes gone, what is left of a frame is a few
 * objects and the crumbs along the planes' borders; SLAM++-style pipelines group those pixels into connected regions and
 * treat each as an object candidate.  oslam_view_segments labels the regions of a view (optionally minus the pixels of a
 * planes object) and describes the largest, oslam_view_select_segments returns the view with or without them.  The
 * restatement in numpy is tests/segments_ref.py; device and restatement agree byte for byte, and two calls give the same
 * bytes: nothing here is a float sum, every result is an integer or one float made from integers in a fixed order.
 *
 *   1. Pixels.  A pixel is in iff z > 0 and, when planes is given, its plane label is < 0.
 *   2. Edges.  Two in pixels a, b that are 4-neighbours are joined iff
 *      fabsf(za - zb) <= max_step + rel_step * fminf(za, zb), in float32 with this grouping (the build's
 *      -ffp-contract=off keeps the operations apart).  max_step 0 = the view's max_jump.  Diagonal neighbours are never
 *      joined.
 *   3. Components are the transitive closure of the edges; a component's root is its smallest linear pixel index
 *      v * w + u.  n_components counts the roots, valid_in the in pixels.
 *   4. Selection.  A component is a candidate iff pixels >= min_pixels (0 = max(1, w * h / 1000) in integer division).
 *      With more than OSLAM_SEGMENTS_CANDIDATES candidates the call returns OSLAM_E_LIMIT with *out = NULL; it sets
 *      res->n_components and res->n_candidates and writes nothing else (candidates are bounded by w * h / min_pixels, so
 *      the default can never overflow).  Candidates are ranked by pixels descending, then by root ascending; the first
 *      max_segments ranks become segments 0 .., every other in pixel gets label -1.  labelled = the sum of the segments'
 *      pixels.
 *   5. Records.  pixels, root, the bounding box (inclusive) and sides, derived from the box against the image borders.
 *      The centroid comes from three int64 sums of q_a = (int32) rintf(p_a * 8192.0f) over the segment's pixels, p =
 *      ((((float)u - cx) * z) / fx, (((float)v - cy) * z) / fy, z); a pixel with some fabsf(p_a * 8192.0f) > 2^30 is left
 *      out of the centroid, and of the centroid only.  No sum can overflow: |q_a| <= 2^30 and w * h <= 2^28 pixels give at
 *      most 2^58 < 2^63.  centroid_a = (float)(((double)S_a / (double)n) / 8192.0) with n the pixels that entered the
 *      sums, 0 when n is 0.  (The bound is 131072 m from the optical axis: no sane camera reaches it; the tests do with
 *      a focal length of a thousandth of a pixel.)
 * Cost: two memsets, OSLAM_SEGMENTS_LAUNCHES (6) kernels whatever the image holds, one copy back, one host wait, no host
 *   round trip inside the call; launches == 6.  The view's maps are not needed.
 * oslam_segments keeps the root and label images on the device.  oslam_segments_get copies the records (OSLAM_E_LIMIT
 *   and *n_out when cap is too small), oslam_segments_labels the label image [h][w] (the segment's rank or -1),
 *   oslam_segments_roots is the test tap: [h][w], the component's root or -1 for a pixel that is not in.
 * oslam_view_select_segments is oslam_view_remove_planes' contract with the segment pixels (label >= 0; with only >= 0:
 *   label == only) as the object pixels: OSLAM_MASK_REMOVE or OSLAM_MASK_KEEP, a genuine view with v's camera and max_jump
 *   that the caller owns, the same three counters, one kernel (k_planes_mask on the label image); launches == 1.
 * Checks, before any device call: NULL v / out / s (planes, sp and res may be NULL), a max_step or rel_step that is not
 *   finite or is < 0, max_segments 0 or above OSLAM_SEGMENTS_MAX, a mode other than the two, only < -1; then the handles:
 *   max_step 0 on a view whose max_jump is 0, planes or segments of another device or image size than the view,
 *   only >= n_segments: all OSLAM_E_INVALID.  OSLAM_E_DEVICE without a device.  A refused call writes nothing but
 *   *out = NULL.
 * Out of scope: 8-connectivity, a normal term in the gate, merging segments across frames, segments of a cloud that has
 *   no image, folding the stage into oslam_db_detect or the tracker's births. */
#define OSLAM_SEGMENTS_MAX        64      /* records kept */
#define OSLAM_SEGMENTS_CANDIDATES 4096    /* components that may pass min_pixels in one call */
#define OSLAM_SEGMENTS_LAUNCHES   6
typedef struct oslam_segments_params {
    float max_step;            /* metres; 0 (default) = the view's max_jump */
    float rel_step;            /* per metre of depth, >= 0, default 0 */
    unsigned min_pixels;       /* 0 (default) = max(1, w * h / 1000) in integer division */
    unsigned max_segments;     /* 1..OSLAM_SEGMENTS_MAX, default 16 */
    int reserved[4];
} oslam_segments_params;
typedef struct oslam_segment {
    uint32_t pixels;           /* of the component */
    uint32_t root;             /* its smallest linear pixel index v * w + u */
    uint16_t u0, v0, u1, v1;   /* bounding box, inclusive */
    float centroid[3];         /* camera frame, metres */
    uint32_t sides;            /* bit 0..3: touches the left, top, right, bottom image border */
} oslam_segment;
typedef struct oslam_segments_result {
    uint32_t n_segments, n_components, n_candidates, valid_in, labelled, launches;
    float ms_total;
} oslam_segments_result;
typedef struct oslam_segments oslam_segments;

int oslam_segments_params_default(oslam_segments_params *p);
int oslam_view_segments(const oslam_view *v, const oslam_planes *planes, const oslam_segments_params *sp, oslam_segments **out,
                        oslam_segments_result *res);
int oslam_segments_get(const oslam_segments *s, oslam_segment *out, size_t cap, size_t *n_out);
int oslam_segments_labels(oslam_segments *s, int32_t *labels_out);
int oslam_segments_roots(oslam_segments *s, int32_t *roots_out);
int oslam_view_select_segments(const oslam_view *v, const oslam_segments *s, int mode, int32_t only, oslam_view **out,
                               oslam_mask_result *res);
int oslam_segments_destroy(oslam_segments *s);

/* ---- colour next to the TSDF (KinFu's colour volume): a view can carry the colour image its sensor registered with the
 * depth image, a volume a colour per voxel, and the fused colour comes back at the points of the surface and the mesh and
 * as the picture of a view.  No stage that existed before reads colour: a view or a volume without it behaves bit for
 * bit as before.  The restatement in numpy is tests/colour_ref.py; device and restatement agree bit for bit.
 * A colour image on a view: rgb is [h] rows of w times 3 bytes R G B, row_stride_bytes apart (0 = 3 * w), registered
 *   with the depth image (same camera, same size); valid is [h][w], 0 = the pixel has no colour, or NULL when every
 *   pixel has one.  On the device a pixel is one word r | g << 8 | b << 16 | a << 24, a = 255 with colour, the whole
 *   word 0 without.  A second call replaces the image, oslam_view_destroy frees it.  Views made by oslam_view_bilateral,
 *   oslam_view_mask, oslam_pyramid_create and oslam_volume_raycast start without colour.  oslam_view_colour is the tap:
 *   [h][w] words, OSLAM_E_INVALID on a view without colour.
 * A colour buffer on a volume: oslam_volume_colour_enable allocates a second buffer of nx * ny * nz words, all zero
 *   (computed in size_t; OSLAM_E_NOMEM changes nothing; enabling twice is OSLAM_E_INVALID).  A voxel's word is
 *   r | g << 8 | b << 16 | wc << 24, wc = 0 reads as never coloured.  oslam_volume_reset zeroes the colours,
 *   oslam_volume_set_voxels does not touch them, oslam_volume_destroy frees them.  oslam_volume_colour_words and
 *   oslam_volume_set_colour_words are the taps, [nz][ny][nx].
 * oslam_volume_integrate_colour is oslam_volume_integrate(vol, v, T_vol_cam) followed by the colour pass in the same
 *   call (one more launch, res->launches = 2; the TSDF words are those of the plain call bit for bit).  c is the view that
 *   carries the colour: it must have colour, and its size and fx, fy, cx, cy must have the float bits of v's (c == v is
 *   the ordinary case; a masked or filtered v takes its colour from the raw view).  For voxel (i, j, k): the centre, p',
 *   the pixel and z_o are oslam_volume_integrate's; the voxel is skipped unless p'z > 0, the pixel lies inside the image,
 *   z_o > 0, sdf = z_o - p'z satisfies -band <= sdf <= band, and the pixel's a != 0.  Update in uint32 arithmetic per
 *   channel: ch' = (ch * wc + pix + ((wc + 1) >> 1)) / (wc + 1), wc' = min(wc + 1, max_weight).  A skipped voxel is
 *   neither read nor written; a voxel belongs to one thread; two calls give the same bits.  *coloured_out (may be NULL) =
 *   the voxels updated.
 * The colour at a volume-frame point P: c_a, b_a, f_a of the ray cast's trilinear read above; when all of
 *   0 <= b_a <= n_a - 2 and all 8 corners have wc > 0, per channel the corner bytes as float, lerp(p, q, f) =
 *   p * (1.0f - f) + q * f along x, then y, then z, floorf(value + 0.5f), clipped to 0..255.  Otherwise the voxel that
 *   holds P, floorf((P_a - origin_a) * inv_voxel) per axis, range-checked in float, gives its colour when wc > 0.
 *   Otherwise there is no colour: valid 0 and rgb 0.  A NaN or infinite coordinate has no colour and reads nothing.
 * oslam_volume_colours: xyz = n points stride_bytes apart (0 = 12; a multiple of 4, at least 12), rgb_out [n][3],
 *   valid_out [n], *n_valid_out (may be NULL) = the points with a colour; n == 0 is allowed.  It serves the points of
 *   oslam_volume_surface, oslam_volume_mesh and oslam_volume_leaving; they go up from the host.
 * oslam_volume_paint_view: for every pixel of v with z > 0 the vertex (dx * z, dy * z, z) with the ray cast's dx, dy,
 *   P_x = ((M0*vx + M1*vy) + M2*vz) + M3 (y, z alike) with M = T_vol_cam, and the colour at P into v's colour image
 *   (created when v has none; a = 255 or the word 0).  On a ray-cast view this is the map's picture from that pose.
 *   *painted_out (may be NULL) = the pixels that got a colour.
 * The moving window: oslam_volume_shift moves the colours with the TSDF words (the same kernel on the colour buffer into
 *   a second spare buffer: oslam_shift_result.launches is 2 on a coloured volume; when a spare cannot be allocated
 *   neither buffer moves).  oslam_volume_shift_world shifts the colours the same way (one launch more).  Through a
 *   plain store voxels that leave lose their colour, and voxels that are reloaded come back with wc = 0 until they are
 *   seen again; a colour store (oslam_world_params.colour) keeps the colour word of every voxel it keeps and gives it
 *   back (above, at oslam_volume_shift_world, "Colour").
 * The PLY writers with colour write the vertex element of oslam_ply_write / oslam_ply_write_mesh plus property uchar
 *   red, green, blue; oslam_ply_read and oslam_ply_read_mesh skip them.
 * Arguments are checked before any device call: NULL pointers, a pose that is not rigid, parameters outside their
 *   ranges, views and volumes on different devices, a c without colour or with another size or other intrinsics, and a
 *   volume without colour where one is needed are OSLAM_E_INVALID, with nothing changed.
 * The colour of the whole map.  oslam_world_colours(w, vol, sp, xyz, n, stride_bytes, rgb_out, valid_out, n_valid_out) is
 *   oslam_volume_colours against colour store plus window, with its arguments and outputs; it serves the points of
 *   oslam_world_surface and the vertices of oslam_world_mesh, which go up from the host as they do for the volume.  The
 *   restatement in numpy is tests/world_colour_ref.py; device and restatement agree byte for byte.
 *   The map.  Gc(g) is the volume's colour word inside the window's box and the store's colour word elsewhere, or 0:
 *   oslam_world_surface's G with "a store entry inside the window's box is ignored".  With vol == NULL the store stands
 *   alone.  The frame.  sp (NULL = defaults) gives the anchor A and with it O = origin(A), oslam_world_surface's word for
 *   word; sp->dev picks the device when vol is NULL; min_weight is checked and not used.  Points are to be coloured with
 *   the anchor they were extracted with.
 *   The rule is the colour at a volume-frame point above, float sequence unchanged: u = (P - O) * inv_voxel, g = u - 0.5f,
 *   b = floorf(g), f = g - b; the range test on b becomes "finite and |b| < 2^22"; the eight corners are Gc at A + b +
 *   (0|1); with all eight wc > 0 the channels are blended, rounded and clipped as there.  Otherwise the voxel A +
 *   floorf(u), under the same range test, gives its colour if its wc > 0; it is looked up on its own, not taken from the
 *   corners.  Otherwise there is no colour: valid 0 and rgb 0.  A NaN or infinite coordinate reads nothing.
 *   Two pins.  (a) A dense coloured oslam_volume with the same voxel and created origin, at offset A, that holds G and Gc
 *   over a box that contains every coloured voxel of the map gives the same bytes through oslam_volume_colours at every
 *   point; no margin is needed, because outside the box both read "uncoloured".  (b) With the default anchor a point whose
 *   eight corners and nearest voxel all lie inside the window gets the bytes oslam_volume_colours(vol) gives it.
 *   Device side.  The ascending key table of oslam_world_surface with the brick array holding colour words: the store's
 *   colour bricks go up through the pinned buffer, window-only bricks are zeroed, k_brick_window writes the volume's
 *   colour buffer over the window's box.  k_brick_colours runs one thread per point: one binary search finds the base
 *   corner's brick and the eight words come from it when the stencil does not cross a brick face (all three local
 *   coordinates <= 6), otherwise each corner is searched for; no LDS, no scratch, one integer atomic per wave for the
 *   count.  2 launches with a volume, 1 without; one host wait.
 *   Refusals, all before any device call, OSLAM_E_INVALID with nothing written: NULL w, a NULL output with n > 0, a bad
 *   stride or n >= 2^31 (oslam_volume_colours' rules), an anchor beyond 2^20 or min_weight outside 1..65535, a store without
 *   colour, a volume without colour, a volume whose voxel or created-origin bits are not the store's.  A map of more than
 *   2^22 bricks is OSLAM_E_LIMIT.  n == 0 and an empty map return zeros without a device call.  Nothing changes in store
 *   or volume; the locks are taken in the usual order (volume, then store); device memory is freed on every path.
 * Out of scope: colours written inside the extraction kernels so that points never go up again, colour through bilateral,
 *   mask and pyramid views, a colour term in tracking,
 *   verification or arbitration, keeping surface points in HBM between the extraction and oslam_volume_colours, several
 *   GPUs. */
typedef struct oslam_colour_params {
    unsigned max_weight;      /* 1..255, default 8.  The mean is kept in 8 bits: at weight wc a pixel moves it only when it
                                 differs by (wc + 1) / 2 levels or more, so a large weight freezes the colour */
    float band;               /* metres; a voxel is coloured when |sdf| <= band.  0 (the default) = the volume's mu,
                                 otherwise 0 < band <= mu */
    int reserved[6];
} oslam_colour_params;

int oslam_view_set_colour(oslam_view *v, const uint8_t *rgb, size_t row_stride_bytes, const uint8_t *valid);
int oslam_view_colour(oslam_view *v, uint32_t *rgba_out);
int oslam_view_has_colour(const oslam_view *v);
int oslam_colour_params_default(oslam_colour_params *p);
/* cp may be NULL (defaults) */
int oslam_volume_colour_enable(oslam_volume *vol, const oslam_colour_params *cp);
int oslam_volume_colour_words(oslam_volume *vol, uint32_t *words_out);
int oslam_volume_set_colour_words(oslam_volume *vol, const uint32_t *words);
int oslam_volume_integrate_colour(oslam_volume *vol, const oslam_view *v, const oslam_view *c, const float T_vol_cam[16],
                                  oslam_integrate_result *res, uint32_t *coloured_out);
int oslam_volume_colours(oslam_volume *vol, const float *xyz, size_t n, size_t stride_bytes, uint8_t *rgb_out,
                         uint8_t *valid_out, size_t *n_valid_out);
int oslam_volume_paint_view(oslam_volume *vol, const float T_vol_cam[16], oslam_view *v, uint32_t *painted_out);
int oslam_ply_write_colour(const char *path, const float *xyz, const float *nrm, const uint8_t *rgb, size_t n, int binary);
int oslam_ply_write_mesh_colour(const char *path, const float *xyz, const float *nrm, const uint8_t *rgb, size_t nv,
                                const uint32_t *tri, size_t nt, int binary);
int oslam_world_colours(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, const float *xyz, size_t n,
                        size_t stride_bytes, uint8_t *rgb_out, uint8_t *valid_out, size_t *n_valid_out);
/* oslam_volume_paint_view against the whole map: the colour of oslam_world_colours at the volume-frame point of every
 * pixel of v with z > 0, seen from T_vol_cam, into the view's colour image (the word 0 elsewhere); *painted_out = the
 * pixels with a colour.  The vertex, its transform and the image word are oslam_volume_paint_view's, the read is
 * oslam_world_colours' (k_brick_colour_view next to k_brick_colours, the same function for the colour at a point).  sp
 * gives the anchor; a map without a volume goes to the view's device (sp->dev is not read).  Refusals are
 * oslam_world_colours' together with oslam_volume_paint_view's (NULL w, T_vol_cam or v, a pose that is not rigid, volume
 * and view on different devices), before any device call.  An empty map paints zeros without a launch */
int oslam_world_paint_view(oslam_world *w, oslam_volume *vol, const oslam_world_surface_params *sp, const float T_vol_cam[16],
                           oslam_view *v, uint32_t *painted_out);

/* ---- parity taps (tests): values the reference materialises as arrays.
 * Scene::getHashKeys row r (scene.cu:49-54): keys_out[n] of reference point r,
 * computed by the GPU key kernel with this d_dist (key 0 on the diagonal). */
int oslam_scene_keys(oslam_scene *s, size_t ref_index, uint32_t *keys_out);
int oslam_model_keys(oslam_model *m, size_t ref_index, uint32_t *keys_out);
/* ParallelHashArray lookup (include/impl/parallel_hash_array.hpp:80-92):
 * flat pair indices m_r*M + m_i stored under `key`, ascending; returns the
 * bucket size in *count_out and copies at most cap indices. */
int oslam_model_bucket(oslam_model *m, uint32_t key, uint32_t *pairs_out, size_t cap,
                       size_t *count_out);
/* The stored words theta_u << 11 | half << 10 | row of one key's bucket in one table slice (slices hold 2 x 1023
 * model reference points: m_r - 2046*slice = 1023*half + row), in storage order (what a vote wave streams, 4
 * consecutive words per lane). */
int oslam_model_bucket_words(oslam_model *m, uint32_t key, int slice, uint32_t *words_out, size_t cap,
                             size_t *count_out);
/* The numbering of the model's key table (its group's, while it is in a database): key, number and weight of every
 * key, in ascending key order; at most cap of each are copied, *n_out = the number of keys.  The weight is the number
 * of entries in the key's buckets, over every slice and every model that shares the numbering. */
int oslam_model_key_numbers(oslam_model *m, uint32_t *keys_out, uint32_t *numbers_out, uint64_t *weights_out, size_t cap,
                            size_t *n_out);
/* The order in which the vote grid takes a batch of n reference points with the demands keep[n] (host only):
 * order_out[p] = the reference point of dispatch position p. */
int oslam_vote_ref_order(const uint32_t *keep, size_t n, uint32_t *order_out);
/* Dense accumulator acc[M][32] of scene reference point ref_index after voting. */
int oslam_vote_accumulator(oslam_model *m, oslam_scene *s, size_t ref_index, uint32_t *acc_out);
/* The hit list of scene reference point ref_index as the votes read it, sorted by key number (a list above one segment
 * of the sort -- 16384 hits, 8192 from 2^18 key numbers on -- segment by segment): per hit the number of
 * its key (oslam_model_key_numbers), theta_v in units of 2^-22 turn (0xffffffff: always re-evaluated) and the scene
 * index of the pair's second point; at most cap of each are copied (any may be NULL), *n_out = the number of hits.
 * *keep_out (may be NULL) = the pairs of the reference point whose distance bin can reach a model key: the places
 * its list was given. */
int oslam_vote_hits(oslam_model *m, oslam_scene *s, size_t ref_index, uint32_t *numbers_out, uint32_t *theta_out,
                    uint32_t *idx_out, size_t cap, size_t *n_out, uint32_t *keep_out);
/* The hit sort alone (k_sort_hits), on n_lists hit lists the caller supplies, in one launch.  List l owns the slots
 * offsets[l] .. offsets[l + 1] of every per-hit array and holds min(counts[l], its slots) hits in arrival order: the
 * number of the hit's key (below 2^id_bits), theta_v and the scene index.  Every array comes back whole: numbers_out =
 * the key numbers in sorted order | (the hit's run holds a marker) << 31, and the input past the hits; theta_out /
 * idx_out = the payloads in sorted order; runs_out[r] = {number | (hits - 1) << 26, first hit | marker << 31} for the
 * run_counts_out[l] runs of list l, from its first slot on.  theta_out, idx_out, runs_out and run_counts_out are filled
 * with 0xA5 bytes before the launch: the words the kernel does not own keep them.  The contract is DESIGN.md's at the
 * hit sort; tests/sort_ref.py restates it.  OSLAM_E_INVALID before any device call: a NULL array, offsets that
 * descend, id_bits outside 1 .. 26, a number at or above 2^id_bits. */
int oslam_sort_hits_tap(const uint32_t *numbers, const uint32_t *theta, const uint32_t *idx, const uint32_t *offsets,
                        const uint32_t *counts, size_t n_lists, uint32_t id_bits, int dev, uint32_t *numbers_out,
                        uint32_t *theta_out, uint32_t *idx_out, uint32_t *runs_out, uint32_t *run_counts_out);
/* The two ordering kernels of the model build alone (k_bucket_spread, k_bucket_psort), on n_buckets buckets the caller
 * supplies, in one launch each.  Bucket b holds lens[b] entries and starts at the running sum of (len + 3) & ~3 over
 * the buckets before it, as the build's scan places it; its slot carries the key keys[b] (keys NULL: b + 1; a slot
 * with key 0 is skipped by both kernels, whatever its length).  e4 / uv (two floats per entry) / mi hold the entries in
 * arrival order with the padding words behind every bucket, `total` = the end of the last bucket of each; they go up as
 * given.  spread 0 leaves k_bucket_spread out (oslam_params.no_bucket_spread), with_uv 0 is the fast-mode build: the
 * kernels get no uv (uv_out = uv as given) and k_bucket_psort is not launched.  Every array comes back whole: e4_out / uv_out / mi_out [total]
 * in the spread's order, pw_out / puv_out [total] the second order and pdir_out [total + 256] its directories; the last
 * three are filled with 0xA5 bytes before the launches and the places the kernels do not own keep them.  The contract
 * is oslamk_entries' (DESIGN.md at the model build); tests/bucket_ref.py restates it.  OSLAM_E_INVALID before any
 * device call: a NULL array (but keys), a bucket above 2^20 entries, a total above 2^24. */
int oslam_bucket_order_tap(const uint32_t *lens, const uint32_t *keys, size_t n_buckets, const uint32_t *e4, const float *uv,
                           const uint16_t *mi, int with_uv, int spread, int dev, uint32_t *e4_out, float *uv_out,
                           uint16_t *mi_out, uint32_t *pw_out, float *puv_out, uint16_t *pdir_out);
/* A built model's tables as they lie in device memory, copied back without sorting or interpreting: the same for a
 * created model, a loaded one and a member of a database group (which shows its group's union tables: ukeys, uids,
 * weights, reach, kmap, and its own slots, uinfo and entries).  Size, then fill: *info always receives the scalars, which
 * give every array's length; each array whose pointer is not NULL is then copied whole:
 *   slots [n_slices * cap][4] (key, start, len, cur)   ukeys, uids [ucap]   weights [ucap] (64-bit)   reach [512]
 *   kmap [kmap_bins * 4913]   uinfo [n_slices * uinfo_stride][2] (start, len | marker << 31)
 *   e4 [n_entries + 256]   mi [n_entries]   pw [n_entries]   puv [n_entries][2]   pdir [n_entries + 256]
 * pw, puv and pdir exist only when info->has_pw (not in a fast-mode model: asking for them there is OSLAM_E_INVALID);
 * the places of pw, puv and pdir the build does not own are whatever the allocation held.  The layout is
 * csrc/oslam_kernels.h's (DESIGN.md at the model build); tests/model_ref.py restates what is determined of it. */
typedef struct oslam_model_tables {
    uint32_t cap, shift, n_slices, ucap, ushift, n_entries, n_ids, id_bits, uinfo_stride, kmap_bins, reach_words, has_pw;
    uint64_t num_model_keys;
    uint32_t reserved[2];
} oslam_model_tables;
int oslam_model_tables_tap(oslam_model *m, oslam_model_tables *info, uint32_t *slots, uint32_t *ukeys, uint32_t *uids,
                           uint64_t *weights, uint32_t *reach, uint32_t *kmap, uint32_t *uinfo, uint32_t *e4, uint16_t *mi,
                           uint32_t *pw, float *puv, uint16_t *pdir);
/* Cells kept by the last oslam_align / oslam_align_finish on this model, in
 * the order (count desc, code asc); poses_out (may be NULL) gets 16 floats per cell. */
int oslam_last_cells(oslam_model *m, oslam_cell *cells_out, float *poses_out, size_t cap,
                     size_t *n_out);
/* The clustering scores of a NAMED pose tail over the n peak records `cells` (as oslam_align_finish takes them, with
 * the global maximum): path 0 = the host loop, 1 = the host tail with the scores from the device kernel at any number
 * of poses (production asks the kernel from 2048 poses on), 2 = the device tail at any number (production: from
 * oslam_params.pose_gpu_min records on; it needs two kept cells, else OSLAM_E_NO_VOTES).  The scores oslam_last_result
 * returns are always recomputed by the host loop; these are the ones the tail itself made.  cells_out / scores_out (may
 * be NULL) receive at most cap kept cells in (count desc, code asc) order and the score of each; *n_out = the number
 * kept, *max_idx_out the winner's index, T its matrix, *path_out the tail that really made the scores (a device tail
 * that fell back to the host loop reports 0).  The model's last result is dropped by path 2. */
int oslam_tail_scores(oslam_model *m, oslam_scene *s, const oslam_cell *cells, size_t n, uint32_t global_max, int path,
                      oslam_cell *cells_out, float *scores_out, size_t cap, size_t *n_out, uint32_t *max_idx_out,
                      float T[16], int *path_out);

/* Launch stream for all kernels of this thread's calls (hipStream_t as void*;
 * NULL = the default stream).  bench.py passes torch's current stream. */
int oslam_set_stream(void *hip_stream);
/* Calls that launch on one device are serialised inside the library (one lock per device: they share
 * the device's hit-list pool, which grows to what a registration needs, at most oslam_params.scratch_gib GiB,
 * default 4, unless a single reference point needs more).  oslam_release_scratch frees the pool and the
 * other per-device work space; the next call allocates them again. */
int oslam_release_scratch(int dev);
const char *oslam_last_error(void);
/* Threads of the host stage (poses and clustering of the gathered peaks); 0 = OpenMP's default,
 * capped at 16.  Launchers that export OMP_NUM_THREADS=1 per rank can raise it here. */
int oslam_set_host_threads(int n);
/* Self-test of the device float path against the host: evaluates pm_acosf /
 * pm_atan2f / key arithmetic on `n` pseudo-random inputs on both sides and
 * returns the number of mismatching results in *mismatches. */
int oslam_selftest_math(size_t n, uint64_t seed, uint64_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif /* OSLAM_H */
