/*
 * oslam_pose.h -- host-side tail of the path: accumulator peaks -> poses ->
 * clustering -> best pose.  The north-star keeps this stage on the host, after
 * the all-gather of per-GPU peaks; it touches a few thousand records.
 * Internal to liboslam_hip.so (the exported wrappers are in include/oslam.h).
 */
#ifndef OSLAM_POSE_H
#define OSLAM_POSE_H

#include <stddef.h>
#include <stdint.h>

#include "oslam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows y and z of T_g (8 floats) for n reference points: what the kernels need */
void oslam_T_g_rows(const float *xyz, const float *nrm, const uint32_t *idx, size_t n,
                    float *rows_out);

/* the whole frame T_g (16 floats, row-major) of the points idx0, idx0 + step, ... (n of them) */
void oslam_T_g_full(const float *xyz, const float *nrm, size_t idx0, size_t step, size_t n, float *out16);

/* cos, sin of alpha_idx * D - pi for alpha_idx = 0..63 (libm): the kernels' rotation table */
void oslam_rotx_table(float cs[128]);

/* Optional accelerator for the clustering scores (set by oslam_align.c while a device is bound):
 * fills score[n] exactly as the host loop would, returns 0 on success.  hash_idx = n pairs
 * {cell hash, pose index} ascending. */
typedef int (*oslam_cluster_hook)(size_t n, const float *trans, const float *quat, const float *wv,
                                  const int32_t *cell, const uint32_t *hash_idx, float d_dist, int use_l1,
                                  float *score);
void oslam_pose_set_cluster_hook(oslam_cluster_hook hook);
/* Both per thread, like the hook.  The hook is asked from n poses on: 0 = the default (2048), which production never
 * changes; oslam_tail_scores lowers it so that small made-up pose sets reach the kernel.  _used: did the last clustering
 * stage of this thread take its scores from the hook (1) or from the host loop (0)? */
void oslam_pose_set_cluster_hook_min(size_t n);
int oslam_pose_cluster_hook_used(void);

/* instance candidates (include/oslam.h at oslam_align_instances), in candidate order: T [n][16], score [n], index [n]
 * (kept-cell index, or the head of a greedy cluster) */
typedef struct oslam_pose_cands {
    size_t n;
    float *T, *score;
    uint32_t *index;
} oslam_pose_cands;
/* oslam_pose_stage with the candidates of every pose (allocated here; oslam_pose_cands_free) */
int oslam_pose_stage_cands(const oslam_cell *cells, size_t n, const float *m_xyz, const float *m_nrm,
                           size_t M, const float *s_xyz, const float *s_nrm, size_t S, float d_dist,
                           int cpu_clustering, int use_l1_norm, int use_averaged_clusters,
                           const float *weights, float T_out[16], float *poses_out, oslam_pose_cands *cands);
void oslam_pose_cands_free(oslam_pose_cands *c);
/* the pieces of the selection rule, shared with the device launcher's argument set-up */
int oslam_instance_params_check(const oslam_instance_params *ip, size_t cap);
void oslam_instance_thresholds(const oslam_instance_params *ip, float extent, float *sep2, float *cos_thr, int *rot_on);
void oslam_instance_centroid(const float T[16], const float c[3], float p[3]);
int oslam_same_instance(const float pa[3], const float *A, const float pb[3], const float *B, float sep2, float cos_thr,
                        int rot_on);

#ifdef __cplusplus
}
#endif
#endif
