/*
 * oslam_internal.h -- the handles behind include/oslam.h, shared by the translation units of
 * liboslam_hip.so that read them (oslam_host.c, oslam_refine.c).  Not installed.
 */
#ifndef OSLAM_INTERNAL_H
#define OSLAM_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "oslam.h"
#include "oslam_kernels.h"

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
};

struct oslam_scene {
    int dev;
    cloud_buf c;
    float d_dist;
    unsigned df;
    int rank, world;
    int n_ref;
    uint32_t *h_ref_idx, *d_ref_idx;
    float *d_tsg;
    float *d_Ts16;                    /* frames of every reference-point candidate (index % df == 0, all ranks) */
    struct oslam_scene_grid *grids;   /* uniform grids of the refinement stage (oslam_refine.c), NULL until the first */
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

/* records `what` for oslam_last_error and returns code */
int oslam_fail(int code, const char *what);
/* the launch stream of this thread's calls (oslam_set_stream) */
void *oslam_stream(void);
/* gives back the scene's refinement grids (oslam_refine.c); called by oslam_scene_destroy */
void oslam_refine_release_grids(oslam_scene *s);

#endif /* OSLAM_INTERNAL_H */
