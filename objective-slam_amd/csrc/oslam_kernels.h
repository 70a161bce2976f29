/*
 * oslam_kernels.h -- C launch interface of the gfx950 (MI355X / CDNA4) kernels, one .hip file per stage beside this
 * header.  Internal to liboslam_hip.so; the public boundary is include/oslam.h.  All pointers are device pointers
 * unless noted; `stream` is a hipStream_t passed as void*.  Launchers return a hipError_t as int.
 *
 * The PPF registration path.  What the reference does with N^2-sized arrays and Thrust sorts
 * (pcl/alignment/src/cuda/{scene,model}.cu) is fused; wave = 64 lanes throughout:
 *   model build  (oslam_model.hip) pair key -> per-slice open-addressing table -> bucketed 4-byte pair entries (two
 *                counting passes, no sort); union table of all keys, and per slice the bucket of every key; bitset of
 *                the distance bins that can reach a key; key map (distance bin, three angle bins) -> key number;
 *                entries ordered inside each bucket for the LDS banks;
 *   scene count  (oslam_scene.hip) per reference point, the pairs whose distance bin can reach a model key: sizes the
 *                hit lists by demand;
 *   scene keys   (oslam_scene.hip) per (8 reference points, tile of scene points): distance bin of every pair,
 *                unreachable bins dropped, the rest compacted in LDS; the pair's feature as bins -> key map (one load,
 *                no hash, no probing) -> per-reference hit list {key number} + {theta_v, i} written by
 *                wave-aggregated appends;
 *   hit sort     (oslam_sort.hip) per reference point, hits ordered by key number (LDS radix sort) and the list of
 *                runs of equal keys;
 *   voting       (oslam_vote.hip, oslam_vote_wide.hip; the workgroup: oslam_vote_body.inc) one workgroup per (scene
 *                reference point, model slice of 2046 points): a run finds its bucket with one load (no probing); very
 *                long items are cut into units dealt to the 16 waves, the rest is handed out dynamically a few runs at
 *                a time; a wave streams a bucket once for all hits that share it (16 bytes = 4 entries per lane, four
 *                steps' loads in flight) -> integer alpha bin -> LDS accumulator [1023 rows + sink][31 words], two
 *                16-bit counters per word; votes near a bin edge are cast, noted and re-checked with the reference's
 *                float sequence; in-kernel peak extraction;
 *   pose tail    (oslam_posegpu.hip) poses of the peaks and their clustering scores (one wave per four poses).
 * The stages after registration (refinement, verification, ..., the whole map) have a .hip each whose head says what
 * its kernels do.
 */
#ifndef OSLAM_KERNELS_H
#define OSLAM_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSLAMK_SLICE 2046      /* model reference points per table slice: two per 32-bit counter word of a row (ppf_core.h) */
#define OSLAMK_ROWS 1024       /* rows of the LDS accumulator: one per reference point of the slice + the sink row of padding entries */
#define OSLAMK_NBIN 32         /* alpha bins per accumulator row (reference uses 0..30) */
/* The accumulator of a vote workgroup in LDS: OSLAMK_ROWS rows of ACC_STRIDE words (bins 0..29 + one unused).
 * The stride is odd on purpose: the LDS bank of a vote is (row * 31 + bin) mod 32 = (bin - row) mod 32, so votes
 * of one instruction that fall into the same bin of different rows do not meet on a bank, and k_bucket_spread
 * can order a bucket so that the 32 lanes the LDS serves together land on 32 different banks whatever the
 * hit's angle is (a stride of 32 would make the bank the bin alone: 30 banks, and as crowded as the model's
 * angles are). */
#ifndef ACC_STRIDE
#define ACC_STRIDE 31
#endif

/* One slot of a slice's open-addressing table, keyed by the 32-bit PPF key. */
typedef struct oslamk_slot {
    uint32_t key;              /* 0 = empty (key 0 is never stored: kernel.cu:491) */
    uint32_t start;            /* first entry of the bucket in the entry arrays */
    uint32_t len;              /* bucket length */
    uint32_t cur;              /* fill cursor (== len after the build) */
} oslamk_slot;

/* Model pair entries, bucketed by (slice, key); every bucket starts on a multiple of 4
 * entries so that a lane can fetch 4 of them with one 16-byte load.
 *   e4[e] = theta_u << 11 | half << 10 | row   the 4 bytes a vote streams (pc_entry_word; theta_u =
 *           pc_angle_t22 of (T_m_g * m_i).y/.z, kernel.cu:330-332, in units of 2^-21 turn; half, row =
 *           pc_row11(m_r - slice*OSLAMK_SLICE)); the up to 3 padding words behind a bucket hold row
 *           1023, the accumulator's sink row
 *   uv[e] = (T_m_g * m_i).y/.z as floats: read only by the rare votes that are
 *           re-evaluated with the reference's own arithmetic (exact mode)
 *   mi[e] = m_i (parity tap only) */
typedef struct oslamk_uv {
    float uy, uz;
} oslamk_uv;

typedef struct oslamk_entries {
    uint32_t *e4;
    oslamk_uv *uv;             /* build time only (bucket order of e4); NULL afterwards and in fast mode */
    uint16_t *mi;
    /* exact mode: every bucket a second time, ordered by the position its entries' votes take inside a bin --
     * P(word) = (word * 30) mod 2^32 -- in segments of OSLAMK_PSEG entries: pw = the words, puv = their uv.  A
     * hit's votes that fall within the margin of a bin edge are the entries with (P(base) - P(word)) mod 2^32
     * below PC_T24_EDGE: a contiguous piece of this order, found by a binary search per (hit, bucket) instead of
     * a test per vote; only those (one vote in 4000) are re-evaluated with the reference's float sequence. */
    uint32_t *pw;
    oslamk_uv *puv;
    /* directory of that order: a segment of n entries at bucket offset b is cut into K = OSLAMK_PDIR_CELLS(n) cells of
     * equal width in P (one or two entries each on average); pdir[(b << OSLAMK_PDIR_SHIFT) + k], k = 0 .. K, is the position inside the
     * segment of the first entry whose cell is >= k (pdir[b + K] = n).  The search for a hit's near-edge entries is two
     * 2-byte loads and the one or two cells between them, not a binary search. */
    uint16_t *pdir;
    uint32_t n_real;           /* entries the arrays hold (the end of the last bucket, padding included): what the near-edge
                                * search checks its indices against before it loads */
} oslamk_entries;
#define OSLAMK_PSEG 4096       /* entries per sorted segment of a bucket (one LDS sort) */
/* cells of a segment of n entries: the largest power of two below the n << OSLAMK_PDIR_SHIFT directory places the
 * segment owns (so that K + 1 places fit; a bucket is padded to a multiple of 4 entries, so a segment of one still has
 * two), at most 4096: a cell must not be narrower than the margin window (2^32 / 4096 > PC_T24_EDGE) */
#ifndef OSLAMK_PDIR_SHIFT
#define OSLAMK_PDIR_SHIFT 0
#endif
#define OSLAMK_PDIR_CELLS_RAW(m) ((m) <= 1u ? 1u : 1u << (31 - __builtin_clz((m) - 1u)))
#define OSLAMK_PDIR_CELLS(n) (OSLAMK_PDIR_CELLS_RAW((n) << OSLAMK_PDIR_SHIFT) > 4096u ? 4096u : OSLAMK_PDIR_CELLS_RAW((n) << OSLAMK_PDIR_SHIFT))

typedef struct oslamk_cloud {
    const float *px, *py, *pz, *nx, *ny, *nz;
    int n;
} oslamk_cloud;

/* A scene's points a second time, in an order that keeps neighbours together (Morton order of the positions: oslam_scene.c), for
 * phase 1 of the scene-key kernels alone: 64 consecutive points of it are one group with a bounding box, and a
 * (reference point, group) whose box cannot hold a pair within reach is dropped with one test instead of 64.
 *   sx sy sz : the positions in that order (the same floats as scene.px py pz)
 *   perm     : perm[k] = the scene's own index of the point at place k
 *   box      : [ceil(n / 64)][6] min x y z, max x y z of each group; all NaN for a group that holds a coordinate
 *              that is not finite (pc_box_bin_range then gives no range and the group is never dropped) */
typedef struct oslamk_order {
    const float *sx, *sy, *sz;
    const uint32_t *perm;
    const float *box;
} oslamk_order;
#define OSLAMK_ORDER_GROUP 64

/* Bucket of one key in one slice, addressed directly by the key's slot in the union table:
 * what a vote workgroup reads instead of probing (the scene-key kernel already found the slot). */
typedef struct oslamk_uinfo {
    uint32_t start;            /* first entry of the bucket */
    uint32_t len;              /* bucket length (0 = the slice has no pair with this key); bit 31: the bucket holds a marker entry */
} oslamk_uinfo;

typedef struct oslamk_table {
    oslamk_slot *slots;        /* [n_slices][cap]: the build's counting tables (kept for the taps and the file) */
    uint32_t cap;              /* power of two */
    uint32_t shift;            /* 32 - log2(cap) */
    int n_slices;
    uint32_t *ukeys;           /* [ucap] union of the keys of all slices (0 = empty) */
    uint32_t ucap;             /* power of two */
    uint32_t ushift;
    /* reach[k1 / 32] bit k1 % 32: some key of the model can come from a pair in distance bin k1
     * (FNV collisions included), k1 < OSLAMK_REACH_BINS; pairs in other bins cannot hit */
    uint32_t *reach;
    uint32_t reach_words;      /* words of `reach` up to and including the last one that has a bit set */
    /* kmap[k1 * 17^3 + combo], k1 < kmap_bins: the number (uids) of the key that distance bin k1 and the
     * angle bins `combo` hash to (pc_key_of_bins), or OSLAMK_KMAP_NONE; covers every reachable bin unless the
     * model spans more than OSLAMK_KMAP_MAX_BINS of them (the rest are hashed and probed) */
    uint32_t *kmap;            /* holds key numbers (uids), not slots */
    uint32_t kmap_bins;
    /* uids[slot]: the dense number (0 .. n_ids-1) of the key in union-table slot `slot`.  From the scene-key
     * kernel on a key is known by this number: the hit lists sort on id_bits = ceil(log2 n_ids) bits (16 for the
     * 38 000 keys of a 5 k-point model: two 8-bit passes instead of three) and the bucket records below take
     * 8 B x n_ids per slice instead of 8 B x ucap.  Number 0 is the key with the most entries in its buckets (all
     * slices, all members of a group), ties by ascending key: a reference point's runs are sorted by this number, so
     * a vote workgroup hands its heavy buckets out first (oslam_build_kmap).  The allocation holds the weights
     * behind the numbers: OSLAMK_UWEIGHTS(t)[slot] = entries under the key of union slot `slot` */
    uint32_t *uids;
    uint32_t n_ids, id_bits, uinfo_stride;
    oslamk_uinfo *uinfo;       /* [n_slices][uinfo_stride], indexed by the key's number */
} oslamk_table;
#define OSLAMK_UWEIGHTS(t) ((unsigned long long *)((t).uids + (t).ucap))
#define OSLAMK_KMAP_NONE 0xffffffffu
#define OSLAMK_KMAP_MAX_BINS 2048

/* The slot rule of the slice tables (shift = table.shift) and of the union table (table.ushift): where the probe
 * sequence of a key starts.  The one text of it, for the kernels that build and probe the tables and for the host
 * taps that read them back. */
#ifdef __HIPCC__
__host__ __device__
#endif
static inline uint32_t oslamk_slot_of(uint32_t key, uint32_t shift)
{
    return (key * 2654435761u) >> shift;
}

#define OSLAMK_REACH_BINS 16384

/* Counters one vote launch accumulates (device memory, zeroed by the host). */
typedef struct oslamk_counters {
    unsigned long long hits;
    unsigned long long votes;
    unsigned long long nonzero_cells;
    uint32_t gmax;
    uint32_t out_count;
    uint32_t redo_count;          /* vote workgroups of the current launch whose 16-bit counters overflowed (redo list length) */
    uint32_t redo_total;          /* the same, summed over the launches of a call */
    unsigned long long entries;   /* model pair entries streamed: sum of the bucket lengths over (run, slice) */
    unsigned long long items;     /* (run, slice) pairs with a bucket */
    unsigned long long prof[4];   /* -DVOTE_PROF builds: k_vote wave cycles (pre-scan, voting, wait at the barrier behind it, peak extraction) */
    uint32_t list_overflow;       /* bit 0: a hit list was too short for its hits (the counting and the hit kernel disagreed); bits 1..3: the
                                   * near-edge search met a key number, a bucket or a directory place out of range.  The call fails */
    uint32_t pad_;
} oslamk_counters;

typedef struct oslamk_cell {
    unsigned long long code;
    uint32_t count;
    uint32_t pad;
} oslamk_cell;

int oslamk_row_keys(oslamk_cloud c, int ref, float d_dist, float inv_d_dist, uint32_t *keys_out,
                    void *stream);

/* model build, pass 1: count pairs per (slice, key); n_unique[n_slices]; *overflow set if a
 * slice table filled up */
int oslamk_model_count(oslamk_cloud c, float d_dist, float inv_d_dist, oslamk_table t,
                       uint32_t *n_unique, uint32_t *overflow, void *stream);
/* exclusive scan of slot.len (each rounded up to a multiple of 4) over all slots -> slot.start;
 * padded total written to *total_out */
int oslamk_table_scan(oslamk_table t, uint32_t *total_out, void *stream);
/* fill t.ukeys with every distinct key; *n_keys = number of distinct keys */
int oslamk_union_build(oslamk_table t, uint32_t *n_keys, uint32_t *overflow, void *stream);
/* fill t.reach by enumerating every key each distance bin can produce */
int oslamk_reach_build(oslamk_table t, float d_dist, void *stream);
/* weights[slot of the key in t.ukeys] += slot.len for every key of t's slice tables (weights zeroed by the caller; a
 * group calls it once per member, each with its own slice tables under the group's t.ukeys) */
int oslamk_union_weights(oslamk_table t, unsigned long long *weights, void *stream);
/* fill t.kmap (t.kmap_bins rows) from t.ukeys / t.uids */
int oslamk_kmap_build(oslamk_table t, float d_dist, void *stream);
/* model build, pass 2: write entries. tmg = [M][8] rows y,z of T_m_g (host-computed). */
int oslamk_model_fill(oslamk_cloud c, float d_dist, float inv_d_dist, oslamk_table t,
                      const float *tmg, oslamk_entries ent, void *stream);

/* model build, pass 3: inside every bucket, order the entries so that the 32 lanes the LDS serves
 * together carry evenly spaced theta_u (fewer bank conflicts of the vote atomics) */
int oslamk_bucket_spread(oslamk_table t, oslamk_entries ent, void *stream);
/* model build, pass 4 (exact mode): ent.pw / ent.puv from ent.e4 / ent.uv, see oslamk_entries */
int oslamk_bucket_psort(oslamk_table t, oslamk_entries ent, void *stream);

/* A scene pair whose key is in the model ("hit"): what a vote needs of it.  The rows y,z of
 * T_s_g * s_i (kernel.cu:334-336) that the rare exact re-evaluation needs are recomputed from the
 * scene index. */
typedef struct oslamk_pay {
    uint32_t theta_t22;        /* pc_angle_t22 of (T_s_g * s_i).y/.z */
    uint32_t idx;              /* scene index of s_i */
} oslamk_pay;

/* A run of hits of one reference point that share a key (at most 64 of them). */
typedef struct oslamk_run {
    uint32_t slot_r;           /* union-table slot of the key | (hits - 1) << OSLAMK_RUN_SHIFT */
    uint32_t first;            /* first hit of the run in the reference point's sorted hit list; bit 31: a hit of the run carries
                                * the "always re-evaluate" marker */
} oslamk_run;
#define OSLAMK_RUN_SHIFT 26    /* union tables have at most 2^26 slots */

typedef struct oslamk_vote_args {
    oslamk_cloud scene;
    const uint32_t *ref_idx;   /* [n_ref] scene indices of this shard's reference points */
    const float *tsg;          /* [n_ref][8] rows y,z of T_s_g per reference point */
    int n_ref;
    float d_dist, inv_d_dist;
    oslamk_table table;
    oslamk_entries ent;
    float thresh;              /* vote_count_threshold */
    uint32_t fixed_gmax;       /* != 0: emit cells with count > thresh*fixed_gmax only */
    oslamk_counters *counters;
    oslamk_cell *out;          /* [out_cap] */
    uint32_t out_cap;
    uint32_t *acc_dump;        /* optional [n_slices*SLICE][NBIN] for reference ordinal dump_ref */
    int dump_ref;
    int first_ref;             /* launch covers reference ordinals first_ref .. first_ref+n_launch-1 */
    int n_launch;
    int mode;                  /* 0 exact (near-edge votes re-evaluated), 1 fast (never) */
    /* Hit lists of the batch, sized by demand: reference point ref_local owns the slots
     * hit_off[ref_local] .. hit_off[ref_local + 1] of every array below; the size is the number of its
     * scene pairs whose distance bin can reach a model key (oslamk_scene_count), an upper bound of its hits.
     *   hit_key / hit_pay : hits in arrival order (oslamk_scene_hits): number of the key, payload; oslamk_sort_hits
     *                       overwrites hit_key with the key numbers in SORTED order | run-holds-a-marker << 31
     *   hit_sorted        : the payloads ordered by slot (oslamk_sort_hits) -- what oslamk_vote reads
     *   runs              : runs of equal keys in hit_sorted, run_count[ref_local] of them */
    uint32_t *keep_count;      /* [n_launch] written by oslamk_scene_count (must be zero on entry) */
    const uint32_t *hit_off;   /* [n_launch + 1] */
    uint32_t *hit_key;
    oslamk_pay *hit_pay;
    oslamk_pay *hit_sorted;
    oslamk_run *runs;
    uint32_t *hit_count;       /* [n_launch] */
    uint32_t *run_count;       /* [n_launch] */
    uint32_t *redo;            /* [vote workgroups of the batch] list of those whose 16-bit counters overflowed */
    /* optional [n_launch]: the reference point (ref_local) that dispatch position p of the vote grid works on, a
     * permutation of 0 .. n_launch-1; NULL = identity.  The host orders it by descending demand, so that the last
     * rounds of workgroups are light ones.  A value outside the batch means no work */
    const uint32_t *ref_order;
    oslamk_order order;        /* the scene in groups of neighbours, what phase 1 of the scene-key kernels walks */
} oslamk_vote_args;

/* fill t.uinfo from the slice tables (after oslamk_table_scan / oslamk_union_build and the fill pass) */
int oslamk_uinfo_build(oslamk_table t, void *stream);

/* keep_count[ref_local] += scene pairs of the reference point whose distance bin can reach a model key */
int oslamk_scene_count(const oslamk_vote_args *a, void *stream);
/* scene pair keys -> per-reference hit lists, for reference ordinals first_ref..+n_launch-1;
 * hit_count[0..n_launch) must be zero on entry */
int oslamk_scene_hits(const oslamk_vote_args *a, void *stream);
/* hit lists -> hits_sorted (by key), same batch */
int oslamk_sort_hits(const oslamk_vote_args *a, void *stream);
/* votes of the same batch (needs the sorted hit lists) */
int oslamk_vote(const oslamk_vote_args *a, void *stream);
/* the two re-vote passes over the launch's redo list (called by oslamk_vote) */
int oslamk_vote_wide(const oslamk_vote_args *a, void *stream);
/* the votes of nm models that share the scene pass (a database group) in one grid: d_all[nm] in device memory, h_all the
 * same on the host (every member with the same batch of reference points and the same mode, its own redo list).  The
 * re-vote passes are not queued here: the caller looks at the members' redo counts and runs oslamk_vote_wide for the
 * (rare) member that has any */
int oslamk_vote_group(const oslamk_vote_args *d_all, const oslamk_vote_args *h_all, int nm, void *stream);

/* voxel grid (oslam_voxel.hip): out6 = device [n][6] (x y z nx ny nz per voxel); returns a
 * hipError_t, or -1 when the voxel count overflows int32 */
int oslamk_voxel_grid(oslamk_cloud c, float leaf, float *out6, uint32_t *n_out, void *stream);

/* depth image -> points + normals (oslam_depth.hip): d_img = device image (uint16 or float, w x h),
 * d_out6 = device [w*h][6]; the pixels that get a normal, in row-major order; returns a hipError_t */
int oslamk_depth_to_cloud(const void *d_img, int is_u16, int w, int h, float fx, float fy, float cx, float cy,
                          float scale, float z_min, float z_max, float max_jump, float *d_out6, uint32_t *n_out,
                          void *stream);

/* Device memory of the per-frame scene path (depth image, voxel grid, scene arrays).  hipFree waits for the device --
 * 0.2 ms a time, and a depth frame freed a dozen blocks -- so freed blocks are kept (per device, up to a limit) and
 * handed out again to requests they fit.  Everything on this path runs on one stream and is waited for before its
 * buffers are given back, so a block is never reused under a kernel.  oslam_dev_alloc returns a hipError_t as int;
 * oslam_release_scratch gives the kept blocks of a device back to the driver. */
int oslam_dev_alloc(void **p, size_t bytes);
void oslam_dev_free(void *p);
void oslam_dev_cache_release(int dev);

/* device [n][6] (x y z nx ny nz) -> device structure of arrays [6][n] */
int oslamk_aos6_to_soa(const float *d_in6, size_t n, float *d_soa, void *stream);

/* clustering scores of n poses (device arrays).  shash[j] = cell hash of the j-th pose in
 * (hash, pose index) order and sidx[j] its pose index; sq/st/sw = quaternions [n][4], translations [n][3], weighted
 * votes [n] in that order; cell [n][3] in pose order; score [n] in pose order.  The translation-averaging variant stays on the host. */
int oslamk_cluster_scores(int n, const int *cell, const uint32_t *shash, const uint32_t *sidx,
                          const float *sq, const float *st, const float *sw, float d_dist, int use_l1,
                          float *score, int whole_host, const unsigned long long *whole_dev, uint32_t *table, void *stream);
/* whole_host / whole_dev: the weighted votes are whole numbers with a sum below 2^24 - 1 (their float sum is then exact
 * in any order and the kernel adds them lane-parallel); whole_dev, if not NULL, points to {sum, not-whole flag} on the device */
/* table: device work space of oslamk_cluster_table_words(n) 32-bit words (the cells of the sorted list, hashed) */
size_t oslamk_cluster_table_words(int n);

/* pose tail on the device (oslam_posegpu.hip): filter, order, poses, clustering scores, winner.
 * d_Tm16 [M][16] / d_Ts16 [ceil(S/df)][16]: the frames T_g of the model points and of the scene's
 * reference-point candidates (host libm); h_rotx_cs: oslam_rotx_table.  Returns a hipError_t, -2 = no host memory */
/* The instance selection of oslam_align_instances (include/oslam.h), resolved for one model: at most max_instances
 * (1..OSLAMK_MAX_INSTANCES) winners; floor = ratio * the first winner's score; two poses are the same instance when
 * their transformed centroids c lie closer than sqrt(sep2) (d2 < sep2) and, when rot_on, their rotation sum is
 * >= cos_thr. */
#define OSLAMK_MAX_INSTANCES 64
typedef struct oslamk_inst_args {
    uint32_t max_instances;
    float ratio, sep2, cos_thr;
    int32_t rot_on;
    float c[3];
} oslamk_inst_args;
/* what the selection leaves in a slot: n winners, each with its candidate index, score and pose (the pose with the
 * translation of the clustering stage), in the order they were accepted */
typedef struct oslamk_inst_out {
    uint32_t n;
    uint32_t idx[OSLAMK_MAX_INSTANCES];
    float score[OSLAMK_MAX_INSTANCES];
    float T[OSLAMK_MAX_INSTANCES][16];
} oslamk_inst_out;

/* ia: NULL = the winner only; otherwise the instance selection runs after it and *inst receives its result */
int oslamk_pose_stage(const oslamk_cell *d_cells_in, uint32_t n_in, float min_votecount, const float *d_Tm16,
                      const float *d_Ts16, uint32_t df, const float *d_weights, const float *h_rotx_cs, float d_dist,
                      int use_l1, oslamk_cell *d_cells_out, float *d_poses, uint32_t gmax, uint32_t model_points,
                      uint32_t scene_points, int two_sorts, const oslamk_inst_args *ia, uint32_t *n_out, uint32_t *best_out,
                      float T_best[16], oslamk_inst_out *inst, void *stream);
/* gmax (the largest count among the records), model_points and scene_points bound the fields of a record: with few
 * enough bits the cells are ordered by one sort of packed keys (two_sorts != 0: never) */

/* The same tail in pieces, for several models in flight on one stream (a database frame): reserve once for the largest
 * record count and the number of models, enqueue every model's selection, wait, read the counts, enqueue every model's
 * chain (n >= 2 selected records), wait, read the results.  The chains share the work space: they run in stream order. */
int oslamk_pose_reserve(uint32_t n_max, uint32_t slots, const float *h_rotx_cs, void *stream);
int oslamk_pose_select_async(const oslamk_cell *d_in, uint32_t n_in, float min_votecount, oslamk_cell *d_sel, uint32_t slot,
                             void *stream);
uint32_t oslamk_pose_selected(uint32_t slot);
int oslamk_pose_finish_async(uint32_t n, const oslamk_cell *d_sel, const float *d_Tm16, const float *d_Ts16, uint32_t df,
                             const float *d_weights, float d_dist, int use_l1, oslamk_cell *d_cells_out, float *d_poses,
                             uint32_t gmax, uint32_t model_points, uint32_t scene_points, int two_sorts,
                             const oslamk_inst_args *ia, uint32_t slot, void *stream);
void oslamk_pose_result(uint32_t slot, uint32_t *best_out, float T_best[16]);
/* test tap: the clustering scores [n] of the last chain over n records, to the host */
int oslamk_pose_scores(uint32_t n, float *h_score, void *stream);
/* the instance selection of a chain that was given ia (after the wait) */
void oslamk_pose_instances(uint32_t slot, oslamk_inst_out *out);

/* records with count > min_votecount, compacted into d_out (capacity n_in); *n_out on the host */
int oslamk_select_cells(const oslamk_cell *d_in, uint32_t n_in, float min_votecount, oslamk_cell *d_out, uint32_t *n_out,
                        void *stream);
/* frees the pose tail's work space on the current device */
void oslamk_pose_release(void);

/* device self-test: out_acos[i] = pm_acosf(x[i]); out_atan2[i] = pm_atan2f(y[i], x2[i]);
 * out_bin[i] = pc_alpha_bin_exact(...) */
int oslamk_selftest(const float *x, const float *y, const float *x2, size_t n, float *out_acos,
                    float *out_atan2, uint32_t *out_quant, uint32_t *out_bin, void *stream);

/* ---- refinement stage (oslam_refine.hip; semantics in include/oslam.h at oslam_refine) ---- */
#define OSLAMK_REFINE_THREADS 256    /* model points per workgroup of the correspondence kernels */
#define OSLAMK_REFINE_SUMS 29        /* per point: J^T J upper triangle (21, row-major), J^T r (6), count, r^2 */
#define OSLAMK_REFINE_STRIDE 32      /* floats per (member, workgroup) of the step slab */
#define OSLAMK_SCAN_ITEMS 4096       /* grid cells per workgroup of the exclusive scan (256 threads x 16) */
#define OSLAMK_GRID_MAX_CELLS (1u << 24)
#define OSLAMK_REFINE_STEP 0         /* correspondence kernel modes */
#define OSLAMK_REFINE_SCORE 1
#define OSLAMK_REFINE_TAP 2

/* Dense uniform grid over a scene's bounding box: cell (cx, cy, cz) = floor((x - lo) * inv_edge) per axis (in double,
 * clamped to the grid), flat index (cz * dim[1] + cy) * dim[0] + cx; the points of cell c are pts[start[c] ..
 * start[c + 1]) in any order (the correspondence rule does not depend on it). */
typedef struct oslamk_grid {
    double lo[3];
    double inv_edge;
    int dim[3];
    uint32_t n_cells;
    int n;                     /* scene points */
    uint32_t *start;           /* [n_cells + 1] */
    float *pts;                /* [n][8]: x y z (scene index, int bits) nx ny nz 0 */
    uint32_t *local;           /* build work space: [n_cells + 1] counts, then their scan inside each 4096-cell block */
    uint32_t *bsum;            /* [(n_cells + 1 + 4095) / 4096] block totals, then their exclusive scan */
    uint32_t *cell_of, *rank;  /* [n]: cell of each point, its place among the points of that cell */
} oslamk_grid;

/* One member of a refinement call.  The host fills everything; the solve kernel updates the state fields. */
typedef struct oslamk_refine_member {
    double T[12];              /* rows of [R | t] in double: the pose between iterations */
    double cm[3];              /* model centroid (double mean of the points) */
    oslamk_cloud m;            /* the model's points and normals (SoA in HBM) */
    float Tf[12];              /* float32 rounding of T: what the correspondences use */
    float c[3];                /* float32 rounding of T * cm */
    float r2_corr, r2_score;   /* radius^2 of the step and of the score (float) */
    float min_dot;
    float stop_rot, stop_trans;   /* stop_trans in scene units */
    uint32_t max_iter;
    uint32_t n_blocks;         /* workgroups of this member: ceil(m.n / OSLAMK_REFINE_THREADS) */
    int32_t active;            /* 0: skipped (all-zero T_in) */
    int32_t done, iterations, converged, n_corr;
} oslamk_refine_member;

/* grid of the scene cloud c: g->lo, inv_edge, dim, n_cells and the device arrays are set by the caller */
int oslamk_refine_grid_build(const oslamk_grid *g, oslamk_cloud c, void *stream);
/* mode STEP: slab[(j * max_blocks + b) * OSLAMK_REFINE_STRIDE + k] = sums of member j's workgroup b (done members are
 * skipped); mode SCORE: slab[(j * max_blocks + b) * 2 + {0, 1}] = inliers, sum of d^2 (inactive members skipped);
 * mode TAP: idx_out[i] of member 0 */
int oslamk_refine_corr(int mode, const oslamk_grid *g, const oslamk_refine_member *d_mem, uint32_t n_mem,
                       uint32_t max_blocks, float *slab, int32_t *idx_out, void *stream);
/* one wave per member that is not done: sums its slab in double, solves, updates the pose; *n_done counts the members
 * that have become done */
int oslamk_refine_solve(oslamk_refine_member *d_mem, uint32_t n_mem, uint32_t max_blocks, const float *slab,
                        uint32_t *n_done, void *stream);

/* ---- normal estimation (oslam_normals.hip; semantics in include/oslam.h at oslam_cloud_normals) ---- */
#define OSLAMK_NORMALS_THREADS 256   /* grid positions per workgroup of k_normals */
typedef struct oslamk_normals_args {
    float r2, scale;           /* radius * radius and 16384.0f / radius, both rounded by the host */
    double view[3];
    double line_ratio;
    int64_t min_neighbours;
    int orient;
    float *nrm;                /* [n][3], by input index */
    float *curvature;          /* [n] */
    uint8_t *valid;            /* [n] */
    int64_t *moments;          /* [n][10], or NULL */
} oslamk_normals_args;
/* one thread per position of g->pts (a grid built by oslamk_refine_grid_build): writes every point's outputs */
int oslamk_normals(const oslamk_grid *g, const oslamk_normals_args *a, void *stream);

/* ---- verification stage (oslam_verify.hip; semantics in include/oslam.h at oslam_verify) ---- */
#define OSLAMK_VERIFY_THREADS 256    /* model points per workgroup of k_verify */
#define OSLAMK_VERIFY_CLASSES 6

/* the camera of a view and its z image: w * h floats, z of a valid pixel (> 0 since z_min > 0), 0 = invalid */
typedef struct oslamk_view {
    const float *z;
    int w, h;
    float fx, fy, cx, cy, z_min, z_max;
} oslamk_view;

/* one member of a verification call */
typedef struct oslamk_verify_member {
    oslamk_cloud m;            /* the model's points and normals (SoA in HBM, the cloud oslam_refine reads) */
    float T[12];               /* rows of [R | t], float32 */
    float tol;                 /* (float)((double)depth_tol * d_dist) */
    uint32_t n_blocks;         /* ceil(m.n / OSLAMK_VERIFY_THREADS); 0 = skipped */
} oslamk_verify_member;

/* d_raw: the image in HBM (uint16 or float, w x h row-major) -> d_z (float, w x h) */
int oslamk_view_z(const void *d_raw, int is_u16, int w, int h, float scale, float z_min, float z_max, float *d_z,
                  void *stream);
/* counts (class_out NULL): counts[j * OSLAMK_VERIFY_CLASSES + c] += points of member j in class c (zeroed by the
 * caller); tap (class_out != NULL): class_out[i] = the class of member 0's point i */
int oslamk_verify(const oslamk_view *v, const oslamk_verify_member *d_mem, uint32_t n_mem, uint32_t max_blocks,
                  int window, uint32_t *counts, uint8_t *class_out, void *stream);

/* ---- arbitration stage (oslam_arbitrate.hip; semantics in include/oslam.h at oslam_arbitrate) ---- */
#define OSLAMK_ARB_MAX_HYP 1024       /* hypotheses of one call: k_arbitrate keeps four words of each in LDS */
#define OSLAMK_ARB_THREADS 256        /* the one workgroup of k_arbitrate */
#define OSLAMK_ARB_LDS_BYTES 40960    /* a claims table up to this size is copied into LDS for the elimination */
#define OSLAMK_ARB_CNT_SHIFT 40       /* a claims word: count in the upper 24 bits, sum of q in the lower 40 */

/* the tiling of a call: tile x tile pixels, tiles_x = ceil(w / tile), n_tiles = tiles_x * ceil(h / tile) */
typedef struct oslamk_arb_grid {
    int tile, tiles_x;
    uint32_t n_tiles;
} oslamk_arb_grid;

/* what k_arbitrate leaves for hypothesis h (rec[1 + h]); rec[0].claimed = the rounds of the call */
typedef struct oslamk_arb_rec {
    uint32_t claimed, owned;
    float share;
    int32_t kept, suppressed_by;
    uint32_t cnt_total;        /* its SUPPORTED points */
    uint64_t sum_total;        /* the sum of their q */
} oslamk_arb_rec;

/* claims[h * n_tiles + t] += (1 << 40) + q for every SUPPORTED point of member h in tile t (zeroed by the caller) */
int oslamk_claim(const oslamk_view *v, const oslamk_verify_member *d_mem, uint32_t n_mem, uint32_t max_blocks, int window,
                 oslamk_arb_grid g, unsigned long long *claims, void *stream);
/* the elimination over the claims of n_mem members (n_blocks == 0: skipped) -> rec[1 + n_mem] */
int oslamk_arbitrate(const oslamk_verify_member *d_mem, uint32_t n_mem, uint32_t n_tiles, const unsigned long long *claims,
                     uint32_t min_tiles, float min_owned_share, oslamk_arb_rec *rec, void *stream);

/* ---- tracking stage (oslam_track.hip; semantics in include/oslam.h at oslam_track) ---- */
#define OSLAMK_TRACK_THREADS 256      /* the one workgroup of a hypothesis; a block of the sums is 256 model points */

/* one hypothesis of a tracking call; the host fills everything */
typedef struct oslamk_track_member {
    double T[12];              /* rows of [R | t]: the input pose (float32 values) */
    double cm[3];              /* model centroid (double mean of the points) */
    oslamk_cloud m;            /* the model's points and normals (SoA in HBM) */
    float c[3];                /* float32 rounding of T * cm */
    float r2_corr, min_dot;
    float stop_rot, stop_trans;   /* stop_trans in scene units */
    float tol;                 /* of the judgement: (float)((double)depth_tol * d_dist) */
    uint32_t max_iter;
    uint32_t n_blocks;         /* ceil(m.n / OSLAMK_TRACK_THREADS); 0 = skipped */
} oslamk_track_member;

/* what k_track leaves for a hypothesis that is not skipped */
typedef struct oslamk_track_rec {
    float T[12];               /* the final float32 pose */
    uint32_t counts[OSLAMK_VERIFY_CLASSES];   /* the classes of oslam_verify at that pose */
    uint32_t n_corr, iterations;
    int32_t converged, pad;
} oslamk_track_rec;

/* maps[(v * w + u) * 8 ..]: x y z has | nx ny nz 0 of pixel (u, v), has = 1.0f where the pixel has a normal (zeros
 * elsewhere); from the z image of the view */
int oslamk_view_normals(const oslamk_view *v, float max_jump, float *maps, void *stream);
/* one workgroup per member: every iteration, then the judgement -> rec[n_mem] */
int oslamk_track(const oslamk_view *v, const float *maps, const oslamk_track_member *d_mem, uint32_t n_mem, int window,
                 oslamk_track_rec *rec, void *stream);
/* tap: pixel_out[i] = pixel of the correspondence of member 0's point i, -1 = none */
int oslamk_track_corr(const oslamk_view *v, const float *maps, const oslamk_track_member *d_mem, uint32_t n_blocks,
                      int32_t *pixel_out, void *stream);

/* ---- camera motion stage (oslam_ego.hip; semantics in include/oslam.h at oslam_view_egomotion) ---- */
#define OSLAMK_EGO_THREADS 256        /* a block of the sums is 256 consecutive selected pixels */
#define OSLAMK_EGO_MAX_LEVELS 3
#define OSLAMK_EGO_MAX_SLOTS 256      /* workgroups of one launch at most: one slot of the partials buffer each */
#define OSLAMK_EGO_STRANDS 8          /* the slots are added in 8 interleaved strands */
#define OSLAMK_EGO_SLOT 32            /* doubles per slot: the 29 sums, [29] = selected source pixels with a normal */

/* the selected pixels of one level: the lattice u % stride == 0 && v % stride == 0 of the source image, row-major */
typedef struct oslamk_ego_level {
    int stride, lw;            /* lw = ceil(w / stride) lattice columns */
    uint32_t n;                /* lattice points: lw * ceil(h / stride) */
    uint32_t n_blocks;         /* ceil(n / OSLAMK_EGO_THREADS) */
    uint32_t chunk;            /* consecutive blocks per workgroup: ceil(n_blocks / OSLAMK_EGO_MAX_SLOTS) */
    uint32_t n_slots;          /* workgroups: ceil(n_blocks / chunk) */
    uint32_t max_iter;
    int32_t level, next_level; /* this level's index; the next level that has iterations (or the number of levels) */
} oslamk_ego_level;

/* the state of a call: the host fills the pose and the gates, every step updates the rest */
typedef struct oslamk_ego_state {
    double T[12];              /* rows of [R | t] in double: the pose between iterations */
    float Tf[12];              /* float32 rounding of T: what the correspondences use */
    float c[3];                /* float32 rounding of t: the pivot (the model centroid is the origin) */
    float r2_corr, min_dot, stop_rot, stop_trans;
    int32_t level, iter;       /* the level in force and the steps taken in it */
    int32_t done, converged;
    int32_t n_levels, pad;
    uint32_t iterations[OSLAMK_EGO_MAX_LEVELS];
    uint32_t corr[OSLAMK_EGO_MAX_LEVELS], n_src[OSLAMK_EGO_MAX_LEVELS];   /* of the level's last step */
    uint32_t last_corr;        /* correspondences of the last step of the call */
    float rmse;                /* of that step */
} oslamk_ego_state;

/* one scheduled iteration: returns at once when the call is done or lv->level is not the level in force; otherwise
 * every workgroup leaves its sums in slots[blockIdx.x] and the last one to arrive at *arrive (zero before the launch,
 * used by this launch alone) adds them, steps and writes *st */
int oslamk_ego_step(const oslamk_view *src, const float *src_maps, const oslamk_view *dst, const float *dst_maps,
                    const oslamk_ego_level *lv, oslamk_ego_state *st, double *slots, uint32_t *arrive, void *stream);
/* tap: pixel_out[i] = pixel in dst of the correspondence of source pixel i under T (float32 rows), -1 = none */
int oslamk_ego_corr(const oslamk_view *src, const float *src_maps, const oslamk_view *dst, const float *dst_maps,
                    const float *T12, float r2_corr, float min_dot, int32_t *pixel_out, void *stream);

/* ---- image pyramid (oslam_pyramid.hip; semantics in include/oslam.h at oslam_pyramid_create) ---- */
/* the z image of the next coarser level of *src: z_out [(h + 1) / 2][(w + 1) / 2], clamped to src's [z_min, z_max] */
int oslamk_pyr_down(const oslamk_view *src, float depth_band, float *z_out, void *stream);

/* ---- bilateral depth filter (oslam_bilateral.hip; semantics in include/oslam.h at oslam_view_bilateral) ---- */
#define OSLAMK_BILATERAL_MAX_RADIUS 8 /* the largest half-width of the window in pixels: sizes the kernel's LDS tile */

/* z_out [h][w] = the z image of *src filtered over the (2 radius + 1)^2 window with inv_s = 1 / sigma_space^2 and
 * inv_r = 1 / sigma_depth^2, clamped to src's [z_min, z_max]; counts[0 .. 2) (zeroed by the caller) += the valid pixels
 * of z_out, the taps that took part */
int oslamk_bilateral(const oslamk_view *src, int radius, float inv_s, float inv_r, float *z_out, uint32_t *counts,
                     void *stream);

/* ---- render stage (oslam_render.hip; semantics in include/oslam.h at oslam_render_create / oslam_view_mask) ---- */
#define OSLAMK_RENDER_MAX_SPLAT 8     /* the largest half-width of a splat in pixels */
#define OSLAMK_MASK_MAX_DILATE 8      /* the largest half-width of the mask's window in pixels */

/* keys[w * h] (all ones before the launch) = min over the drawn points of (bits of p'z) << 32 | member; the camera and
 * size are *v's (v->z is not read); rho[j]: member j's splat radius in metres; drawn[j] (zeroed by the caller) += the
 * points of member j that were splatted.  The grid and the descriptors are oslamk_verify's */
int oslamk_render_splat(const oslamk_view *v, const oslamk_verify_member *d_mem, const float *d_rho, uint32_t n_mem,
                        uint32_t max_blocks, int max_splat, int keep_back, unsigned long long *keys, uint32_t *drawn,
                        void *stream);
/* keys -> z_out [w * h] (0 = nothing drawn) and labels [w * h] (-1 = nothing drawn); pixels[j] (zeroed by the caller) +=
 * the pixels labelled j; tol_out[j] = d_mem[j].tol for j < n_mem */
int oslamk_render_resolve(const unsigned long long *keys, int w, int h, const oslamk_verify_member *d_mem, uint32_t n_mem,
                          float *z_out, int32_t *labels, float *tol_out, uint32_t *pixels, void *stream);
/* *v without (mode 0) or with only (mode 1) the object pixels under the render z_r / labels / tol of the same size ->
 * z_out [w * h]; counts[0 .. 3) (zeroed by the caller) += valid pixels of *v, object pixels, valid pixels of z_out */
int oslamk_view_mask(const oslamk_view *v, const float *z_r, const int32_t *labels, const float *tol, int mode, int dilate,
                     int32_t only, float *z_out, uint32_t *counts, void *stream);

/* ---- planes stage (oslam_planes.hip; semantics in include/oslam.h at oslam_view_planes) ---- */
#define OSLAMK_PLANES_MAX 8           /* rounds of one call at most */
#define OSLAMK_PLANES_CAND 256        /* the 16 x 16 lattice nodes: one thread of a workgroup each */
#define OSLAMK_PLANES_MAX_GROUPS 512  /* workgroups of the score and moments kernels at most */
#define OSLAMK_PLANES_BOUND 131072.0f /* |(p_a - p0_a) * scale| above this leaves a pixel out of the fit */

/* one plane: the layout of oslam_plane */
typedef struct oslamk_plane {
    float normal[3], d;
    uint32_t support, pixels, candidate;
    float rms;
} oslamk_plane;

/* the device block of one call, zeroed before the first launch */
typedef struct oslamk_planes_block {
    uint32_t done;             /* 0 while the search runs; 1 = count below min_pixels, 2 = degenerate fit, 3 = no candidate */
    uint32_t n_planes;
    uint32_t valid_in;         /* pixels with z > 0 (round 0's score kernel counts them) */
    uint32_t pad;
    uint32_t counts[OSLAMK_PLANES_MAX][OSLAMK_PLANES_CAND];
    unsigned long long moments[OSLAMK_PLANES_MAX][10];    /* int64 sums, added as two's complement */
    oslamk_plane rec[OSLAMK_PLANES_MAX];
} oslamk_planes_block;

typedef struct oslamk_planes_args {
    oslamk_view v;
    const float *maps;         /* [h][w][8]: x y z has | nx ny nz 0 */
    int32_t *labels;           /* [h][w], all -1 before the first launch */
    oslamk_planes_block *blk;
    float dist_tol, min_normal_dot, label_min_dot;
    float scale;               /* 16.0f / dist_tol, made once by the host */
    uint32_t min_pixels;       /* resolved: never the 0 of the parameters */
    double line_ratio;
} oslamk_planes_args;

/* every kernel of a call: per round k_planes_score, k_planes_moments, k_planes_round, k_planes_label; 4 * max_planes
 * launches whatever the image holds */
int oslamk_planes_find(const oslamk_planes_args *a, unsigned max_planes, void *stream);
/* *v without (mode 0) or with only (mode 1) the pixels whose label is >= 0 (only >= 0: == only) -> z_out [w * h];
 * counts[0 .. 3) (zeroed by the caller) += valid pixels of *v, plane pixels among them, valid pixels of z_out */
int oslamk_planes_mask(const oslamk_view *v, const int32_t *labels, int mode, int32_t only, float *z_out, uint32_t *counts,
                       void *stream);

/* ---- segments stage (oslam_segments.hip; semantics in include/oslam.h at oslam_view_segments) ---- */
#define OSLAMK_SEG_MAX 64             /* segment records of one call at most */
#define OSLAMK_SEG_CAND 4096          /* components that may pass min_pixels in one call */
#define OSLAMK_SEG_TILE 32            /* side of k_seg_tile's tile in pixels */
#define OSLAMK_SEG_LAUNCHES 6         /* kernels of one call, whatever the image holds */
#define OSLAMK_SEG_SCALE 8192.0f      /* the centroid sums' units per metre */
#define OSLAMK_SEG_BOUND 1073741824.0f /* |p_a * 8192| above this (2^30) leaves a pixel out of the centroid */

/* one segment as the kernels leave it: the host turns it into an oslam_segment */
typedef struct oslamk_seg_acc {
    uint32_t pixels, root;
    uint32_t u0, v0, u1, v1;   /* bounding box, inclusive; k_seg_rank presets u0 = v0 = all ones */
    uint32_t n;                /* pixels that entered the sums */
    uint32_t pad;
    unsigned long long s[3];   /* int64 sums of q_a, added as two's complement */
} oslamk_seg_acc;

/* the device block of one call, zeroed before the first launch; the host reads it up to `cand` */
typedef struct oslamk_seg_block {
    uint32_t n_components, n_candidates, valid_in;
    uint32_t overflow;         /* 1: more than OSLAMK_SEG_CAND candidates, nothing was ranked or labelled */
    oslamk_seg_acc acc[OSLAMK_SEG_MAX];
    uint32_t cand[OSLAMK_SEG_CAND][2];   /* pixels, root; in the order the list was filled */
} oslamk_seg_block;

typedef struct oslamk_seg_args {
    oslamk_view v;
    const int32_t *plane_labels;   /* [h][w] or NULL: a pixel with a label >= 0 is not in */
    uint32_t *L;               /* [h][w]: the parent of every in pixel, OSLAM_SEG_NONE elsewhere; the roots at the end */
    uint32_t *tcount;          /* [h][w] scratch: at a tile-local root the pixels of its part of the tile, 0 elsewhere */
    uint32_t *count;           /* [h][w] scratch, zeroed before the first launch: at a root the pixels of the component,
                                  after k_seg_rank 1 << 31 | rank at the roots of the segments */
    int32_t *labels;           /* [h][w]: the rank of the pixel's segment or -1 */
    oslamk_seg_block *blk;
    float max_step, rel_step;
    uint32_t min_pixels;       /* resolved: never the 0 of the parameters */
    uint32_t max_segments;     /* 1..OSLAMK_SEG_MAX */
} oslamk_seg_args;

/* every kernel of a call: k_seg_tile, k_seg_seam, k_seg_flatten, k_seg_collect, k_seg_rank, k_seg_label */
int oslamk_segments_find(const oslamk_seg_args *a, void *stream);

/* ---- explain stage (oslam_explain.hip; semantics in include/oslam.h at oslam_explain) ---- */
/* the private z-buffer of one hypothesis: pixels [x0, x0 + w) x [y0, y0 + h) of the image, row-major from word `off` of
 * the pool; w == 0 or h == 0: it can draw nothing */
typedef struct oslamk_explain_rect {
    int x0, y0, w, h;
    unsigned long long off;
} oslamk_explain_rect;

/* the counters of one hypothesis (zeroed by the caller) */
typedef struct oslamk_explain_rec {
    uint32_t drawn, agree, occluded, through, unknown;
    uint32_t clipped;          /* points whose splat would have left the rectangle: not written */
    unsigned long long resid_sum;
} oslamk_explain_rec;

/* pool[rect[j].off + ...] (all ones before the launch) = min over member j's drawn points of the bits of p'z, the splat
 * of oslamk_render_splat into the member's own rectangle; rec[j].drawn and rec[j].clipped += */
int oslamk_explain_splat(const oslamk_view *v, const oslamk_verify_member *d_mem, const float *d_rho,
                         const oslamk_explain_rect *d_rect, uint32_t n_mem, uint32_t max_blocks, int max_splat,
                         int keep_back, uint32_t *pool, oslamk_explain_rec *rec, void *stream);
/* every pixel of every member's rectangle against *v: rec[j]'s class counters and resid_sum +=, and cnt[j * g.n_tiles +
 * t] (zeroed by the caller) += the AGREE pixels of member j in tile t; max_w, max_h: the largest rectangle's sides */
int oslamk_explain_score(const oslamk_view *v, const oslamk_verify_member *d_mem, const oslamk_explain_rect *d_rect,
                         uint32_t n_mem, int max_w, int max_h, const uint32_t *pool, oslamk_arb_grid g,
                         unsigned long long *cnt, oslamk_explain_rec *rec, void *stream);
/* cnt[j * n_tiles + t] = c  ->  c << 40 | c * conflict_q(rec[j]): the words oslamk_arbitrate reads */
int oslamk_explain_claims(const oslamk_explain_rec *rec, uint32_t n_mem, uint32_t n_tiles, unsigned long long *cnt,
                          void *stream);

/* ---- fusion stage (oslam_volume.hip; semantics in include/oslam.h at oslam_volume_integrate / oslam_volume_raycast) ---- */
#define OSLAMK_VOL_ZRUN 8             /* consecutive z a thread of k_tsdf_integrate walks; nz is a multiple of it */
#define OSLAMK_VOL_MAX_STEPS 1024     /* samples of one ray at most: step >= one voxel and the box's diagonal is below
                                         887 voxels, so the march never reaches it */

/* the volume: one word per voxel, int16 q | uint16 w << 16, x fastest, then y, then z */
typedef struct oslamk_volume {
    uint32_t *words;
    int nx, ny, nz;
    float voxel, inv_voxel;    /* inv_voxel = 1.0f / voxel */
    float origin[3];
    float mu;
    uint32_t max_weight;
} oslamk_volume;

/* The limits of a volume's side lengths, for every check of them: 16..512 voxels each, and the first mult8_axes of
 * nx, ny, nz multiples of 8 (0: the extraction; 1: the shift's quads of a row; 3: a volume as it is created) */
static inline int oslamk_sides_ok(unsigned nx, unsigned ny, unsigned nz, int mult8_axes)
{
    const unsigned n[3] = {nx, ny, nz};
    int a;
    for (a = 0; a < 3; a++)
        if (n[a] < 16u || n[a] > 512u || (a < mult8_axes && n[a] % 8u != 0u)) return 0;
    return 1;
}

/* rows of [R | t], float32 */
typedef struct oslamk_pose {
    float T[12];
} oslamk_pose;

/* one frame into the volume; T12 = rows of the inverse of T_vol_cam; *count (zeroed by the caller) += voxels updated */
int oslamk_tsdf_integrate(const oslamk_volume *vol, const oslamk_view *v, const float *T12, uint32_t *count, void *stream);
/* the volume seen from T12 = rows of T_vol_cam with the camera and size of *v (v->z is not read): z_out [w*h], maps
 * [w*h][8]; count[0] += pixels with a hit, count[1] += pixels with a normal (zeroed by the caller) */
int oslamk_tsdf_raycast(const oslamk_volume *vol, const oslamk_view *v, const float *T12, float *z_out, float *maps,
                        uint32_t *count, void *stream);
/* the records of a view's maps that have a normal, in row-major order, as device [n][6] (oslam_depth.hip: the flag,
 * scan and compact path of oslamk_depth_to_cloud); d_out6 = device [n_pix][6]; returns a hipError_t */
int oslamk_maps_to_cloud(const float *maps, size_t n_pix, float *d_out6, uint32_t *n_out, void *stream);

/* ---- surface extraction, of the whole surface and of what a shift loses (oslam_surface.hip; semantics in include/oslam.h
 * at oslam_volume_surface and oslam_volume_leaving) ---- */
#define OSLAMK_SURF_THREADS 256
#define OSLAMK_SURF_ITEMS 4           /* chunks of 256 consecutive voxels per workgroup */
#define OSLAMK_SURF_RUN (OSLAMK_SURF_THREADS * OSLAMK_SURF_ITEMS)   /* consecutive linear voxel indices a workgroup owns */

/* workgroups of the two passes: ceil(nx * ny * nz / OSLAMK_SURF_RUN), at most 2^17 */
uint32_t oslamk_surface_groups(const oslamk_volume *vol);
/* In both passes shift NULL means the whole surface; otherwise (three ints that pass oslamk_shift_ok) only the crossings
 * that a shift by it loses, over the same workgroups and in the same order.
 * first pass and scan: counts [n_groups] leaves as the exclusive offsets of the workgroups' points; totals[0] +=
 * crossings (zeroed by the caller), totals[1] = points */
int oslamk_surface_count(const oslamk_volume *vol, const int *shift, uint32_t min_weight, uint32_t n_groups, uint32_t *counts,
                         uint32_t *totals, void *stream);
/* second pass: out6 = device [n_points][6] (x y z nx ny nz), offsets and n_points as oslamk_surface_count left them */
int oslamk_surface_emit(const oslamk_volume *vol, const int *shift, uint32_t min_weight, uint32_t n_groups,
                        const uint32_t *offsets, uint32_t n_points, float *out6, void *stream);
/* the scan alone: counts [n] (n <= 2^17) becomes its exclusive prefix sums in place, *total_out = the sum */
int oslamk_surface_scan(uint32_t *counts, uint32_t n, uint32_t *total_out, void *stream);

/* ---- mesh extraction (oslam_mesh.hip; semantics in include/oslam.h at oslam_volume_mesh); workgroups and runs are the
 * surface extraction's, n_groups = oslamk_surface_groups(vol) ---- */
#define OSLAMK_MESH_T_CUBES 0         /* totals: full cubes with a case other than 0 and 255 (zeroed by the caller) */
#define OSLAMK_MESH_T_VERTS 1         /*         vertices */
#define OSLAMK_MESH_T_TRIS 2          /*         triangles */
#define OSLAMK_MESH_T_MISS 3          /*         triangle corners whose edge has no vertex (zeroed by the caller; stays 0) */
/* first pass and scans: vcounts and tcounts [n_groups] leave as the exclusive offsets of the workgroups' vertices and
 * triangles; totals [4] as above */
int oslamk_mesh_count(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, uint32_t *vcounts, uint32_t *tcounts,
                      uint32_t *totals, void *stream);
/* second pass: xyz [n_verts][3], nrm [n_verts][3] or NULL (the normals are then not computed), edge_id [n_verts] =
 * 3 * voxel + axis of each vertex, ascending */
int oslamk_mesh_vertices(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, const uint32_t *voffsets,
                         uint32_t n_verts, float *xyz, float *nrm, uint32_t *edge_id, void *stream);
/* third pass: tri [n_tris][3] vertex indices, found by binary search in edge_id; totals[OSLAMK_MESH_T_MISS] += misses */
int oslamk_mesh_triangles(const oslamk_volume *vol, uint32_t min_weight, uint32_t n_groups, const uint32_t *toffsets,
                          uint32_t n_tris, const uint32_t *edge_id, uint32_t n_verts, uint32_t *tri, uint32_t *totals,
                          void *stream);

/* ---- the shifting window: the limit of a shift, and the copy (oslam_shift.hip; semantics in include/oslam.h at
 * oslam_volume_shift).  What a shift loses of the surface is the surface extraction's, above ---- */
#define OSLAMK_SHIFT_MAX (1 << 20)    /* the largest shift, and the largest window offset, per axis in voxels: exact as a float */
/* a shift as the kernels take it, by value */
typedef struct oslamk_shift3 {
    int s[3];
} oslamk_shift3;
/* the limit of a shift triple, and of a window offset, for every check of it */
static inline int oslamk_shift_ok(const int s[3])
{
    int a;
    for (a = 0; a < 3; a++)
        if (s[a] < -OSLAMK_SHIFT_MAX || s[a] > OSLAMK_SHIFT_MAX) return 0;
    return 1;
}
/* dst [nx*ny*nz] (not vol->words) gets vol's words moved by shift, zeros where no source voxel exists; *kept (zeroed by
 * the caller) += the words of dst with w > 0.  vol->words is only read: the caller swaps the two buffers */
int oslamk_tsdf_shift(const oslamk_volume *vol, uint32_t *dst, const int shift[3], uint32_t *kept, void *stream);

/* ---- the voxels a shift moves out, as records for the voxel store, and the store's records back into the window
 * (oslam_reload.hip; semantics in include/oslam.h at oslam_volume_shift_world).  A record is two words: the linear index
 * lin = (k * ny + j) * nx + i, then the voxel's word ---- */
#define OSLAMK_PACK_THREADS 256
#define OSLAMK_PACK_ITEMS 4           /* chunks of 256 consecutive voxels per workgroup */
#define OSLAMK_PACK_RUN (OSLAMK_PACK_THREADS * OSLAMK_PACK_ITEMS)   /* consecutive linear voxel indices a workgroup owns */
/* workgroups of the two passes: ceil(nx * ny * nz / OSLAMK_PACK_RUN), at most 2^17 */
uint32_t oslamk_pack_groups(const oslamk_volume *vol);
/* first pass and scan: counts [n_groups] leaves as the exclusive offsets of the workgroups' records, *total_out = the
 * voxels with w > 0 that lie outside the window after the shift */
int oslamk_tsdf_pack_count(const oslamk_volume *vol, const int shift[3], uint32_t n_groups, uint32_t *counts, uint32_t *total_out,
                           void *stream);
/* second pass: rec_out = device [n_rec][2] (8-byte aligned), ascending lin; offsets and n_rec as the first pass left them */
int oslamk_tsdf_pack_emit(const oslamk_volume *vol, const int shift[3], uint32_t n_groups, const uint32_t *offsets, uint32_t n_rec,
                          uint32_t *rec_out, void *stream);
/* dst[lin] = word for each of the n_rec records of recs = device [n_rec][2] (8-byte aligned, distinct lin, n_rec at most
 * nx * ny * nz); a record whose lin is not below nx * ny * nz is skipped */
int oslamk_tsdf_unpack(uint32_t *dst, int nx, int ny, int nz, const uint32_t *recs, uint32_t n_rec, void *stream);
/* the colour words next to those records, through a colour store (oslam_reload_colour.hip): colours_out[r] =
 * colours[lin of record r] behind oslamk_tsdf_pack_emit, and dst[lin of record r] = colours_in[r] behind the colour
 * buffer's oslamk_tsdf_shift.  recs as above, colours_out / colours_in = device [n_rec]; a lin not below nx * ny * nz
 * reads as 0 and writes nothing */
int oslamk_pack_colours(const uint32_t *colours, int nx, int ny, int nz, const uint32_t *recs, uint32_t n_rec, uint32_t *colours_out,
                        void *stream);
int oslamk_unpack_colours(uint32_t *dst, int nx, int ny, int nz, const uint32_t *recs, const uint32_t *colours_in, uint32_t n_rec,
                          void *stream);

/* ---- the colour volume (oslam_colour.hip; semantics in include/oslam.h at oslam_volume_integrate_colour,
 * oslam_volume_colours and oslam_volume_paint_view).  A voxel's colour word is r | g << 8 | b << 16 | wc << 24, an image's
 * r | g << 8 | b << 16 | a << 24 with a = 255 or 0 ---- */
/* the colour buffer of a volume: one word per voxel in the volume's order, and the rule's two parameters */
typedef struct oslamk_colour {
    uint32_t *words;
    float band;                /* metres, 0 < band <= mu */
    uint32_t max_weight;       /* 1..255 */
} oslamk_colour;
/* the colour pass of one frame: rgba = the colour image that goes with v's z image ([h][w] words); T12 = rows of the
 * inverse of T_vol_cam; *count (zeroed by the caller) += voxels coloured */
int oslamk_tsdf_colour(const oslamk_volume *vol, const oslamk_colour *col, const oslamk_view *v, const uint32_t *rgba,
                       const float *T12, uint32_t *count, void *stream);
/* out[t] = the image word of the colour at the volume-frame point xyz[t] (device [n][3], n > 0), 0 without a colour; words =
 * the volume's colour buffer; *count (zeroed by the caller) += points with a colour */
int oslamk_colour_points(const oslamk_volume *vol, const uint32_t *words, const float *xyz, uint32_t n, uint32_t *out,
                         uint32_t *count, void *stream);
/* out [h][w] = the image word of the colour at every pixel of v with z > 0, seen from T12 = rows of T_vol_cam, 0 elsewhere;
 * *count (zeroed by the caller) += pixels with a colour */
int oslamk_colour_view(const oslamk_volume *vol, const uint32_t *words, const oslamk_view *v, const float *T12, uint32_t *out,
                       uint32_t *count, void *stream);

/* ---- the surface of the whole map, voxel store plus window, from sparse bricks (oslam_world_surface.hip; semantics in
 * include/oslam.h at oslam_world_surface; host side: oslam_world_surface.c) ---- */
#define OSLAMK_BRICK_SIDE 8
#define OSLAMK_BRICK_WORDS 512        /* [z][y][x] */
#define OSLAMK_BRICK_BIAS (1 << 20)   /* a brick coordinate floor(g / 8) lies in [-2^20, 2^20): 21 bits with this added */
#define OSLAMK_BRICK_MAX (1u << 22)   /* the most bricks of one map */
#define OSLAMK_BRICK_SCAN (1u << 17)  /* the most counters one run of oslamk_surface_scan takes: the counts are scanned in
                                         chunks of this many, and a chunk's base is added by the second pass */
#define OSLAMK_BRICK_CHUNKS (OSLAMK_BRICK_MAX / OSLAMK_BRICK_SCAN)
/* the packed key of brick (bx, by, bz): ascending keys are ascending (bz, by, bx).  A macro: host and device use it */
#define OSLAMK_BRICK_KEY(bx, by, bz)                                                                                       \
    ((uint64_t)(uint32_t)((bz) + OSLAMK_BRICK_BIAS) << 42 | (uint64_t)(uint32_t)((by) + OSLAMK_BRICK_BIAS) << 21 |           \
     (uint64_t)(uint32_t)((bx) + OSLAMK_BRICK_BIAS))
/* the map on the device: n table entries (keys ascending and distinct; slots[e] < n is entry e's brick in words
 * [n][512]) and the frame: voxel index r = g - anchor, origin = the window origin at offset anchor */
typedef struct oslamk_brick_map {
    const uint64_t *keys;
    const uint32_t *slots;
    uint32_t *words;
    uint32_t n;
    int anchor[3];
    float origin[3];
    float voxel, inv_voxel;
} oslamk_brick_map;
/* the bases the second pass adds to the scanned offsets: base[c] for the entries c * 2^17 .. */
typedef struct oslamk_brick_bases {
    uint32_t base[OSLAMK_BRICK_CHUNKS];
} oslamk_brick_bases;
/* writes the window's words (vol, at offset off[3]) into the bricks the window's box overlaps, voxel by voxel; the bricks
 * kb0 .. kb0 + nb - 1 per axis, each of which has a table entry */
int oslamk_brick_window(const oslamk_brick_map *map, const oslamk_volume *vol, const int off[3], const int kb0[3], const int nb[3],
                        void *stream);
/* first pass and scans: counts [map->n] leaves as the exclusive offsets of the entries' points inside each chunk of
 * 2^17 entries; totals[0] += crossings (zeroed by the caller), totals[2 + c] = the points of chunk c */
int oslamk_brick_count(const oslamk_brick_map *map, uint32_t min_weight, uint32_t *counts, uint32_t *totals, void *stream);
/* second pass: out6 = device [n_points][6] (x y z nx ny nz), key_out = device [n_points][4] (g_x g_y g_z axis) or NULL */
int oslamk_brick_emit(const oslamk_brick_map *map, uint32_t min_weight, const uint32_t *offsets, const oslamk_brick_bases *bases,
                      uint32_t n_points, float *out6, int32_t *key_out, void *stream);

/* ---- the colour at points of the whole map (oslam_world_colour.hip; semantics in include/oslam.h at oslam_world_colours;
 * host side: oslam_world_colour.c).  The map is the surface's with the brick array holding colour words ---- */
/* out[t] = the image word of the colour at the volume-frame point xyz[t] (device [n][3], 0 < n < 2^31), 0 without a colour;
 * *count (zeroed by the caller) += points with a colour */
int oslamk_brick_colours(const oslamk_brick_map *map, const float *xyz, uint32_t n, uint32_t *out, uint32_t *count, void *stream);
/* oslamk_colour_view against the map: out [h][w] = the image word of the colour at every pixel of v with z > 0, seen from
 * T12 = rows of T_vol_cam, 0 elsewhere; *count (zeroed by the caller) += pixels with a colour */
int oslamk_brick_colour_view(const oslamk_brick_map *map, const oslamk_view *v, const float *T12, uint32_t *out, uint32_t *count,
                             void *stream);

/* ---- the whole map ray-cast back into a view (oslam_world_raycast.hip; semantics in include/oslam.h at
 * oslam_world_raycast; host side: oslam_world_raycast.c).  The map is the surface's, TSDF words in the bricks ---- */
#define OSLAMK_WRAY_MAX_STEPS 65536   /* samples of one ray at most; the host refuses a (z_max - z_min) / step that reaches it */
/* the box of the slab test as voxel indices r = g - anchor (hi exclusive, hi - lo >= 2 per axis), and the truncation mu */
typedef struct oslamk_wray {
    int r_lo[3], r_hi[3];
    float mu;
} oslamk_wray;
/* oslamk_tsdf_raycast against the map: z_out [w*h], maps [w*h][8]; count[0] += pixels with a hit, count[1] += pixels with
 * a normal (zeroed by the caller) */
int oslamk_brick_raycast(const oslamk_brick_map *map, const oslamk_wray *box, const oslamk_view *v, const float *T12, float *z_out,
                         float *maps, uint32_t *count, void *stream);

/* ---- the mesh of the whole map from the same bricks (oslam_world_mesh.hip; semantics in include/oslam.h at
 * oslam_world_mesh; host side: oslam_world_mesh.c).  The map is the surface's, window written in by oslamk_brick_window ---- */
/* first pass and scans: vcounts and tcounts [map->n] leave as the exclusive offsets of the entries' vertices and triangles
 * inside each chunk of 2^17 entries, vsums[c] and tsums[c] = the sums of chunk c (device, OSLAMK_BRICK_CHUNKS each);
 * totals[OSLAMK_MESH_T_CUBES] += full cubes with a case other than 0 and 255 (zeroed by the caller) */
int oslamk_brick_mesh_count(const oslamk_brick_map *map, uint32_t min_weight, uint32_t *vcounts, uint32_t *tcounts, uint32_t *totals,
                            uint32_t *vsums, uint32_t *tsums, void *stream);
/* second pass: xyz [n_verts][3], nrm [n_verts][3] or NULL (the normals are then not computed), key_out [n_verts][4] (g_x g_y
 * g_z axis, 16-byte aligned) or NULL, edge_id [n_verts] = 3 * (voxel in its brick) + axis, ascending inside an entry */
int oslamk_brick_mesh_vertices(const oslamk_brick_map *map, uint32_t min_weight, const uint32_t *voffsets,
                               const oslamk_brick_bases *vbases, uint32_t n_verts, float *xyz, float *nrm, int32_t *key_out,
                               uint32_t *edge_id, void *stream);
/* third pass: tri [n_tris][3] vertex indices, found by binary search in the run of edge_id that belongs to the entry of the
 * edge's start voxel; totals[OSLAMK_MESH_T_MISS] += misses (zeroed by the caller; stays 0) */
int oslamk_brick_mesh_triangles(const oslamk_brick_map *map, uint32_t min_weight, const uint32_t *toffsets,
                                const oslamk_brick_bases *tbases, uint32_t n_tris, const uint32_t *voffsets,
                                const oslamk_brick_bases *vbases, const uint32_t *edge_id, uint32_t n_verts, uint32_t *tri,
                                uint32_t *totals, void *stream);

#ifdef __cplusplus
}
#endif
#endif
