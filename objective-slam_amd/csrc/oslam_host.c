/*
 * oslam_host.c -- the C-ABI of include/oslam.h: host orchestration in C over
 * the gfx950 kernels of the .hip files beside it (oslam_kernels.h).  This file: what every stage shares
 * (oslam_internal.h); each stage has a file of its own beside it.
 *
 * Mirrors the reference's host layer (pcl/alignment/src/cuda/{ppf,model,scene}.cu)
 * with two structural differences: nothing N^2-sized is materialised, and a
 * model's table stays resident in HBM for as many scenes as the caller aligns
 * (the reference rebuilds scene and model per pair, ppf.cu:57-100).
 * There is no CPU fallback: every compute call needs the HIP device.
 */
#include <pthread.h>
#include <stdio.h>

#include "oslam_internal.h"

static __thread char g_err[512];
static __thread void *g_stream;

const char *oslam_last_error(void) { return g_err; }

int oslam_set_stream(void *hip_stream)
{
    g_stream = hip_stream;
    return OSLAM_OK;
}

void *oslam_stream(void) { return g_stream; }

int oslam_fail(int code, const char *what)
{
    if (what != g_err) snprintf(g_err, sizeof g_err, "%s", what);
    return code;
}

int oslam_fail_call(const char *call, int err, const char *file, int line)
{
    snprintf(g_err, sizeof g_err, "%s: %s (%s:%d)", call, hipGetErrorString((hipError_t)err), file, line);
    return OSLAM_E_DEVICE;
}

/* ------------------------------------------------------------------------ */
int oslam_params_default(oslam_params *p)
{
    if (!p) return fail(OSLAM_E_INVALID, "params is NULL");
    memset(p, 0, sizeof *p);
    p->ref_point_df = 1;              /* alignment.cpp:134 */
    p->vote_count_threshold = 0.4f;   /* alignment.cpp:136 */
    p->cpu_clustering = 0;
    p->use_l1_norm = 0;
    p->use_averaged_clusters = 0;
    p->dev = 0;
    p->vote_mode = OSLAM_VOTE_EXACT;
    p->shard_rank = 0;
    p->shard_world = 1;
    p->max_cells = 1u << 22;
    p->pose_gpu_min = 0;              /* 0 = default (4096 records) */
    p->no_bucket_spread = 0;
    p->scratch_gib = 0;               /* 0 = default (4 GiB) */
    p->vote_order = 0;                /* largest first */
    return OSLAM_OK;
}

int oslam_d_dist_from_cloud(const float *xyz, size_t n, size_t stride_bytes, float tau_d,
                            float *d_dist_out)
{
    float lo[3], hi[3], ext;
    size_t i;
    int a;
    if (!xyz || !d_dist_out || n == 0 || stride_bytes < 12) return fail(OSLAM_E_INVALID, "bad cloud");
    for (a = 0; a < 3; a++) lo[a] = hi[a] = xyz[a];
    for (i = 1; i < n; i++) {
        const float *p = (const float *)((const char *)xyz + i * stride_bytes);
        for (a = 0; a < 3; a++) {
            if (p[a] < lo[a]) lo[a] = p[a];
            if (p[a] > hi[a]) hi[a] = p[a];
        }
    }
    ext = hi[0] - lo[0];
    if (hi[1] - lo[1] > ext) ext = hi[1] - lo[1];
    if (hi[2] - lo[2] > ext) ext = hi[2] - lo[2];
    *d_dist_out = tau_d * ext;        /* alignment.cpp:250-253 */
    return OSLAM_OK;
}

int oslam_pick_device(int dev_req, int *dev_out)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(OSLAM_E_DEVICE, "no HIP device available (the PPF path has no CPU fallback)");
    if (dev_req < 0) dev_req = 0;
    *dev_out = dev_req < n - 1 ? dev_req : n - 1;     /* ppf.cu:45 */
    e = hipSetDevice(*dev_out);
    if (e != hipSuccess) return fail(OSLAM_E_DEVICE, hipGetErrorString(e));
    return OSLAM_OK;
}

/* ---- kept device blocks of the scene path (oslam_kernels.h) ---- */
#define DEVCACHE_SLOTS 64
#define DEVCACHE_MAX_BLOCK ((size_t)1 << 30)        /* larger blocks go straight back to the driver */
typedef struct {
    void *p;
    size_t bytes;
    int dev, used;
} devblock;
static devblock g_devcache[DEVCACHE_SLOTS];
static pthread_mutex_t g_devcache_mu = PTHREAD_MUTEX_INITIALIZER;

int oslam_dev_alloc(void **out, size_t bytes)
{
    int dev = 0, i, best = -1, spare = -1;
    hipError_t e;
    size_t want;
    *out = NULL;
    if (bytes == 0) bytes = 16;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipErrorInvalidDevice;
    pthread_mutex_lock(&g_devcache_mu);
    for (i = 0; i < DEVCACHE_SLOTS; i++) {
        devblock *b = &g_devcache[i];
        if (!b->p) { if (spare < 0) spare = i; continue; }
        if (b->used || b->dev != dev || b->bytes < bytes || b->bytes > 2 * bytes + 65536) continue;
        if (best < 0 || b->bytes < g_devcache[best].bytes) best = i;
    }
    if (best >= 0) {
        g_devcache[best].used = 1;
        *out = g_devcache[best].p;
        pthread_mutex_unlock(&g_devcache_mu);
        return 0;
    }
    /* a frame's clouds differ by a few per cent from the last one's: head room lets the next frame reuse the block */
    want = bytes <= DEVCACHE_MAX_BLOCK ? bytes + bytes / 8 + 256 : bytes;
    e = hipMalloc(out, want);
    if (e != hipSuccess) {              /* out of memory with blocks kept: give them back and try once more */
        (void)hipGetLastError();
        for (i = 0; i < DEVCACHE_SLOTS; i++)
            if (g_devcache[i].p && !g_devcache[i].used && g_devcache[i].dev == dev) {
                (void)hipFree(g_devcache[i].p);
                memset(&g_devcache[i], 0, sizeof g_devcache[i]);
                if (spare < 0) spare = i;
            }
        want = bytes;
        e = hipMalloc(out, want);
    }
    if (e == hipSuccess && spare >= 0 && want <= DEVCACHE_MAX_BLOCK) {
        g_devcache[spare].p = *out;
        g_devcache[spare].bytes = want;
        g_devcache[spare].dev = dev;
        g_devcache[spare].used = 1;
    }
    pthread_mutex_unlock(&g_devcache_mu);
    return (int)e;
}

void oslam_dev_free(void *p)
{
    int i;
    if (!p) return;
    pthread_mutex_lock(&g_devcache_mu);
    for (i = 0; i < DEVCACHE_SLOTS; i++)
        if (g_devcache[i].p == p) {
            g_devcache[i].used = 0;
            pthread_mutex_unlock(&g_devcache_mu);
            return;
        }
    pthread_mutex_unlock(&g_devcache_mu);
    (void)hipFree(p);                   /* not one of the kept blocks (table full, or too large) */
}

void oslam_dev_cache_release(int dev)
{
    int i;
    pthread_mutex_lock(&g_devcache_mu);
    for (i = 0; i < DEVCACHE_SLOTS; i++)
        if (g_devcache[i].p && !g_devcache[i].used && g_devcache[i].dev == dev) {
            (void)hipFree(g_devcache[i].p);
            memset(&g_devcache[i], 0, sizeof g_devcache[i]);
        }
    pthread_mutex_unlock(&g_devcache_mu);
}
