/*
 * oslam_window.c -- the moving window of a TSDF volume, host side (include/oslam.h at oslam_volume_shift and
 * oslam_volume_shift_world).  oslam_volume_shift moves the window of voxels the volume holds (k_tsdf_shift of
 * oslam_shift.hip into a second buffer, then a swap of the two); oslam_volume_shift_world makes the same move through a
 * voxel store that keeps what leaves and gives back what returns (the store: oslam_world.c; kernels: oslam_reload.hip and
 * oslam_reload_colour.hip).  Both are one body, shift_window, whose store may be NULL; a coloured volume's colour buffer
 * moves with every shift.  oslam_volume_pack taps the pack, oslam_volume_follow decides a move on the host.  The window's
 * arithmetic and the layout of a batch of records are oslam_window.h's; the volume itself, its lock and the fusion are
 * oslam_volume.c's; the limits of a shift are oslam_kernels.h's.
 */
#include <math.h>

#include "oslam_internal.h"
#include "oslam_window.h"
#include "oslam_world.h"

/* the second buffers a shift needs, with the volume lock held and the volume's device bound: the TSDF's and, on a coloured
 * volume, the colours'.  Both exist afterwards or the call fails before anything moved */
static int shift_spares(oslam_volume *vol)
{
    uint32_t **want[2] = {&vol->spare, vol->colour.words ? &vol->colour_spare : NULL};
    int b;
    for (b = 0; b < 2; b++) {
        if (!want[b] || *want[b]) continue;
        if (hipMalloc((void **)want[b], oslam_volume_bytes(&vol->p)) != hipSuccess) {
            (void)hipGetLastError();
            *want[b] = NULL;
            return fail(OSLAM_E_NOMEM, "no device memory for the second buffer of the shift");
        }
    }
    return OSLAM_OK;
}

/* the colours of a coloured volume moved as k_tsdf_shift moves words, into colour_spare: launched behind the TSDF's shift;
 * scratch = a zeroed counter for the kernel's count, which nobody reads.  The commit swaps after the wait */
static int shift_colours(const oslam_volume *vol, const int shift[3], uint32_t *scratch, void *stream)
{
    oslamk_volume k = vol->k;
    k.words = vol->colour.words;
    return oslamk_tsdf_shift(&k, vol->colour_spare, shift, scratch, stream);
}

int oslam_world_params_of(const oslam_volume *vol, oslam_world_params *p)
{
    if (!vol || !p) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(p, 0, sizeof *p);
    p->voxel = vol->p.voxel;
    memcpy(p->origin0, vol->p.origin, sizeof p->origin0);
    return OSLAM_OK;
}

/* The two passes of the pack, with the volume lock held and the volume's device bound: *n_rec = the seen voxels that
 * leave under shift; at most cap of them are packed, into *d_rec = a batch of records on the device (NULL otherwise),
 * coloured with colours (the volume's colour buffer, or NULL), which are gathered behind the second pass.  One host wait,
 * for the total; the second pass is only launched.  The caller frees *d_cnt and *d_rec after its own wait */
static int pack_leaving(oslam_volume *vol, const int shift[3], size_t cap, const uint32_t *colours, uint32_t **d_cnt, uint32_t **d_rec,
                        uint32_t *n_rec, uint32_t *launches)
{
    int rc = OSLAM_OK;
    const uint32_t n_groups = oslamk_pack_groups(&vol->k);
    void *stream = oslam_stream();
    *n_rec = 0;
    KCHK(oslam_counters_open(d_cnt, n_groups, stream));            /* the total in the first 256 bytes, then one counter per workgroup */
    KCHK(oslamk_tsdf_pack_count(&vol->k, shift, n_groups, *d_cnt + 64, *d_cnt, stream));
    *launches += 2;
    HIPCHK(hipMemcpyAsync(n_rec, *d_cnt, sizeof *n_rec, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (*n_rec > 0 && (size_t)*n_rec <= cap) {
        KCHK(oslam_dev_alloc((void **)d_rec, oslam_records_bytes(*n_rec, colours != NULL)));
        KCHK(oslamk_tsdf_pack_emit(&vol->k, shift, n_groups, *d_cnt + 64, *n_rec, *d_rec, stream));
        *launches += 1;
        if (colours) {
            KCHK(oslamk_pack_colours(colours, vol->k.nx, vol->k.ny, vol->k.nz, *d_rec, *n_rec, *d_rec + oslam_records_colours(*n_rec), stream));
            *launches += 1;
        }
    }
done:
    return rc;
}

static void stage_release(void *p) { (void)hipHostFree(p); }

/* a pinned staging buffer of the store with room for bytes: grown by half as much again, so a stream of similar shifts
 * allocates once (oslam_world_surface.c stages the store's bricks through it too) */
int oslam_world_stage_fit(oslam_world_stage *st, size_t bytes)
{
    void *p = NULL;
    const size_t want = bytes + bytes / 2;
    if (st->bytes >= bytes) return OSLAM_OK;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(OSLAM_E_NOMEM, "no pinned host memory for the records of the shift");
    }
    if (st->p) st->release(st->p);
    st->p = p;
    st->bytes = want;
    st->release = stage_release;
    return OSLAM_OK;
}

/* ---- one shift, with a store or without (w == NULL): the state of the call, then its steps in order ---- */
typedef struct shift_run {
    oslam_volume *vol;
    oslam_world *w;
    const int *shift;
    void *stream;
    unsigned n[3];                                                  /* the window's sides */
    int off[3];                                                     /* its offset after the shift */
    int cs;                                                         /* the store keeps colour: a record crosses the host link as 12 bytes, not 8 */
    uint32_t *d_cnt, *d_out;                                        /* device: the pack's counters, the batch that leaves */
    uint32_t *d_in, *d_kept;                                        /* the batch that enters; {kept, the colour shift's count, which nobody reads} */
    const uint32_t *rec_out;                                        /* host: the batch that leaves (the store's stage 0) */
    uint32_t *rec_in;                                               /* the batch that enters (stage 1), n_read of its n_in records filled */
    uint32_t n_out, kept, launches;
    size_t n_in, n_read;
    int nb;                                                         /* the entering region as boxes */
    int32_t lo[7][3], hi[7][3];
    size_t mark;                                                    /* of the store, before the first brick was reserved */
    int locked, reserved;                                           /* taken so far: the store's lock, the mark */
} shift_run;

/* offsets, compatibility, the colour rule, the zero shift, device and spares; *moves = there is a shift to make */
static int shift_begin(shift_run *s, oslam_reload_result *res, int *moves)
{
    const oslam_volume *vol = s->vol;
    int a;
    for (a = 0; a < 3; a++) s->off[a] = vol->off[a] + s->shift[a];
    if (!oslamk_shift_ok(s->off)) return fail(OSLAM_E_INVALID, "the window's offset is at most 2^20 voxels");
    if (s->w && !oslam_world_compatible(s->w, vol->p.voxel, vol->p.origin))
        return fail(OSLAM_E_INVALID, "the voxel store was made for another voxel size or origin");
    s->cs = s->w && oslam_world_coloured(s->w);                     /* fixed when the store was created */
    if (s->cs && !vol->colour.words) return fail(OSLAM_E_INVALID, "a colour store needs a volume with colour");
    if (res) memset(res, 0, sizeof *res);
    *moves = (s->shift[0] | s->shift[1] | s->shift[2]) != 0;
    if (!*moves) {
        if (res) memcpy(res->offset, s->off, sizeof s->off);
        return OSLAM_OK;
    }
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    return shift_spares(s->vol);
}

/* pack what leaves, with its colours for a colour store, take the store's lock and bring the batch down */
static int shift_pack(shift_run *s)
{
    int rc;
    size_t bytes;
    oslam_world_stage *st;
    rc = pack_leaving(s->vol, s->shift, (size_t)-1, s->cs ? s->vol->colour.words : NULL, &s->d_cnt, &s->d_out, &s->n_out, &s->launches);
    if (rc != OSLAM_OK) return rc;
    oslam_world_lock(s->w);
    s->locked = 1;
    if (!s->n_out) return OSLAM_OK;
    st = oslam_world_stages(s->w);
    bytes = oslam_records_bytes(s->n_out, s->cs);
    rc = oslam_world_stage_fit(&st[0], bytes);
    if (rc != OSLAM_OK) return rc;
    HIPCHK(hipMemcpyAsync(st[0].p, s->d_out, bytes, hipMemcpyDeviceToHost, (hipStream_t)s->stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)s->stream));
    s->rec_out = (const uint32_t *)st[0].p;
done:
    return rc;
}

/* the bricks the leaving records need, still empty: from here on a failure rolls the store back to the mark */
static int shift_reserve(shift_run *s)
{
    int rc = OSLAM_OK;
    uint32_t r;
    int32_t g[3];
    s->mark = oslam_world_mark(s->w);
    s->reserved = 1;
    for (r = 0; r < s->n_out && rc == OSLAM_OK; r++) {
        oslam_window_global(s->n, s->vol->off, s->rec_out[2 * r], g);
        rc = oslam_world_reserve(s->w, g);
    }
    return rc;
}

/* one stored word of the entering region, as the next record of the batch: its linear index in the new window */
static void enter_record(void *ctx, const int32_t g[3], uint32_t word, uint32_t colour)
{
    shift_run *s = (shift_run *)ctx;
    s->rec_in[2 * s->n_read] = oslam_window_lin(s->n, s->off, g);
    s->rec_in[2 * s->n_read + 1] = word;
    if (s->cs) s->rec_in[oslam_records_colours(s->n_in) + s->n_read] = colour;
    s->n_read++;
}

/* the entering records: counted, then read into the store's stage 1, which does not change the store, and sent up */
static int shift_enter(shift_run *s)
{
    int rc = OSLAM_OK, b;
    size_t bytes;
    oslam_world_stage *st = oslam_world_stages(s->w);
    s->nb = oslam_window_entering(s->vol->off, s->off, s->n, s->lo, s->hi);
    for (b = 0; b < s->nb; b++) s->n_in += oslam_world_visit(s->w, s->lo[b], s->hi[b], 0, NULL, NULL);
    if (!s->n_in) return OSLAM_OK;
    bytes = oslam_records_bytes(s->n_in, s->cs);
    rc = oslam_world_stage_fit(&st[1], bytes);
    if (rc != OSLAM_OK) return rc;
    s->rec_in = (uint32_t *)st[1].p;
    for (b = 0; b < s->nb; b++) (void)oslam_world_visit_colour(s->w, s->lo[b], s->hi[b], 0, enter_record, s);
    KCHK(oslam_dev_alloc((void **)&s->d_in, bytes));
    HIPCHK(hipMemcpyAsync(s->d_in, s->rec_in, bytes, hipMemcpyHostToDevice, (hipStream_t)s->stream));
done:
    return rc;
}

/* shift, colour shift, unpack colours and unpack in stream order into the second buffers, then kept on its way down */
static int shift_launch(shift_run *s)
{
    int rc = OSLAM_OK;
    const oslam_volume *vol = s->vol;
    KCHK(oslam_counters_open(&s->d_kept, 0, s->stream));
    KCHK(oslamk_tsdf_shift(&vol->k, vol->spare, s->shift, s->d_kept, s->stream));
    s->launches++;
    if (vol->colour.words) {                                        /* a plain store keeps no colour: what it reloads has wc = 0 */
        KCHK(shift_colours(vol, s->shift, s->d_kept + 1, s->stream));
        s->launches++;
        if (s->cs && s->n_in) {                                     /* a colour store's colours, into the buffer that shift wrote */
            KCHK(oslamk_unpack_colours(vol->colour_spare, vol->k.nx, vol->k.ny, vol->k.nz, s->d_in, s->d_in + oslam_records_colours(s->n_in),
                                       (uint32_t)s->n_in, s->stream));
            s->launches++;
        }
    }
    if (s->n_in) {
        KCHK(oslamk_tsdf_unpack(vol->spare, vol->k.nx, vol->k.ny, vol->k.nz, s->d_in, (uint32_t)s->n_in, s->stream));
        s->launches++;
    }
    HIPCHK(hipMemcpyAsync(&s->kept, s->d_kept, sizeof s->kept, hipMemcpyDeviceToHost, (hipStream_t)s->stream));
done:
    return rc;
}

/* The commit, after the wait: the only place that swaps the buffers and writes vol->off and k.origin, for a shift with a
 * store and without.  Nothing here can fail: the leaving records' bricks exist (shift_reserve) */
static void shift_commit(shift_run *s, oslam_reload_result *res)
{
    oslam_volume *vol = s->vol;
    const uint32_t *col_out = s->cs && s->rec_out ? s->rec_out + oslam_records_colours(s->n_out) : NULL;
    uint32_t *t, r;
    int32_t g[3];
    int b;
    for (r = 0; r < s->n_out; r++) {                                /* n_out and nb are 0 without a store */
        oslam_window_global(s->n, vol->off, s->rec_out[2 * r], g);
        oslam_world_store_colour(s->w, g, s->rec_out[2 * r + 1], col_out ? col_out[r] : 0u);
    }
    for (b = 0; b < s->nb; b++) (void)oslam_world_visit(s->w, s->lo[b], s->hi[b], 1, NULL, NULL);
    s->reserved = 0;
    t = vol->spare;
    vol->spare = vol->k.words;
    vol->k.words = t;
    if (vol->colour.words) {
        t = vol->colour.words;
        vol->colour.words = vol->colour_spare;
        vol->colour_spare = t;
    }
    memcpy(vol->off, s->off, sizeof s->off);
    oslam_window_origin(vol->p.origin, vol->p.voxel, vol->off, vol->k.origin);
    if (res) {
        memcpy(res->offset, s->off, sizeof s->off);
        res->kept = s->kept + (uint32_t)s->n_in;                    /* the reloaded words are seen and their voxels were 0 */
        res->stored = s->n_out;
        res->reloaded = (uint32_t)s->n_in;
        res->launches = s->launches;
    }
}

/* oslam_volume_shift (w == NULL) and oslam_volume_shift_world after their NULL checks.  res is zeroed once the offset,
 * the store and the colour rule have passed.  Lock order: the volume lock, then the store's, taken after the pack's wait */
static int shift_window(oslam_volume *vol, oslam_world *w, const int shift[3], oslam_reload_result *res)
{
    int rc, moves = 0;
    const double t0 = now_ms();
    shift_run s = {.vol = vol, .w = w, .shift = shift, .stream = oslam_stream(), .n = {vol->p.nx, vol->p.ny, vol->p.nz}};
    if (!oslamk_shift_ok(shift)) return fail(OSLAM_E_INVALID, "a shift is at most 2^20 voxels");
    oslam_volume_lock();
    rc = shift_begin(&s, res, &moves);
    if (rc == OSLAM_OK && moves && w) {
        rc = shift_pack(&s);
        if (rc == OSLAM_OK) rc = shift_reserve(&s);
        if (rc == OSLAM_OK) rc = shift_enter(&s);
    }
    if (rc != OSLAM_OK || !moves) goto done;
    rc = shift_launch(&s);
    if (rc != OSLAM_OK) goto done;
    HIPCHK(hipStreamSynchronize((hipStream_t)s.stream));
    shift_commit(&s, res);
done:
    /* whatever was enqueued has run before a block is freed; the store goes back to its mark; window, offset and origin
     * were not written */
    if (rc != OSLAM_OK && (s.d_cnt || s.d_kept)) (void)hipStreamSynchronize((hipStream_t)s.stream);
    if (s.reserved) oslam_world_rollback(w, s.mark);
    if (s.locked) oslam_world_unlock(w);
    oslam_volume_unlock();
    if (s.d_kept) oslam_dev_free(s.d_kept);
    if (s.d_in) oslam_dev_free(s.d_in);
    if (s.d_out) oslam_dev_free(s.d_out);
    if (s.d_cnt) oslam_dev_free(s.d_cnt);
    if (rc == OSLAM_OK && res) res->ms_total = (float)(now_ms() - t0);
    return rc;
}

int oslam_volume_shift(oslam_volume *vol, const int shift[3], oslam_shift_result *res)
{
    int rc;
    oslam_reload_result r;
    if (!vol || !shift) return fail(OSLAM_E_INVALID, "NULL argument");
    if (res) {                                                      /* r starts as *res: a call refused before the body zeroes its result leaves *res as it was */
        memcpy(r.offset, res->offset, sizeof r.offset);
        r.kept = res->kept;
        r.launches = res->launches;
        r.ms_total = res->ms_total;
    }
    rc = shift_window(vol, NULL, shift, res ? &r : NULL);
    if (res) {
        memcpy(res->offset, r.offset, sizeof r.offset);
        res->kept = r.kept;
        res->launches = r.launches;
        res->ms_total = r.ms_total;
    }
    return rc;
}

int oslam_volume_shift_world(oslam_volume *vol, oslam_world *w, const int shift[3], oslam_reload_result *res)
{
    if (!vol || !w || !shift) return fail(OSLAM_E_INVALID, "NULL argument");
    return shift_window(vol, w, shift, res);
}

/* the tap of the pack, without colours (colour_out == NULL, want_colour == 0) or with them */
static int pack_tap(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, uint32_t *colour_out, int want_colour,
                    size_t cap, size_t *n_out)
{
    int rc = OSLAM_OK;
    uint32_t *d_cnt = NULL, *d_rec = NULL, *h = NULL, n = 0, launches = 0, r;
    if (!vol || !shift || !n_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (cap != 0 && (!lin_out || !word_out || (want_colour && !colour_out)))
        return fail(OSLAM_E_INVALID, "the outputs must be given with cap != 0");
    if (want_colour && !vol->colour.words) return fail(OSLAM_E_INVALID, "the volume has no colour");
    if (!oslamk_shift_ok(shift)) return fail(OSLAM_E_INVALID, "a shift is at most 2^20 voxels");
    *n_out = 0;
    if (!(shift[0] | shift[1] | shift[2])) return OSLAM_OK;
    if (hipSetDevice(vol->dev) != hipSuccess) return fail(OSLAM_E_DEVICE, "hipSetDevice failed");
    oslam_volume_lock();
    rc = pack_leaving(vol, shift, cap, want_colour ? vol->colour.words : NULL, &d_cnt, &d_rec, &n, &launches);
    if (rc != OSLAM_OK) goto done;
    *n_out = n;
    if (cap != 0 && (size_t)n > cap) { rc = fail(OSLAM_E_LIMIT, "output capacity too small"); goto done; }
    if (d_rec) {
        h = (uint32_t *)malloc(oslam_records_bytes(n, want_colour));
        if (!h) { rc = fail(OSLAM_E_NOMEM, "host allocation failed"); goto done; }
        HIPCHK(hipMemcpy(h, d_rec, oslam_records_bytes(n, want_colour), hipMemcpyDeviceToHost));
        for (r = 0; r < n; r++) {
            lin_out[r] = h[2 * r];
            word_out[r] = h[2 * r + 1];
            if (want_colour) colour_out[r] = h[oslam_records_colours(n) + r];
        }
    }
done:
    if (d_cnt) (void)hipStreamSynchronize((hipStream_t)oslam_stream());
    oslam_volume_unlock();
    free(h);
    if (d_rec) oslam_dev_free(d_rec);
    if (d_cnt) oslam_dev_free(d_cnt);
    return rc;
}

int oslam_volume_pack(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, size_t cap, size_t *n_out)
{
    return pack_tap(vol, shift, lin_out, word_out, NULL, 0, cap, n_out);
}

int oslam_volume_pack_colour(oslam_volume *vol, const int shift[3], uint32_t *lin_out, uint32_t *word_out, uint32_t *colour_out,
                             size_t cap, size_t *n_out)
{
    return pack_tap(vol, shift, lin_out, word_out, colour_out, 1, cap, n_out);
}

int oslam_volume_window(oslam_volume *vol, int offset_out[3], float origin_out[3])
{
    if (!vol || !offset_out || !origin_out) return fail(OSLAM_E_INVALID, "NULL argument");
    oslam_volume_lock();
    memcpy(offset_out, vol->off, sizeof vol->off);
    memcpy(origin_out, vol->k.origin, sizeof vol->k.origin);
    oslam_volume_unlock();
    return OSLAM_OK;
}

int oslam_follow_params_default(const oslam_volume *vol, oslam_follow_params *fp)
{
    unsigned n_min;
    if (!vol || !fp) return fail(OSLAM_E_INVALID, "NULL argument");
    memset(fp, 0, sizeof *fp);
    n_min = vol->p.nx < vol->p.ny ? vol->p.nx : vol->p.ny;
    if (vol->p.nz < n_min) n_min = vol->p.nz;
    fp->lookahead = (float)(0.5 * (double)vol->p.nz * (double)vol->p.voxel);
    fp->threshold = (float)n_min / 4.0f;
    fp->granule = 8;
    return OSLAM_OK;
}

int oslam_volume_follow(oslam_volume *vol, const float T_vol_cam[16], const oslam_follow_params *fp, int shift_out[3])
{
    int rc, a, moved = 0;
    oslam_follow_params p;
    float origin[3];
    double d[3];
    if (!vol || !T_vol_cam || !shift_out) return fail(OSLAM_E_INVALID, "NULL argument");
    if (fp && (!isfinite(fp->lookahead) || !isfinite(fp->threshold) || !(fp->lookahead >= 0.0f) || !(fp->threshold >= 0.0f)))
        return fail(OSLAM_E_INVALID, "lookahead and threshold must be finite and not negative");
    if (fp && (fp->granule < 1 || fp->granule > 64)) return fail(OSLAM_E_INVALID, "granule must lie in 1..64");
    rc = oslam_refine_check_rigid(T_vol_cam);
    if (rc != OSLAM_OK) return rc;
    if (fp) p = *fp;
    else oslam_follow_params_default(vol, &p);
    oslam_volume_lock();
    memcpy(origin, vol->k.origin, sizeof origin);
    oslam_volume_unlock();
    {
        const unsigned n[3] = {vol->p.nx, vol->p.ny, vol->p.nz};
        const double h = (double)vol->p.voxel;
        for (a = 0; a < 3; a++) {
            const double c = (double)T_vol_cam[4 * a + 3] + (double)p.lookahead * (double)T_vol_cam[4 * a + 2];
            const double centre = (double)origin[a] + 0.5 * (double)n[a] * h;
            d[a] = (c - centre) / h;
            if (!(fabs(d[a]) <= (double)p.threshold)) moved = 1;
        }
        for (a = 0; a < 3; a++) {
            double s = moved ? (double)p.granule * rint(d[a] / (double)p.granule) : 0.0;
            if (s > (double)n[a]) s = (double)n[a];
            if (s < -(double)n[a]) s = -(double)n[a];
            shift_out[a] = (int)s;
        }
    }
    return OSLAM_OK;
}
