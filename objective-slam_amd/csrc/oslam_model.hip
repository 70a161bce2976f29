/*
 * oslam_model.hip -- the model build of the PPF registration path (gfx950; host side: oslam_model.c, the group's key
 * numbers: oslam_db.c; the overview of the path is at the top of oslam_kernels.h).  Built with -ffp-contract=off: the
 * float sequences of ppf_core.h must round exactly as on the host.
 *
 * What the reference does with an N^2-sized key array and Thrust sorts (pcl/alignment/src/cuda/model.cu) is fused:
 *   k_model_count    pair key -> the open-addressing table of the reference point's slice (counts the buckets)
 *   k_table_scan     bucket lengths, padded to multiples of 4 entries -> bucket starts (one workgroup)
 *   k_union_build    the union table of the keys of all slices
 *   k_reach_build    the bitset of the distance bins that can reach a key
 *   k_union_weights  per union slot, the entries a hit on its key streams (the order of the key numbers)
 *   k_kmap_build     the key map (distance bin, three angle bins) -> key number
 *   k_uinfo_build    per slice, the bucket of every key number
 *   k_model_fill     the same pairs again, written into their buckets as 4-byte entries (no sort)
 *   k_bucket_spread  the entries ordered inside each bucket for the LDS banks of the vote
 *   k_bucket_psort   exact mode: every bucket a second time, ordered by position inside a bin, with its directory
 *   k_row_keys       parity tap: the keys of one reference row
 * Bounds: a thread checks its point or slot index against the cloud or the tables before it loads; a probe sequence is
 * masked to the table and ends after cap probes (overflow flag); a bucket is written inside [start, start + len) as
 * k_model_count counted it.  The resources are in profiles/r31_kernel_resources_split.txt.
 */
#include <hip/hip_runtime.h>

#include "oslam_kernels.h"
#include "ppf_core.h"

/* key of the ordered pair (r -> i) of one cloud; r's data is passed in registers */
__device__ __forceinline__ uint32_t cloud_pair_key(const oslamk_cloud &c, int i, float prx,
                                                   float pry, float prz, float nrx, float nry,
                                                   float nrz, float nrn, float d_dist,
                                                   float inv_d_dist, float *pix, float *piy,
                                                   float *piz)
{
    float px = c.px[i], py = c.py[i], pz = c.pz[i];
    float nx = c.nx[i], ny = c.ny[i], nz = c.nz[i];
    *pix = px;
    *piy = py;
    *piz = pz;
    return pc_pair_key(prx, pry, prz, nrx, nry, nrz, nrn, px, py, pz, nx, ny, nz,
                       pc_norm3(nx, ny, nz), d_dist, inv_d_dist);
}

/* --------------------------------------------------------------------------
 * parity tap: keys of one reference row (Scene::getHashKeys row, scene.cu:49-54)
 * ------------------------------------------------------------------------*/
__global__ void k_row_keys(oslamk_cloud c, int ref, float d_dist, float inv_d_dist,
                           uint32_t *keys_out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    float nrx = c.nx[ref], nry = c.ny[ref], nrz = c.nz[ref];
    float x, y, z;
    uint32_t k = 0;
    if (i != ref)
        k = cloud_pair_key(c, i, c.px[ref], c.py[ref], c.pz[ref], nrx, nry, nrz,
                           pc_norm3(nrx, nry, nrz), d_dist, inv_d_dist, &x, &y, &z);
    keys_out[i] = k;
}

/* --------------------------------------------------------------------------
 * model build
 * ------------------------------------------------------------------------*/
/* grid (ceil(M/256), M): blockIdx.y = m_r, x covers m_i.  Counts each pair in
 * the table of m_r's slice (Model ctor + ParallelHashArray, model.cu:43-82). */
__global__ void k_model_count(oslamk_cloud c, float d_dist, float inv_d_dist, oslamk_table t,
                              uint32_t *n_unique, uint32_t *overflow)
{
    int m_r = blockIdx.y;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n || i == m_r) return;
    float nrx = c.nx[m_r], nry = c.ny[m_r], nrz = c.nz[m_r];
    float x, y, z;
    uint32_t key = cloud_pair_key(c, i, c.px[m_r], c.py[m_r], c.pz[m_r], nrx, nry, nrz,
                                  pc_norm3(nrx, nry, nrz), d_dist, inv_d_dist, &x, &y, &z);
    if (key == 0) return;
    int slice = m_r / OSLAMK_SLICE;
    oslamk_slot *tab = t.slots + (size_t)slice * t.cap;
    uint32_t mask = t.cap - 1, slot = oslamk_slot_of(key, t.shift);
    for (uint32_t probe = 0; probe < t.cap; probe++) {
        uint32_t old = atomicCAS(&tab[slot].key, 0u, key);
        if (old == 0u) atomicAdd(&n_unique[slice], 1u);
        if (old == 0u || old == key) {
            atomicAdd(&tab[slot].len, 1u);
            return;
        }
        slot = (slot + 1) & mask;
        /* a table that gets more than half full is thrown away and counted again at twice the size
         * (oslam_model_create): its pairs need not be counted, and must not walk a full table slot by slot (a model
         * of 4.6e5 keys spent seconds in the three passes that fill 2^16 .. 2^18 slots).  Looked at on long walks only;
         * the pass that is kept never gets there */
        if ((probe & 31u) == 31u && __hip_atomic_load(&n_unique[slice], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > t.cap / 2u) return;
    }
    atomicExch(overflow, 1u);
}

/* single workgroup: exclusive scan of len over every slot -> start */
__global__ __launch_bounds__(1024) void k_table_scan(oslamk_table t, uint32_t *total_out)
{
    __shared__ uint32_t part[1024];
    size_t total = (size_t)t.n_slices * t.cap;
    size_t chunk = (total + 1023) / 1024;
    size_t b = (size_t)threadIdx.x * chunk, e = b + chunk < total ? b + chunk : total;
    uint32_t s = 0;
    for (size_t i = b; i < e; i++) s += (t.slots[i].len + 3u) & ~3u;
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < 1024; i++) {
            uint32_t v = part[i];
            part[i] = run;
            run += v;
        }
        *total_out = run;
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (size_t i = b; i < e; i++) {
        t.slots[i].start = run;
        run += (t.slots[i].len + 3u) & ~3u;
    }
}

/* union table: every key of every slice once (what the scene-key kernel probes);
 * *n_keys counts the distinct keys */
__global__ void k_union_build(oslamk_table t, uint32_t *n_keys, uint32_t *overflow)
{
    size_t total = (size_t)t.n_slices * t.cap;
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    uint32_t key = t.slots[idx].key;
    if (key == 0) return;
    uint32_t mask = t.ucap - 1, slot = oslamk_slot_of(key, t.ushift);
    for (uint32_t probe = 0; probe < t.ucap; probe++) {
        uint32_t old = atomicCAS(&t.ukeys[slot], 0u, key);
        if (old == 0u) atomicAdd(n_keys, 1u);
        if (old == 0u || old == key) return;
        slot = (slot + 1) & mask;
    }
    atomicExch(overflow, 1u);
}

/* one workgroup per distance bin k1: does any of the 17^3 keys of that bin exist in the model? */
__global__ __launch_bounds__(256) void k_reach_build(oslamk_table t, float d_dist)
{
    __shared__ uint32_t s_found;
    const uint32_t k1 = blockIdx.x, mask = t.ucap - 1;
    if (threadIdx.x == 0) s_found = 0;
    __syncthreads();
    for (uint32_t combo = threadIdx.x; combo < PC_ANGLE_COMBOS; combo += 256) {
        const uint32_t key = pc_key_of_bins(k1, combo, d_dist);
        if (key == 0) continue;
        uint32_t slot = oslamk_slot_of(key, t.ushift);
        for (uint32_t probe = 0; probe <= mask; probe++) {
            const uint32_t k = t.ukeys[slot];
            if (k == key) { s_found = 1; break; }
            if (k == 0) break;
            slot = (slot + 1) & mask;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_found) atomicOr(&t.reach[k1 >> 5], 1u << (k1 & 31u));
}

/* weights[union slot of the key] += the length of the key's bucket, over the slice tables of one model: the entries a
 * hit on that key streams.  One thread per slot of the slice tables, probing as k_uinfo_build does. */
__global__ void k_union_weights(oslamk_table t, unsigned long long *weights)
{
    const size_t total = (size_t)t.n_slices * t.cap;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const oslamk_slot sl = t.slots[idx];
    if (sl.key == 0) return;
    const uint32_t mask = t.ucap - 1;
    uint32_t slot = oslamk_slot_of(sl.key, t.ushift);
    for (uint32_t probe = 0; probe <= mask; probe++) {
        const uint32_t k = t.ukeys[slot];
        if (k == sl.key) {
            atomicAdd(&weights[slot], (unsigned long long)sl.len);
            return;
        }
        if (k == 0) return;
        slot = (slot + 1) & mask;
    }
}

/* table.kmap[k1][combo] = the number (table.uids) of the key that distance bin k1 and the angle bins
 * `combo` hash to (pc_key_of_bins), or OSLAMK_KMAP_NONE: the scene-key kernel then needs neither the hash nor
 * a probe sequence.  One workgroup per distance bin k1 < table.kmap_bins. */
__global__ __launch_bounds__(256) void k_kmap_build(oslamk_table t, float d_dist)
{
    const uint32_t k1 = blockIdx.x, mask = t.ucap - 1;
    for (uint32_t combo = threadIdx.x; combo < PC_ANGLE_COMBOS; combo += 256) {
        const uint32_t key = pc_key_of_bins(k1, combo, d_dist);
        uint32_t found = OSLAMK_KMAP_NONE;
        if (key != 0) {
            uint32_t slot = oslamk_slot_of(key, t.ushift);
            for (uint32_t probe = 0; probe <= mask; probe++) {
                const uint32_t k = t.ukeys[slot];
                if (k == key) { found = t.uids[slot]; break; }
                if (k == 0) break;
                slot = (slot + 1) & mask;
            }
        }
        t.kmap[(size_t)k1 * PC_ANGLE_COMBOS + combo] = found;
    }
}

/* table.uinfo[slice][slot of the key in the union table] = the key's bucket in that slice: lets the vote
 * kernel go from a hit to its bucket with one load instead of a probe sequence.  One thread per slot of
 * the slice tables; uinfo is zeroed by the host (len 0 = the slice has no pair with that key). */
__global__ void k_uinfo_build(oslamk_table t)
{
    const size_t total = (size_t)t.n_slices * t.cap;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const oslamk_slot sl = t.slots[idx];
    if (sl.key == 0) return;
    const uint32_t mask = t.ucap - 1;
    uint32_t slot = oslamk_slot_of(sl.key, t.ushift);
    for (uint32_t probe = 0; probe <= mask; probe++) {
        if (t.ukeys[slot] == sl.key) {
            oslamk_uinfo ui;
            ui.start = sl.start;
            ui.len = sl.len | (sl.cur & 0x80000000u);      /* bit 31 of the fill cursor: marker entry in the bucket */
            t.uinfo[(idx / t.cap) * (size_t)t.uinfo_stride + t.uids[slot]] = ui;
            return;
        }
        slot = (slot + 1) & mask;
    }
}

/* pass 2: same pairs, written into their buckets */
__global__ void k_model_fill(oslamk_cloud c, float d_dist, float inv_d_dist, oslamk_table t,
                             const float *tmg, oslamk_entries ent)
{
    int m_r = blockIdx.y;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n || i == m_r) return;
    float nrx = c.nx[m_r], nry = c.ny[m_r], nrz = c.nz[m_r];
    float x, y, z;
    uint32_t key = cloud_pair_key(c, i, c.px[m_r], c.py[m_r], c.pz[m_r], nrx, nry, nrz,
                                  pc_norm3(nrx, nry, nrz), d_dist, inv_d_dist, &x, &y, &z);
    if (key == 0) return;
    int slice = m_r / OSLAMK_SLICE;
    oslamk_slot *tab = t.slots + (size_t)slice * t.cap;
    uint32_t mask = t.cap - 1, slot = oslamk_slot_of(key, t.shift);
    for (uint32_t probe = 0; probe < t.cap; probe++) {
        if (tab[slot].key == key) break;
        slot = (slot + 1) & mask;
    }
    uint32_t pos = atomicAdd(&tab[slot].cur, 1u) & 0x7fffffffu;   /* bit 31 is the marker flag */
    size_t e = (size_t)tab[slot].start + pos;
    const float *rows = tmg + 8 * (size_t)m_r;
    float uy = pc_row_dot(rows, x, y, z), uz = pc_row_dot(rows + 4, x, y, z);
    {
        const uint32_t th = pc_angle_t22(uy, uz);
        /* a marker forces the whole bucket through the exact path: flagged in bit 31 of the cursor */
        if (th == PC_T22_FORCE) atomicOr(&tab[slot].cur, 0x80000000u);
        ent.e4[e] = pc_entry_word(th == PC_T22_FORCE ? 0u : th, pc_row11((uint32_t)(m_r - slice * OSLAMK_SLICE)));
    }
    ent.mi[e] = (uint16_t)i;
    if (ent.uv) {
        oslamk_uv en;
        en.uy = uy;
        en.uz = uz;
        ent.uv[e] = en;
    }
}

/* pass 3: order inside every bucket.  A vote instruction adds 64 lanes' entries into acc[row][bin]; the LDS
 * serves 32 lanes together, one cycle per distinct address on the busiest bank (two are free: the instruction
 * takes four cycles to hand over its operands anyway).  The fill pass leaves the entries in arrival order:
 * 32 random banks collide 3-4 deep (7 LDS cycles per instruction instead of 4, tools/micro/lds_atomic_bench.hip).
 * Here every segment of 4096 positions (16 chunks) of a bucket is sorted by spread_key -- the quantity that
 * decides an entry's bank for every hit angle at once -- and dealt out so that each such group of 32 (same
 * chunk, same register j, same half of the wave) takes every G-th entry of the sorted order: keys about one
 * bank apart, mostly distinct banks.  Votes commute, so the order inside a bucket is free (model.cu:95-171
 * sorts them anyway).  One workgroup per slot. */
#define SPREAD_SEG 4096
#define SPREAD_THREADS 256
/* What the entries of a bucket are ordered by: the bank a vote lands on is floor(s - kappa) mod 32 with
 * kappa = (theta_u in bins - ACC_STRIDE * row) mod 32 and s the hit's angle in bins (but for the wrap of the bin
 * at 30, which moves a bank by 2), so lanes whose kappa are one apart never collide, whatever s is.  In units
 * of 2^-16 bank. */
__device__ __forceinline__ uint32_t spread_key(uint32_t entry_word)
{
    const uint32_t u = ((entry_word >> PC_ROW_BITS) * 30u) >> 5;              /* theta_u21 * 30 / 2^21 bins, << 16 */
    const uint32_t row = entry_word & PC_ROW10_MASK;
    return (u - ((row * ACC_STRIDE) << 16)) & ((32u << 16) - 1u);
}
/* how many positions p' < n of a chunk image (position = 4*lane + j) come before position p in
 * the dealing order (lane & 31, j, lane >> 5), for a chunk that holds n entries */
__device__ __forceinline__ uint32_t spread_rank_in_chunk(uint32_t p, uint32_t n)
{
    const uint32_t lane = p >> 2, j = p & 3u, h = lane & 31u, g = lane >> 5;
    uint32_t r = 0;
    for (uint32_t h2 = 0; h2 < h; h2++) {
        const uint32_t a0 = 4u * h2, a1 = 4u * (h2 + 32u);
        r += (n > a0 ? (n - a0 < 4u ? n - a0 : 4u) : 0u) + (n > a1 ? (n - a1 < 4u ? n - a1 : 4u) : 0u);
    }
    for (uint32_t j2 = 0; j2 < 4; j2++)
        for (uint32_t g2 = 0; g2 < 2; g2++) {
            if (j2 > j || (j2 == j && g2 >= g)) continue;
            r += (4u * (32u * g2 + h) + j2) < n;
        }
    return r;
}
__global__ __launch_bounds__(SPREAD_THREADS) void k_bucket_spread(oslamk_table t, oslamk_entries ent)
{
    __shared__ unsigned long long key[SPREAD_SEG];     /* theta_u << 32 | index in the segment */
    __shared__ uint32_t s_e4[SPREAD_SEG];
    __shared__ oslamk_uv s_uv[SPREAD_SEG];
    __shared__ uint16_t s_mi[SPREAD_SEG];
    const oslamk_slot sl = t.slots[blockIdx.x];
    if (sl.key == 0 || sl.len < 2) return;
    const int tid = threadIdx.x;
    for (uint32_t seg = 0; seg < sl.len; seg += SPREAD_SEG) {
        const uint32_t n = sl.len - seg < SPREAD_SEG ? sl.len - seg : SPREAD_SEG;
        const size_t base = (size_t)sl.start + seg;
        uint32_t P = 2;
        while (P < n) P <<= 1;
        for (uint32_t i = tid; i < P; i += SPREAD_THREADS) {
            if (i < n) {
                const uint32_t w = ent.e4[base + i];
                s_e4[i] = w;
                if (ent.uv) s_uv[i] = ent.uv[base + i];
                s_mi[i] = ent.mi[base + i];
                key[i] = ((unsigned long long)spread_key(w) << 32) | i;
            } else {
                key[i] = ~0ull;
            }
        }
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t x = tid; x < P / 2; x += SPREAD_THREADS) {
                    const uint32_t lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
                    const unsigned long long a = key[lo], b = key[hi];
                    const bool up = (lo & k) == 0;
                    if ((a > b) == up) { key[lo] = b; key[hi] = a; }
                }
                __syncthreads();
            }
        }
        /* position p of the segment takes the entry whose sorted rank is the number of positions
         * dealt before p: (lane & 31) first, then chunk, then (j, half) */
        const uint32_t n_full = n >> 8, n_last = n & 255u;
        for (uint32_t p = tid; p < n; p += SPREAD_THREADS) {
            const uint32_t c = p >> 8, q = p & 255u, h = (q >> 2) & 31u;
            const uint32_t nc = c < n_full ? 256u : n_last;
            uint32_t rank = 8u * h * n_full + spread_rank_in_chunk(4u * h, n_last);
            rank += 8u * (c < n_full ? c : n_full);
            rank += spread_rank_in_chunk(q, nc) - spread_rank_in_chunk(4u * h, nc);
            const uint32_t src = (uint32_t)key[rank];
            ent.e4[base + p] = s_e4[src];
            if (ent.uv) ent.uv[base + p] = s_uv[src];
            ent.mi[base + p] = s_mi[src];
        }
        __syncthreads();
    }
}

/* pass 4 (exact mode): every bucket once more, in segments of OSLAMK_PSEG entries ordered by P(word) = (word * 30)
 * mod 2^32 -- the position inside its bin that the entry's vote takes, up to the hit's constant (oslamk_entries).
 * ent.pw gets the words, ent.puv their uv (what a re-evaluation reads).  One workgroup per slot. */
__global__ __launch_bounds__(SPREAD_THREADS) void k_bucket_psort(oslamk_table t, oslamk_entries ent)
{
    __shared__ unsigned long long key[OSLAMK_PSEG];    /* P << 32 | index in the segment */
    __shared__ uint32_t s_e4[OSLAMK_PSEG];
    __shared__ oslamk_uv s_uv[OSLAMK_PSEG];
    const oslamk_slot sl = t.slots[blockIdx.x];
    if (sl.key == 0 || sl.len == 0) return;
    const int tid = threadIdx.x;
    for (uint32_t seg = 0; seg < sl.len; seg += OSLAMK_PSEG) {
        const uint32_t n = sl.len - seg < OSLAMK_PSEG ? sl.len - seg : OSLAMK_PSEG;
        const size_t base = (size_t)sl.start + seg;
        uint32_t P = 2;
        while (P < n) P <<= 1;
        for (uint32_t i = tid; i < P; i += SPREAD_THREADS) {
            if (i < n) {
                const uint32_t w = ent.e4[base + i];
                s_e4[i] = w;
                s_uv[i] = ent.uv[base + i];
                key[i] = ((unsigned long long)(w * 30u) << 32) | i;
            } else {
                key[i] = ~0ull;
            }
        }
        __syncthreads();
        for (uint32_t k = 2; k <= P; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t x = tid; x < P / 2; x += SPREAD_THREADS) {
                    const uint32_t lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
                    const unsigned long long a = key[lo], b = key[hi];
                    const bool up = (lo & k) == 0;
                    if ((a > b) == up) { key[lo] = b; key[hi] = a; }
                }
                __syncthreads();
            }
        }
        for (uint32_t i = tid; i < n; i += SPREAD_THREADS) {
            const uint32_t src = (uint32_t)key[i];
            ent.pw[base + i] = s_e4[src];
            ent.puv[base + i] = s_uv[src];
        }
        /* the directory: first position whose cell (the top log2 K bits of P) is >= k */
        const uint32_t K = OSLAMK_PDIR_CELLS(n);
        for (uint32_t k = tid; k <= K; k += SPREAD_THREADS) {
            uint32_t lo = 0, hi = n;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const uint32_t cell = (uint32_t)(((key[mid] >> 32) * (unsigned long long)K) >> 32);
                if (cell < k) lo = mid + 1; else hi = mid;
            }
            ent.pdir[(base << OSLAMK_PDIR_SHIFT) + k] = (uint16_t)lo;
        }
        __syncthreads();
    }
}

/* --------------------------------------------------------------------------
 * launchers
 * ------------------------------------------------------------------------*/
extern "C" {

int oslamk_row_keys(oslamk_cloud c, int ref, float d_dist, float inv_d_dist, uint32_t *keys_out,
                    void *stream)
{
    hipLaunchKernelGGL(k_row_keys, dim3((c.n + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, ref,
                       d_dist, inv_d_dist, keys_out);
    return (int)hipGetLastError();
}

int oslamk_model_count(oslamk_cloud c, float d_dist, float inv_d_dist, oslamk_table t,
                       uint32_t *n_unique, uint32_t *overflow, void *stream)
{
    hipLaunchKernelGGL(k_model_count, dim3((c.n + 255) / 256, c.n), dim3(256), 0, (hipStream_t)stream,
                       c, d_dist, inv_d_dist, t, n_unique, overflow);
    return (int)hipGetLastError();
}

int oslamk_table_scan(oslamk_table t, uint32_t *total_out, void *stream)
{
    hipLaunchKernelGGL(k_table_scan, dim3(1), dim3(1024), 0, (hipStream_t)stream, t, total_out);
    return (int)hipGetLastError();
}

int oslamk_union_build(oslamk_table t, uint32_t *n_keys, uint32_t *overflow, void *stream)
{
    size_t total = (size_t)t.n_slices * t.cap;
    hipLaunchKernelGGL(k_union_build, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, t, n_keys, overflow);
    return (int)hipGetLastError();
}

int oslamk_model_fill(oslamk_cloud c, float d_dist, float inv_d_dist, oslamk_table t,
                      const float *tmg, oslamk_entries ent, void *stream)
{
    hipLaunchKernelGGL(k_model_fill, dim3((c.n + 255) / 256, c.n), dim3(256), 0, (hipStream_t)stream,
                       c, d_dist, inv_d_dist, t, tmg, ent);
    return (int)hipGetLastError();
}

int oslamk_bucket_spread(oslamk_table t, oslamk_entries ent, void *stream)
{
    const size_t total = (size_t)t.n_slices * t.cap;
    hipLaunchKernelGGL(k_bucket_spread, dim3((unsigned)total), dim3(SPREAD_THREADS), 0, (hipStream_t)stream, t, ent);
    return (int)hipGetLastError();
}

int oslamk_bucket_psort(oslamk_table t, oslamk_entries ent, void *stream)
{
    const size_t total = (size_t)t.n_slices * t.cap;
    hipLaunchKernelGGL(k_bucket_psort, dim3((unsigned)total), dim3(SPREAD_THREADS), 0, (hipStream_t)stream, t, ent);
    return (int)hipGetLastError();
}

int oslamk_reach_build(oslamk_table t, float d_dist, void *stream)
{
    hipLaunchKernelGGL(k_reach_build, dim3(OSLAMK_REACH_BINS), dim3(256), 0, (hipStream_t)stream, t, d_dist);
    return (int)hipGetLastError();
}

int oslamk_union_weights(oslamk_table t, unsigned long long *weights, void *stream)
{
    const size_t total = (size_t)t.n_slices * t.cap;
    hipLaunchKernelGGL(k_union_weights, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, weights);
    return (int)hipGetLastError();
}

int oslamk_kmap_build(oslamk_table t, float d_dist, void *stream)
{
    if (t.kmap_bins == 0) return 0;
    hipLaunchKernelGGL(k_kmap_build, dim3(t.kmap_bins), dim3(256), 0, (hipStream_t)stream, t, d_dist);
    return (int)hipGetLastError();
}

int oslamk_uinfo_build(oslamk_table t, void *stream)
{
    const size_t total = (size_t)t.n_slices * t.cap;
    hipLaunchKernelGGL(k_uinfo_build, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t);
    return (int)hipGetLastError();
}

} /* extern "C" */
