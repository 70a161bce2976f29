/*
 * oslam_vote_body.inc -- the vote workgroup of the PPF registration path (gfx950): everything between a reference
 * point's sorted hit list and its accumulator peaks (ComputeUniqueVotes, model.cu:95-171; K3/K4, kernel.cu:480-554).
 * Included by two translation units: oslam_vote.hip (k_vote: the launch every registration runs) and
 * oslam_vote_wide.hip (k_vote_wide: the rare re-vote of workgroups whose 16-bit counters overflowed, which walks a
 * list in a loop and is built with its own flag, see there).  Expects oslam_kernels.h and ppf_core.h; the lane
 * helpers (WAVE, wave_sum_*, readlane_*, uni_*) are oslam_lane.h's.
 */
#ifndef OSLAM_VOTE_BODY_INC
#define OSLAM_VOTE_BODY_INC

#include "oslam_lane.h"

#ifndef VOTE_THREADS
#define VOTE_THREADS 1024
#endif
/* the accumulator of a vote workgroup in LDS: OSLAMK_ROWS rows of ACC_STRIDE words (oslam_kernels.h) */
#define ACC_CELLS (OSLAMK_ROWS * ACC_STRIDE)
#define ACC_REAL_CELLS (1023 * ACC_STRIDE)       /* counter words without the sink row; each holds two 16-bit counters */

/* thresholds of pc_alpha_bin_table(); every vote workgroup copies them into LDS */
static __device__ const uint32_t k_alpha_thr[32] = {PC_ALPHA_THR_FLAT};

/* --------------------------------------------------------------------------
 * voting
 * ------------------------------------------------------------------------*/
/* bin and position inside the bin of one vote, from tm = hit base - entry word (a 32-bit fraction of a turn; the
 * subtraction wraps with the angle): tm * 30 = bin * 2^32 + position.  The vote loop takes the high word alone
 * (v_mul_hi_u32, VoteRegs::vote); the re-evaluation of the near-edge votes wants both.  The empty asm keeps the
 * compiler from fusing (bin << 2) with the low word into a 64-bit shift. */
__device__ __forceinline__ void vote_product(uint32_t tm8, uint32_t &bin, uint32_t &pos)
{
    const unsigned long long p = (unsigned long long)tm8 * 30ull;
    bin = (uint32_t)(p >> 32);
    pos = (uint32_t)p;
    asm("" : "+v"(bin));
}

/* ---- the vote of one (model pair entry, scene hit) ---------------------------
 * A wave holds a chunk of 256 model-pair entries in registers: lane l has entries 4l .. 4l+3
 * of the chunk (one 16-byte load).  Every hit of the run votes with the chunk:
 *     tm  = hit's base (theta_v + half a turn + margin, scaled; one SGPR) - the entry word as stored
 *     bin = v_mul_hi_u32(tm, 30); the position inside the bin is the low word of the same product
 * Every vote goes into that bin.  The votes whose position lies within the margin of a bin edge (one in 4000) are
 * found afterwards by search (vote_body: correct_pass), re-evaluated with the reference's float sequence via
 * pc_alpha_bin_table (ppf_core.h) and moved if it says otherwise, so the bins are the reference's.  Lanes past the
 * end of the bucket are masked out of the atomics (EXEC), padding entries vote into the accumulator's sink row. */
#define ACC_TRASH_WORDS 96              /* slack behind the accumulator (16-byte zeroing, alignment of what follows) */

/* what the re-evaluation of a vote reads: the model's entries in the order of oslamk_entries.pw / .puv, the
 * reference point's hit list, the scene cloud and the rows y,z of T_s_g (kernel.cu:334-336) */
struct SlowCtx {
    const uint32_t *pw;
    const oslamk_uv *puv;
    const oslamk_pay *hits;
    const float *px, *py, *pz;
    const float *rows;
    uint32_t inc_lo, inc_hi;           /* what a vote adds to its counter word: by the half the model point owns */
    uint32_t dropped;                  /* re-evaluated votes that fell into no bin (alpha not a number) */
};

/* The second instantiation of ppf_math_atan.inc (see there): pm_atan2f_cold / pc_alpha_bin_exact_cold with every
 * literal materialised where it is used.  The re-evaluation of a vote takes the table path (pc_alpha_bin_table_main)
 * and this formula only for inputs the table does not cover -- zero or non-finite cross and dot products. */
#define PM_FN(n) n##_cold
#define PM_KU(bits) ({ uint32_t pinned_; asm volatile("v_mov_b32 %0, %1" : "=v"(pinned_) : "i"(bits)); pinned_; })
#define PM_KF(bits) __builtin_bit_cast(float, PM_KU(bits))
#undef PM_HD
#define PM_HD __device__ static inline
#include "ppf_math_atan.inc"
#undef PM_FN
#undef PM_KU
#undef PM_KF
__device__ __forceinline__ unsigned alpha_bin_reeval(float uy, float uz, float vy, float vz, const uint32_t *tbl)
{
    const unsigned b = pc_alpha_bin_table_main(uy, uz, vy, vz, tbl);
    return b != PC_ALPHA_OUTSIDE ? b : pc_alpha_bin_exact_cold(uy, uz, vy, vz);
}

/* LDS pointers of the out-of-line paths; their context lives in LDS too (a kernel's stack would be scratch memory) */
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) unsigned long long lds_u64;
typedef __attribute__((address_space(3))) SlowCtx lds_ctx;

/* Per-wave queue (LDS) of votes to re-evaluate with pc_alpha_bin_table: {entry index (pw order) | flag, hit index |
 * which of the four entries from there on << 28}; their operands are a dependent gather, so they are evaluated 64 at a
 * time by slow_queue_flush().  q: the wave's SLOW_CAP places; n: how many are taken (wave-uniform). */
#define SLOW_CAP 96
#define SLOW_VERIFY 0x80000000u        /* in an item's entry index: the votes have been cast into their quantised bins */
#define SLOW_HIT_BITS 28               /* a reference point's hit list has fewer than 2^28 hits (oslam_scene_create) */

__device__ __forceinline__ void slow_queue_flush(lds_ctx *sc, lds_u32 *acc, lds_u32 *tbl, lds_u64 *q, uint32_t n, int lane)
{
    const uint32_t *t = (const uint32_t *)tbl;
    for (uint32_t base = 0; base < n; base += WAVE) {
        if (base + lane < n) {
            const unsigned long long it = q[base + lane];
            const uint32_t entry = (uint32_t)it & ~SLOW_VERIFY, hi = (uint32_t)(it >> 32);
            const bool cast = ((uint32_t)it & SLOW_VERIFY) != 0u;
            const oslamk_pay hp = sc->hits[hi & ((1u << SLOW_HIT_BITS) - 1u)];
            const uint32_t i = hp.idx;
            const float x = sc->px[i], y = sc->py[i], z = sc->pz[i];
            const float vy = pc_row_dot(sc->rows, x, y, z);        /* as k_scene_hits computed them */
            const float vz = pc_row_dot(sc->rows + 4, x, y, z);
            /* a cast item names up to four consecutive entries (bits 28..31 of its hit word), an item that has not
             * been cast (an item with a marker) one */
#pragma nounroll
            for (uint32_t which = cast ? hi >> SLOW_HIT_BITS : 1u, j = 0; which; which >>= 1, j++) {
                if (!(which & 1u)) continue;
                const uint32_t ew = sc->pw[entry + j];
                const uint32_t mr = ew & PC_ROW10_MASK;
                const uint32_t inc = (ew >> PC_ROW_HALF_BIT) & 1u ? sc->inc_hi : sc->inc_lo;
                const float2 uv = *reinterpret_cast<const float2 *>(&sc->puv[entry + j]);
                const unsigned bin = alpha_bin_reeval(uv.x, uv.y, vy, vz, t);
                if (!cast) {
                    if (bin < OSLAMK_NBIN) atomicAdd((uint32_t *)&acc[mr * ACC_STRIDE + bin], inc);
                    else atomicAdd((uint32_t *)&sc->dropped, 1u);
                } else {
                    /* cast into its quantised bin and within the margin of a bin edge: moved if the reference's float
                     * sequence puts it into another bin (a counter word is only ever added to and subtracted from, so a
                     * carry between its two halves that a misplaced vote caused is undone with it, whichever comes
                     * first) */
                    uint32_t qbin, pos;
                    vote_product(pc_vote_base_t32(hp.theta_t22) - ew, qbin, pos);
                    if (bin != qbin) {
                        atomicSub((uint32_t *)&acc[mr * ACC_STRIDE + qbin], inc);
                        if (bin < OSLAMK_NBIN) atomicAdd((uint32_t *)&acc[mr * ACC_STRIDE + bin], inc);
                        else atomicAdd((uint32_t *)&sc->dropped, 1u);
                    }
                }
            }
        }
    }
}

/* appends the votes of `mask`'s lanes (entry, hit) to the wave's queue, emptying it first when they would not fit */
__device__ __forceinline__ uint32_t slow_push(lds_ctx *sc, lds_u32 *acc, lds_u32 *tbl, lds_u64 *q, uint32_t n,
                                              unsigned long long mask, uint32_t entry, uint32_t hit, int lane)
{
    if (n > SLOW_CAP - WAVE) {
        slow_queue_flush(sc, acc, tbl, q, n, lane);
        n = 0;
    }
    if ((mask >> lane) & 1ull)
        q[n + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (unsigned long long)entry | ((unsigned long long)hit << 32);
    return n + (uint32_t)__popcll(mask);
}

/* One step of a wave (all fields wave-uniform): one chunk of a bucket voted by the hits
 * i0 .. i1-1 of a run (at most 64 hits, one per lane). */
struct VoteStep {
    uint32_t e0;                       /* byte offset of the chunk's first entry from the slice's first entry */
    uint32_t nl;                       /* lanes that hold entries: (entries from the chunk start to the bucket end + 3) / 4, capped at 64 */
    uint32_t h0;                       /* byte offset of the run's first hit in the reference point's sorted list */
    uint32_t ne, nh;                   /* e0 / h0 + the bytes the step reads there: the sizes of its two buffer descriptors */
    uint32_t R;                        /* hits of the run */
    uint32_t i0, i1;                   /* the hits of the run that vote in this step */
    bool valid;
};

/* An item whose every vote is re-evaluated with the reference's float sequence -- its bucket holds an
 * entry with the marker, or one of its hits carries it (degenerate geometry: a second point on the
 * reference point's normal, a non-finite coordinate): every (entry, hit) pair goes through the queue.
 * Rare and slow on purpose; used after the vote loop, never inside it (inlined there: a call anywhere in the
 * kernel costs callee-saved registers and spills). */
__device__ __forceinline__ uint32_t forced_item(lds_ctx *sc, lds_u32 *acc, lds_u32 *tbl, lds_u64 *q, uint32_t n, uint32_t st,
                                             uint32_t ln, uint32_t h0, uint32_t R, int lane)
{
    for (uint32_t e = 0; e < ln; e += WAVE) {
        const unsigned long long nm = __ballot(e + (uint32_t)lane < ln);
        for (uint32_t i = 0; i < R; i++) n = slow_push(sc, acc, tbl, q, n, nm, st + e + (uint32_t)lane, h0 + i, lane);
    }
    return n;
}

/* The registers of a step in flight and its votes: lane l holds entries 4l .. 4l+3 of the chunk (one
 * 16-byte load) and theta_v of hit `lane` of the run.  One code path for full and partial chunks: the
 * atomics are issued with EXEC narrowed to the lanes that hold entries, so idle lanes cost no LDS cycles
 * and cause no bank conflicts; the padding behind a bucket votes into the sink row.  Written in asm because
 * the compiler has no way to say this; the workgroup waits for these atomics (lgkmcnt) before it reads the
 * accumulator.  Per hit (256 votes): v_readlane + 4 x (v_sub, v_mul_hi, v_fma_f32) + 4 LDS atomics + three scalar
 * instructions of loop control = 20 instructions, in both modes.  Items that carry a marker never come here
 * (forced_item). */
/* word 3 of a raw buffer descriptor on gfx9: 32-bit data format, no swizzle, no stride */
#define OSLAM_RSRC_RAW 0x00020000
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int MODE>
struct VoteRegs {
    uint4 v;
    uint32_t th;
    /* Unconditional on purpose: every lane loads, whatever the chunk and the run hold, so that the loads of
     * a group are straight-line code and the compiler can wait for each member's registers alone
     * (vmcnt(N)) instead of draining everything. */
    __device__ __forceinline__ void load(const uint32_t *e4, const oslamk_pay *hits, const VoteStep &d, int lane)
    {
        /* Buffer loads: the descriptor (base = the chunk's / the run's first byte, size = what the step holds) is built
         * with scalar instructions from the wave-uniform step, the lane's offset is a loop-invariant register, and
         * lanes past the end of the bucket / the run read nothing and get 0 -- no vector instruction per step for the
         * addresses (a flat load took four: compare, select, 64-bit add). */
        const uint32_t lane16 = 16u * (uint32_t)lane, lane8 = 8u * (uint32_t)lane;
        /* the base stays (the slice's entries, the reference point's hit list) and the step's place goes into the scalar
         * offset; the range check adds it to the lane's offset, so the size counts from the base as well */
        const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc((void *)e4, 0, (int)d.ne, OSLAM_RSRC_RAW);
        const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void *)&hits[0].theta_t22, 0, (int)d.nh, OSLAM_RSRC_RAW);
        const u32x4 e = __builtin_amdgcn_raw_buffer_load_b128(re, (int)lane16, (int)d.e0, 0);
        v = make_uint4(e.x, e.y, e.z, e.w);
        th = __builtin_amdgcn_raw_buffer_load_b32(rh, (int)lane8, (int)d.h0, 0);
    }
    __device__ __forceinline__ void vote(uint32_t *accp, const VoteStep &d, int lane, uint32_t inc_lo, uint32_t inc_hi) const
    {
        lds_u32 *acc = (lds_u32 *)accp;
        /* the entry words as they are: theta_u << 11 | half << 10 | row (pc_entry_word); lanes and words past the
         * end of the bucket are masked out of the atomics (EXEC) or are padding entries that vote into the sink
         * row.  A counter word holds two 16-bit counters: the model points of the lower half of the slice add 1,
         * those of the upper half 0x10000 (inc_lo / inc_hi; one of them is 0 in the rare second and third pass
         * of a workgroup whose 16-bit counters overflowed) */
        const uint32_t wa[4] = {v.x, v.y, v.z, v.w};
        /* pc_vote_base_t32(th) = (th << 10) + a constant, which is kept in a scalar register; fast mode casts from the
         * unshifted base (pc_vote_base_fast_t32: nothing there moves a vote that the margin shifted across an edge) */
        uint32_t csmv;
        asm("v_lshl_add_u32 %0, %1, 10, %2" : "=v"(csmv) : "v"(th), "s"(MODE == 0 ? pc_vote_base_t32(0u) : pc_vote_base_fast_t32(0u)));
        const uint32_t acc_base = (uint32_t)(uintptr_t)acc;  /* the accumulator's LDS address */
        uint32_t rowb[4], inc[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            rowb[j] = acc_base + (wa[j] & PC_ROW10_MASK) * (4u * ACC_STRIDE);     /* LDS address of the entry's row */
            /* inc_lo or inc_hi by the half bit: a bit-field extract and (first pass) one 24-bit multiply-add, in asm
             * because the compiler turns every spelling of it into and + compare + select */
            if (inc_hi == 0x10000u)
                asm("v_bfe_u32 %0, %1, 10, 1\n\tv_mad_u32_u24 %0, %0, %2, 1" : "=&v"(inc[j]) : "v"(wa[j]), "s"(0xffffu));
            else                         /* the wide passes count one half of the slice's model points with 32-bit counters: 1 or 0 */
                inc[j] = ((wa[j] >> PC_ROW_HALF_BIT) & 1u) ^ (inc_lo ? 1u : 0u);
        }
        /* lanes that hold at least one entry of this chunk (wave-uniform: two scalar instructions; an empty step has
         * no hits to vote, its mask does not matter) */
        const unsigned long long live = ~0ull >> ((64u - d.nl) & 63u);
#ifdef VOTE_DIAG_NOLOOP                 /* timing-only build: steps and loads without the votes */
        asm volatile("" ::"v"(wa[0]), "v"(wa[1]), "v"(wa[2]), "v"(wa[3]), "v"(csmv), "s"(live));
        return;
#endif
        /* Every vote goes into its quantised bin, in both modes.  The kernel is bound by the number of instructions its
         * waves issue, of whatever kind (3.6 cycles per instruction and SIMD over the whole kernel, scalar ones
         * included: profiles/r03_pmc_sq_k_vote.txt), so the loop over the hits is written out: per hit and chunk
         * v_readlane + 4 x (v_sub, v_mul_hi, v_fma_f32) + 4 ds_add_u32 + s_add, s_cmp, s_cbranch = 20 instructions,
         * EXEC narrowed to the live lanes once per step, not per hit (the compiler's loop had 24: EXEC saved, set and
         * restored around the atomics of every hit, and a hazard s_nop).  The two scalar instructions between
         * v_readlane and the first v_sub are the wait states gfx950 asks for between a vector write of a scalar
         * register and its vector read.  Three vector instructions per vote; two would do -- (base - word) * 120 +
         * (row address << 32) has row address + 4 * bin + (0..3) in its high word -- if the LDS ignored the two low
         * address bits of a 32-bit atomic; gfx950 raises a memory violation instead
         * (tools/micro/lds_misaligned_atomic.hip).  In exact mode the votes that lie within the margin of a bin edge
         * are found afterwards, by search (vote_body: correct_pass), and moved where the reference's float sequence
         * says so. */
        if (d.i0 < d.i1) {
            uint32_t c, t0, t1, t2, t3;
            unsigned long long saved;
#ifdef VOTE_DIAG_NOATOM             /* timing-only build: the vote arithmetic without the LDS atomics */
#define VOTE_ATOMICS ""
#else
#define VOTE_ATOMICS "ds_add_u32 %[t0], %[n0]\n\tds_add_u32 %[t1], %[n1]\n\tds_add_u32 %[t2], %[n2]\n\tds_add_u32 %[t3], %[n3]\n\t"
#endif
            /* The vote's address, row address + 4 * bin, is computed on the float pipe.  A 32-bit pattern below 2^23 read
             * as a float is zero or a denormal worth n * 2^-149, so v_fma_f32 on such patterns is exact integer
             * arithmetic, and on gfx950 it issues in 2.5 cycles where v_lshl_add_u32 takes 4.2
             * (tools/micro/valu_rate_bench.hip, profiles/r19_float_pipe_microbench.txt).  What the form depends on:
             *   - patterns below 2^23 on both sides, so that nothing is rounded: the largest value is the last bin of
             *     the sink row, acc_base + 1023 * 124 + 4 * 30 (checked here for any acc_base in the 160 KiB of LDS);
             *   - f32 denormals kept, in and out: float_denorm_mode_32 = 3 in the kernel descriptor, which
             *     tools/kernel_resources.sh prints for the vote kernels.  Flushed, every vote would land in word 0.
             * In asm like the rest of the loop, so the compiler sees no float arithmetic that it could fold.  The
             * integer form stays behind -DVOTE_INT_ADDR for A/B builds from one source (make EXTRA=-DVOTE_INT_ADDR).
             * The row address and the first-pass increment of the step were built the same way (v_fmamk_f32, v_fma_f32)
             * and gained too little to keep: profiles/r19_bench_parent_vs_float_pipe.txt. */
            static_assert(160u * 1024u + (OSLAMK_ROWS - 1u) * (4u * ACC_STRIDE) + 4u * 30u < (1u << 23),
                          "the float form of the vote address needs every pattern below 2^23");
#ifdef VOTE_INT_ADDR
#define VOTE_ADDR(t, r) "v_lshl_add_u32 " t ", " t ", 2, " r "\n\t"
#else
#define VOTE_ADDR(t, r) "v_fma_f32 " t ", " t ", 4.0, " r "\n\t"
#endif
            uint32_t i = d.i0;
            asm volatile("s_mov_b64 %[sv], exec\n\t"
                         "s_mov_b64 exec, %[live]\n"
                         ".Lvote_hit_%=:\n\t"
                         "v_readlane_b32 %[c], %[csmv], %[i]\n\t"
                         "s_add_u32 %[i], %[i], 1\n\t"
                         "s_cmp_lt_u32 %[i], %[i1]\n\t"
                         "v_sub_u32 %[t0], %[c], %[w0]\n\t"
                         "v_sub_u32 %[t1], %[c], %[w1]\n\t"
                         "v_sub_u32 %[t2], %[c], %[w2]\n\t"
                         "v_sub_u32 %[t3], %[c], %[w3]\n\t"
                         "v_mul_hi_u32 %[t0], %[t0], 30\n\t"
                         "v_mul_hi_u32 %[t1], %[t1], 30\n\t"
                         "v_mul_hi_u32 %[t2], %[t2], 30\n\t"
                         "v_mul_hi_u32 %[t3], %[t3], 30\n\t"
                         VOTE_ADDR("%[t0]", "%[r0]") VOTE_ADDR("%[t1]", "%[r1]") VOTE_ADDR("%[t2]", "%[r2]") VOTE_ADDR("%[t3]", "%[r3]") VOTE_ATOMICS
                         "s_cbranch_scc1 .Lvote_hit_%=\n\t"
                         "s_mov_b64 exec, %[sv]"
                         : [sv] "=&s"(saved), [c] "=&s"(c), [i] "+s"(i), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3)
                         : [live] "s"(live), [csmv] "v"(csmv), [i1] "s"(d.i1), [w0] "v"(wa[0]), [w1] "v"(wa[1]), [w2] "v"(wa[2]),
                           [w3] "v"(wa[3]), [r0] "v"(rowb[0]), [r1] "v"(rowb[1]), [r2] "v"(rowb[2]), [r3] "v"(rowb[3]), [n0] "v"(inc[0]),
                           [n1] "v"(inc[1]), [n2] "v"(inc[2]), [n3] "v"(inc[3])
                         : "scc", "memory");
#undef VOTE_ATOMICS
#undef VOTE_ADDR
        }
    }
};

/* --------------------------------------------------------------------------
 * One workgroup = one (scene reference point, model slice).
 * LDS: acc[1024][32] u32 = 128 KiB (one workgroup per CU, 16 waves).
 * ComputeUniqueVotes (model.cu:95-171) without the vote list: K3/K4
 * (kernel.cu:480-554) accumulate straight into acc, and the sort/histogram/
 * threshold of model.cu:148-170 becomes the scan at the end.
 *
 * An item of work is one run of the reference point (hits that share a key) with the key's bucket
 * in this slice, found by one load of table.uinfo[slice][slot]: there is no probing here and no
 * list of items.  Its cost is chunks x hits vote iterations (a chunk = 256 entries, an iteration =
 * one hit voting with the chunk a wave holds in registers: four LDS atomics per lane).
 *   - Pre-scan, all threads: items above VOTE_GIANT iterations ("giants": the buckets of planar
 *     surfaces hold 10^4 entries) are queued in LDS.
 *   - Giants first: cut into units of one chunk x at most 16-32 hits, dealt round-robin to the
 *     16 waves.
 *   - Then the rest, dynamically: a wave takes VOTE_BLOCK runs at a time from a counter in LDS and
 *     skips the giants; the run records of the block two ahead and the bucket records of the next
 *     one are in flight.
 * No barrier between the two; the waves meet at the end.
 * The entry stream (200 GB per 5k x 100k registration, from the Infinity Cache and HBM) is what
 * has to be kept busy: with one step's loads in flight per wave the kernel sat at the latency of a
 * load per step (59 of 89 ms with the votes compiled out).  So a wave works in groups of VOTE_GROUP
 * steps: their descriptors first, then all their loads back to back (16 B per lane each), then the
 * votes, one copy of the vote loop per member so that each waits for its own registers only.
 * Workgroups b and b + 8 share an XCD (speed only): the slices of one reference point are placed
 * on one XCD, so its hit and run lists reach one L2 once.
 * ------------------------------------------------------------------------*/
#define VOTE_QCAP 1024
#ifndef VOTE_BLOCK
#define VOTE_BLOCK 16
#endif
#ifndef VOTE_TAIL
#define VOTE_TAIL VOTE_BLOCK    /* runs per block at the end of a reference point's run list (a divisor of VOTE_BLOCK) */
#endif
#ifndef VOTE_TAIL_RUNS
#define VOTE_TAIL_RUNS 0
#endif
#ifndef VOTE_GIANT
#define VOTE_GIANT 16            /* 16 and groups of 8: profiles/r03_ab_giant_threshold_and_group.txt */
#endif
#ifndef VOTE_WIDE_DIRECT
#define VOTE_WIDE_DIRECT (1ull << 27)      /* votes of a workgroup from which it skips the pass with 16-bit counters */
#endif
#ifndef VOTE_GROUP
#define VOTE_GROUP 8           /* must divide 64 */
#endif
#define RUN_SLOT_MASK ((1u << OSLAMK_RUN_SHIFT) - 1u)

template <int MODE, int PASS>
__device__ __forceinline__ void vote_body(const oslamk_vote_args &a, const uint32_t wg)
{
    __shared__ __attribute__((aligned(16))) uint32_t acc[ACC_CELLS + ACC_TRASH_WORDS];
    __shared__ uint32_t s_wave[VOTE_THREADS / WAVE];
    __shared__ uint32_t s_wave2[VOTE_THREADS / WAVE];
    __shared__ unsigned long long s_tot[2];            /* votes; entries streamed | items << 40 */
    __shared__ unsigned long long s_sum[VOTE_THREADS / WAVE];
    __shared__ uint32_t s_redo;
    __shared__ uint32_t s_g, s_lmax, s_base, s_qn, s_next;
    __shared__ uint32_t s_tbl[32];
    __shared__ uint32_t s_q[VOTE_QCAP];
    __shared__ SlowCtx s_ctx;
    __shared__ unsigned long long s_slow[MODE == 0 ? (VOTE_THREADS / WAVE) * SLOW_CAP : 1];

    typedef VoteRegs<MODE> VR;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
    const uint32_t nsl = (uint32_t)a.table.n_slices;
    const uint32_t xg = wg & 7u, xi = wg >> 3;
    const uint32_t ref_pos = (xi / nsl) * 8u + xg;   /* dispatch position: the slices of a reference point share an XCD */
    const int slice = (int)(xi % nsl);
    if (ref_pos >= (uint32_t)a.n_launch) return;     /* the grid is padded to a multiple of 8 reference points */
    /* the reference point of that position: the host hands the heavy ones out first (oslamk_vote_args.ref_order) */
    const int ref_local = (int)(a.ref_order ? uni_u32(a.ref_order[ref_pos]) : ref_pos);
    if ((uint32_t)ref_local >= (uint32_t)a.n_launch) return;
    const int ref_ord = a.first_ref + ref_local;
    const uint32_t r = a.ref_idx[ref_ord];
    const uint32_t n_runs = a.run_count[ref_local];
    const size_t off = a.hit_off[ref_local];
    const oslamk_pay *hits = a.hit_sorted + off;
    const oslamk_run *runs = a.runs + off;
    const oslamk_uinfo *uinfo = a.table.uinfo + (size_t)slice * a.table.uinfo_stride;
    /* The slice's entries are one contiguous piece of the entry array (k_table_scan lays the slots out slice by slice;
     * oslam_model_load checks it): steps address them relative to its first entry, as a 32-bit byte offset */
    const uint32_t e_first = uni_u32(a.table.slots[(size_t)slice * a.table.cap].start);
    const uint32_t *e4 = a.ent.e4 + e_first;
    const uint32_t m_base = (uint32_t)slice * OSLAMK_SLICE;   /* first model reference of the slice */
    if (tid == 0) {
        s_ctx.pw = a.ent.pw;
        s_ctx.puv = a.ent.puv;
        s_ctx.hits = hits;
        s_ctx.px = a.scene.px;
        s_ctx.py = a.scene.py;
        s_ctx.pz = a.scene.pz;
        s_ctx.rows = a.tsg + 8 * (size_t)ref_ord;
        s_ctx.inc_lo = PASS == 2 ? 0u : 1u;
        s_ctx.inc_hi = PASS == 0 ? 0x10000u : PASS == 2 ? 1u : 0u;
        s_ctx.dropped = 0;
    }
    const SlowCtx *sc = &s_ctx;

    for (int c = tid; c < ACC_CELLS / 4; c += VOTE_THREADS) reinterpret_cast<uint4 *>(acc)[c] = make_uint4(0, 0, 0, 0);
    if (tid < 32) s_tbl[tid] = k_alpha_thr[tid];

    unsigned long long *sq = s_slow + (MODE == 0 ? wid * SLOW_CAP : 0);   /* this wave's re-evaluation queue */
    uint32_t sq_n = 0;
#ifdef VOTE_PROF
    const long long pt0 = clock64();
#endif

    /* ---- pre-scan: votes of this workgroup, giants into the queue ---- */
    uint32_t T = VOTE_GIANT;
    for (bool first = true;; first = false) {
        if (tid == 0) {
            s_qn = 0;
            s_next = 0;
            if (first) s_tot[0] = s_tot[1] = 0;
        }
        __syncthreads();
        for (uint32_t k0 = 0; k0 < n_runs; k0 += VOTE_THREADS) {
            const uint32_t k = k0 + (uint32_t)tid;
            bool giant = false;
            unsigned long long lv = 0, le = 0;
            if (k < n_runs) {
                const oslamk_run rr = runs[k];
                const uint32_t lf = uinfo[rr.slot_r & RUN_SLOT_MASK].len;
                const uint32_t ln = lf & 0x7fffffffu, R = (rr.slot_r >> OSLAMK_RUN_SHIFT) + 1u;
                lv = (unsigned long long)ln * R;
                le = ((unsigned long long)(ln != 0u) << 40) + ln;       /* items in the upper bits: one reduction for both */
                /* items with a marker (MODE 0) are neither giants nor small items: they wait for the pass after the loop */
                giant = ((ln + 255u) >> 8) * R > T && !(MODE == 0 && ((lf | rr.first) >> 31));
            }
            if (first) {            /* summed over the wave and parked in LDS: no register lives on through the vote loops */
                lv = wave_sum_u64(lv);
                le = wave_sum_u64(le);
                if (lane == 0 && le) {
                    atomicAdd(&s_tot[0], lv);
                    atomicAdd(&s_tot[1], le);
                }
            }
            const unsigned long long gm = __ballot(giant);
            if (gm) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&s_qn, (uint32_t)__popcll(gm));
                base = readlane_u(base, 0);
                const uint32_t p = base + (uint32_t)__popcll(gm & ((1ull << lane) - 1ull));
                if (giant && p < VOTE_QCAP) s_q[p] = k;
            }
        }
        __syncthreads();            /* also: acc zeroed, s_tbl and s_ctx written */
        if (s_qn <= VOTE_QCAP) break;
        T *= 2;                     /* more giants than the queue holds: a higher bar, same for every thread */
        __syncthreads();
    }
    const uint32_t n_q = uni_u32(s_qn);
    T = uni_u32(T);
    /* A workgroup with this many votes for its 61 380 sixteen-bit counters (clouds dominated by large planes: every
     * in-plane pair has the same feature) would overflow them almost surely: it goes straight to the passes with
     * 32-bit counters instead of voting here first and noticing afterwards.  The bench scene's workgroups cast 5e6. */
    if (PASS == 0 && s_tot[0] > VOTE_WIDE_DIRECT) {
        if (tid == 0) {
            a.redo[atomicAdd(&a.counters->redo_count, 1u)] = wg;
            atomicAdd(&a.counters->redo_total, 1u);
        }
        return;
    }
#ifdef VOTE_PROF
    const long long ptA = clock64();
#endif

    /* A counter word of the accumulator holds two 16-bit counters (two model reference points per row: a slice of
     * 2046 fits the 128 KiB).  PASS 0 -- the kernel every registration runs -- votes into both at once.  A counter
     * that passes 65535 carries into its neighbour: the sum of all counters then falls short of the votes cast
     * (every overflow takes 65535 or 65536 away, never adds); the workgroup notices, emits nothing and puts itself
     * on the redo list, and k_vote_wide votes for it again with full 32-bit counters, first for the lower half of
     * the slice's model points (PASS 1), then for the upper (PASS 2).  Counts beyond 16 bits need large planar
     * surfaces in both clouds; the bench scene's largest cell is 17 186. */
    const uint32_t pass = PASS;
    const uint32_t inc_lo = PASS == 2 ? 0u : 1u, inc_hi = PASS == 0 ? 0x10000u : PASS == 2 ? 1u : 0u;
    {
        /* ---- the work of this wave, as windows of up to 64 step descriptors made lane-parallel ----
         * A set of items sits in the lanes of two register pairs: the run record {slot | hits - 1, first hit} and
         * the bucket record {start, length} of up to 64 items; `take` says which lanes belong to the set, and
         * every item is cut into units (chunks, times 1, 2 or 4 ranges of hits for a giant).  The wave takes the
         * units u0, u0 + stride, ... of the set: lane i of a window looks its unit up in the running sums of the
         * set (binary search across lanes with ds_bpermute) and computes the step {first entry, entries left,
         * first hit, hits, hit range} -- about one instruction per step instead of a scalar generator of ~60.
         * The steps of a window are then voted in groups of VOTE_GROUP: descriptors to scalar registers,
         * all the group's loads back to back (16 B per lane each), the votes, one copy of the vote loop
         * per member so that each waits for its own registers only. */
        uint2 B_ru = make_uint2(0, 0), B_inf = make_uint2(0, 0);
        auto bperm = [&](uint32_t from_lane, uint32_t v) -> uint32_t {
            return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(from_lane << 2), (int)v);
        };
        /* step g of a window: its descriptor from lane g of the window's registers (VOTE_GROUP divides 64, so a
         * group never runs past lane 63; lanes past the window's end describe empty steps) */
        auto step_at = [&](uint32_t ve0, uint32_t vh0, uint32_t vmisc, int l) -> VoteStep {
            VoteStep d;
            const uint32_t misc = readlane_u(vmisc, l);
            d.e0 = readlane_u(ve0, l);
            d.h0 = readlane_u(vh0, l);
            /* the sizes of the two descriptors with scalar instructions: taking them from two more window registers
             * (v_readlane, then wait states before the loads may use them) cost 0.8 ms */
            d.ne = d.e0 + (misc >> 20) * 16u;
            d.nh = d.h0 + (misc & 63u) * 8u + 8u;
            d.R = (misc & 63u) + 1u;
            d.i0 = (misc >> 6) & 127u;
            d.i1 = (misc >> 13) & 127u;
            d.nl = misc >> 20;
            d.valid = true;
            return d;
        };
        /* hit ranges a chunk of an item with R hits is cut into, as a shift: giants only */
        auto split_of = [&](uint32_t R, bool split) -> uint32_t { return !split ? 0u : R > 32u ? 2u : R > 16u ? 1u : 0u; };
        /* votes the units u0, u0 + stride, ... of the items in the lanes where `take` holds */
        auto vote_set = [&](bool take, bool split, uint32_t u0, uint32_t stride) {
            uint32_t excl, incl;
            {
                const uint32_t R = (B_ru.x >> OSLAMK_RUN_SHIFT) + 1u;
                const uint32_t nu = take ? (((B_inf.y & 0x7fffffffu) + 255u) >> 8) << split_of(R, split) : 0u;
                incl = nu;
                for (int o = 1; o < WAVE; o <<= 1) {
                    const uint32_t up = __shfl_up(incl, o, WAVE);
                    if (lane >= o) incl += up;
                }
                excl = incl - nu;
            }
            const uint32_t total = readlane_u(incl, WAVE - 1);
            for (uint32_t ub = u0; ub < total; ub += stride * WAVE) {
                /* ---- the window: lane i <-> unit ub + stride * i ---- */
                const uint32_t u = ub + stride * (uint32_t)lane;
                const bool act = u < total;
                uint32_t lo = 0;                                   /* items whose running sum is <= u: the unit's item */
    #pragma unroll
                for (uint32_t s2 = WAVE / 2; s2 > 0; s2 >>= 1) lo += bperm(lo + s2 - 1u, incl) <= u ? s2 : 0u;
                lo = lo < (uint32_t)WAVE - 1u ? lo : (uint32_t)WAVE - 1u;
                const uint32_t st = bperm(lo, B_inf.x), ln = bperm(lo, B_inf.y) & 0x7fffffffu, h0 = bperm(lo, B_ru.y) & 0x7fffffffu;
                const uint32_t R = (bperm(lo, B_ru.x) >> OSLAMK_RUN_SHIFT) + 1u, lg = split_of(R, split);
                const uint32_t local = u - bperm(lo, excl);
                const uint32_t c = local >> lg, hs = local & ((1u << lg) - 1u), per = (R + (1u << lg) - 1u) >> lg;
                const uint32_t i0 = hs * per, i1 = i0 + per < R ? i0 + per : R;
                /* a lane past the end describes a step that loads entry 0 and hit 0 and votes nothing */
                const uint32_t left = ln - (c << 8), nl = left < 256u ? (left + 3u) >> 2 : 64u;
                /* the scalar side of a step is kept short (every instruction counts, see VoteRegs::vote): byte offsets and
                 * the number of live lanes are made here, once for 64 steps */
                const uint32_t w_e0 = act ? (st - e_first + (c << 8)) * 4u : 0u, w_h0 = act ? h0 * 8u : 0u,
                               w_misc = act ? (R - 1u) | (i0 << 6) | (i1 << 13) | (nl << 20) : 0u;
                const uint32_t rest = (total - ub + stride - 1u) / stride, n_w = rest < (uint32_t)WAVE ? rest : (uint32_t)WAVE;
                for (uint32_t g0 = 0; g0 < n_w; g0 += VOTE_GROUP) {
                    VR regs[VOTE_GROUP];
                    VoteStep ds[VOTE_GROUP];
    #pragma unroll
                    for (int g = 0; g < VOTE_GROUP; g++) {
                        ds[g] = step_at(w_e0, w_h0, w_misc, (int)g0 + g);
                        regs[g].load(e4, hits, ds[g], lane);
                    }
                    asm volatile("" ::: "memory");      /* all the group's loads are issued here, in this order: none sinks into its vote */
    #pragma unroll
                    for (int g = 0; g < VOTE_GROUP; g++) regs[g].vote(acc, ds[g], lane, inc_lo, inc_hi);
                }
            }
        };
        /* Exact mode: the votes that lie within the margin of a bin edge, found instead of tested for.  A vote of hit h
         * with entry word w has position (P(base_h) - P(w)) mod 2^32 inside its (shifted) bin, P(x) = x * 30 mod 2^32 --
         * the low word of vote_product -- and is near an edge when that is below PC_T24_EDGE.  Every bucket exists a
         * second time ordered by P(w) (oslamk_entries.pw, segments of OSLAMK_PSEG entries) with a directory of cells of
         * equal width in P (pdir), so the near-edge entries of a hit are a contiguous piece of it, cyclically: the cells
         * that the window [A, A + PC_T24_EDGE) touches, A = P(base_h) - PC_T24_EDGE + 1.  One lane per HIT of the
         * reference point: the sorted key number of the hit (k_sort_hits leaves them in hit_key; bit 31: its run holds a
         * marker and is not voted here) gives the bucket of this slice with one load, two directory places give the
         * piece, and its entries that pass the test -- one vote in 4000 -- go to the wave's queue, whose flush moves
         * those that the reference's float sequence bins otherwise.  The search does not depend on which wave voted the
         * hit's run, or when (moves and votes commute): the passes of 64 hits are dealt round-robin to the waves, one
         * between two sets of votes so that its loads fly while the others vote, the rest behind the votes. */
        const uint32_t *skeys = a.hit_key + off;
        const uint32_t n_hits = a.hit_count[ref_local] < (uint32_t)(a.hit_off[ref_local + 1] - off) ? a.hit_count[ref_local]
                                                                                                   : (uint32_t)(a.hit_off[ref_local + 1] - off);
        const uint32_t n_cq = (n_hits + WAVE - 1u) / WAVE;
        uint32_t cq = uni_u32((uint32_t)wid);           /* the next pass of this wave */
#ifdef VOTE_PROF
        long long prof_corr = 0;
#endif
        auto correct_pass = [&]() {
#ifdef VOTE_PROF
            const long long pc0 = clock64();
#endif
            const uint32_t *pw = a.ent.pw;
            const uint16_t *pdir = a.ent.pdir;
            const uint32_t hit = cq * WAVE + (uint32_t)lane;
            cq += VOTE_THREADS / WAVE;
            const bool in = hit < n_hits;
            const uint32_t kw = skeys[in ? hit : 0u];
            /* checked, not assumed (a damaged table or list must not become a wild load): the key number inside the
             * bucket records, the bucket inside the entry arrays, the directory places inside their segment */
            const bool key_ok = (kw & RUN_SLOT_MASK) < a.table.uinfo_stride;
            const oslamk_uinfo ui = uinfo[key_ok ? kw & RUN_SLOT_MASK : 0u];
            uint32_t ln = in && key_ok && !((kw | ui.len) >> 31) ? ui.len : 0u;    /* 0: no bucket in this slice, or an item with a marker */
            const bool bucket_ok = ln == 0u || (ui.start <= a.ent.n_real && ln <= a.ent.n_real - ui.start);
            if (!bucket_ok) ln = 0;
            if (__ballot((in && !key_ok) || !bucket_ok)) {
                if (in && !key_ok) atomicOr(&a.counters->list_overflow, 2u);
                if (!bucket_ok) atomicOr(&a.counters->list_overflow, 4u);
            }
            const uint32_t A = pc_vote_base_t32(hits[in ? hit : 0u].theta_t22) * 30u - (PC_T24_EDGE - 1u), B = A + (PC_T24_EDGE - 1u);
            for (uint32_t seg = 0; __ballot(seg < ln); seg += OSLAMK_PSEG) {        /* one round unless a bucket is above OSLAMK_PSEG entries */
                const uint32_t n = seg < ln ? (ln - seg < OSLAMK_PSEG ? ln - seg : OSLAMK_PSEG) : 0u;
                const uint32_t sbase = n ? ui.start + seg : 0u, K = OSLAMK_PDIR_CELLS(n);
                const uint32_t cA = __umulhi(A, K), cB = __umulhi(B, K);
                const uint32_t d0 = n ? pdir[((size_t)sbase << OSLAMK_PDIR_SHIFT) + cA] : 0u, d1 = n ? pdir[((size_t)sbase << OSLAMK_PDIR_SHIFT) + cB + 1u] : 0u;
                uint32_t cnt = K == 1u ? n : B < A ? n - d0 + d1 : d1 - d0;         /* B < A: the window wraps past 2^32 */
#ifdef VOTE_DIAG_NOCAND                 /* timing-only build: the search without its candidate loop */
                cnt = 0;
#endif
                if (d0 > n || d1 > n || cnt > 2u * n) {
                    atomicOr(&a.counters->list_overflow, 8u);
                    cnt = 0;
                }
                /* The lanes' candidates as one list, lane after lane (running sums across the wave), tested 64 at a
                 * time whoever owns them, four rounds' loads in flight together: a pass has three candidates per hit
                 * on average but a dozen on its busiest lane; walking them lane by lane, four per round, made the whole
                 * wave wait three to four load round trips for its busiest lane (the candidate walk with its queue
                 * traffic is 3.4 of the search's 4.5 ms, -DVOTE_DIAG_NOCAND; the list form took 0.25 ms of it:
                 * profiles/r03_ab_search_candidates.txt). */
                uint32_t incl = cnt;
                for (int o = 1; o < WAVE; o <<= 1) {
                    const uint32_t up = __shfl_up(incl, o, WAVE);
                    if (lane >= o) incl += up;
                }
                const uint32_t excl = incl - cnt, total = readlane_u(incl, WAVE - 1);
                const uint32_t hit0 = hit - (uint32_t)lane;                     /* the pass's first hit */
                for (uint32_t base = 0; base < total; base += 4u * WAVE) {
                    uint32_t kk[4], own[4], w[4];
                    bool inl[4];
    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t f = base + (uint32_t)u * WAVE + (uint32_t)lane;
                        inl[u] = f < total;
                        kk[u] = own[u] = w[u] = 0;
                        if (base + (uint32_t)u * WAVE >= total) continue;      /* wave-uniform: nothing left for this round */
                        /* every ds_bpermute below is executed by all 64 lanes (a lane that is switched off cannot be read
                         * from): no lane-dependent condition around them */
                        uint32_t o = 0;                                         /* the owner of list position f: running sum <= f */
    #pragma unroll
                        for (uint32_t s2 = WAVE / 2; s2 > 0; s2 >>= 1) o += bperm(o + s2 - 1u, incl) <= f ? s2 : 0u;
                        o = o < (uint32_t)WAVE - 1u ? o : (uint32_t)WAVE - 1u;
                        const uint32_t no = bperm(o, n), d0o = bperm(o, d0), exo = bperm(o, excl), sbo = bperm(o, sbase);
                        uint32_t k = d0o + (f - exo);
                        k = k >= no ? k - no : k;
                        k = k < no ? k : 0u;                                    /* a damaged directory (flagged above) must not become a wild load */
                        own[u] = o;
                        kk[u] = inl[u] ? sbo + k : 0u;
                        w[u] = pw[kk[u]];
                    }
    #pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (base + (uint32_t)u * WAVE >= total) continue;      /* wave-uniform */
                        const uint32_t Ao = bperm(own[u], A);
                        const bool near = inl[u] && w[u] * 30u - Ao < PC_T24_EDGE;
                        const unsigned long long nm = __ballot(near);
                        if (nm) sq_n = slow_push((lds_ctx *)sc, (lds_u32 *)acc, (lds_u32 *)s_tbl, (lds_u64 *)sq, sq_n, nm, kk[u] | SLOW_VERIFY, (hit0 + own[u]) | (1u << SLOW_HIT_BITS), lane);
                    }
                }
            }
#ifdef VOTE_PROF
            prof_corr += clock64() - pc0;
#endif
        };
        auto marked = [&](const uint2 &ru, const uint2 &inf) -> bool { return MODE == 0 && ((inf.y | ru.y) >> 31); };

        /* ---- the sets, one after the other (one call site of vote_set: its vote loops exist once) ----
         * giants first: 64 queued items at a time, their units dealt round-robin to the waves;
         * then the rest, dynamically: VOTE_BLOCK runs at a time from a counter in LDS.  Four blocks sit side by
         * side in the lanes of B_ru / B_inf (block b in lanes 16 * (b's turn mod 4) ..): the one being voted, the
         * next (its bucket records in flight) and the one after it (its run records in flight) */
        {
            /* The last VOTE_TAIL_RUNS runs can be handed out in blocks of VOTE_TAIL instead of VOTE_BLOCK, so that the waves
             * reach the barrier behind the votes closer together (a wave waits there for half a block's time on average:
             * 7 % of the kernel, profiles/r03_k_vote_phases_and_diag_builds.txt).  Off by default (VOTE_TAIL_RUNS 0):
             * blocks of 8 and of 4 at the end cost more in block overhead than they save at the barrier
             * (profiles/r03_ab_tail_blocks_fine_directory.txt). */
            const uint32_t tail_runs = n_runs < VOTE_TAIL_RUNS ? n_runs : VOTE_TAIL_RUNS;
            const uint32_t n_big = (n_runs - tail_runs) / VOTE_BLOCK;
            const uint32_t n_blocks = n_big + (n_runs - n_big * VOTE_BLOCK + VOTE_TAIL - 1) / VOTE_TAIL;
            auto block_first = [&](uint32_t b) -> uint32_t { return b < n_big ? b * VOTE_BLOCK : n_big * VOTE_BLOCK + (b - n_big) * VOTE_TAIL; };
            auto block_len = [&](uint32_t b) -> uint32_t { return b < n_big ? (uint32_t)VOTE_BLOCK : (uint32_t)VOTE_TAIL; };
            const uint32_t my_slot = (uint32_t)lane / VOTE_BLOCK, k_in = (uint32_t)lane % VOTE_BLOCK;
            auto grab = [&]() -> uint32_t {
                uint32_t b = 0;
                if (lane == 0) b = atomicAdd(&s_next, 1u);
                return uni_u32(readlane_u(b, 0));
            };
            /* run records of block b into the lanes of `slot` (zeros past the end of the run list) */
            auto fetch_runs = [&](uint32_t b, uint32_t slot) {
                if (my_slot == slot) {
                    const uint32_t k = block_first(b) + k_in;
                    B_ru = make_uint2(0, 0);
                    B_inf = make_uint2(0, 0);
                    if (k_in < block_len(b) && k < n_runs) {
                        const oslamk_run rr = runs[k];
                        B_ru = make_uint2(rr.slot_r, rr.first);
                    }
                }
            };
            /* bucket records of the block in `slot` (its run records have landed) */
            auto fetch_info = [&](uint32_t b, uint32_t slot) {
                if (my_slot == slot && k_in < block_len(b) && block_first(b) + k_in < n_runs) {
                    const oslamk_uinfo ui = uinfo[B_ru.x & RUN_SLOT_MASK];
                    B_inf = make_uint2(ui.start, ui.len);
                }
            };
            uint32_t cur_b = 0, nx1_b = 0, nx2_b = 0, turn = 0;
            uint32_t tw = 0;                                 /* giants: first queue entry of the next set */
            bool started = false;
            for (;;) {
                bool take, split;
                uint32_t u0, stride;
                if (tw < n_q) {
                    const uint32_t t = tw + (uint32_t)lane;
                    B_ru = make_uint2(0, 0);
                    B_inf = make_uint2(0, 0);
                    if (t < n_q) {
                        const oslamk_run rr = runs[s_q[t]];
                        const oslamk_uinfo ui = uinfo[rr.slot_r & RUN_SLOT_MASK];
                        B_ru = make_uint2(rr.slot_r, rr.first);
                        B_inf = make_uint2(ui.start, ui.len);
                    }
                    tw += WAVE;
                    take = t < n_q;
                    split = true;
                    u0 = uni_u32((uint32_t)wid);
                    stride = VOTE_THREADS / WAVE;
                } else {
                    if (!started) {                          /* the first three blocks of this wave */
                        started = true;
                        cur_b = grab();
                        fetch_runs(cur_b, 0u);
                        nx1_b = grab();
                        fetch_runs(nx1_b, 1u);
                        nx2_b = grab();
                        fetch_runs(nx2_b, 2u);
                        fetch_info(cur_b, 0u);
                        fetch_info(nx1_b, 1u);
                    }
                    if (cur_b >= n_blocks) break;            /* the counter only grows: this wave is done */
                    const uint32_t ln = B_inf.y & 0x7fffffffu, R = (B_ru.x >> OSLAMK_RUN_SHIFT) + 1u;
                    /* of the current block: present in the slice, not a giant (those are done), no marker (those come last) */
                    take = my_slot == (turn & 3u) && ln != 0u && ((ln + 255u) >> 8) * R <= T && !marked(B_ru, B_inf);
                    split = false;
                    u0 = 0u;
                    stride = 1u;
                    /* the next blocks move up before the votes, so that their loads fly meanwhile */
                    cur_b = nx1_b;
                    nx1_b = nx2_b;
                    fetch_info(nx1_b, (turn + 2u) & 3u);
                    nx2_b = grab();
                    fetch_runs(nx2_b, (turn + 3u) & 3u);
                    turn++;
                }
                vote_set(take, split, u0, stride);
#ifndef VOTE_DIAG_NOCORRECT          /* timing-only build: exact mode without the near-edge search */
                if (MODE == 0 && cq < n_cq) correct_pass();
#endif
            }
        }
#ifndef VOTE_DIAG_NOCORRECT
        if (MODE == 0) {
            while (cq < n_cq) correct_pass();
#ifdef VOTE_PROF
            if (lane == 0) atomicAdd(&a.counters->prof[3], (unsigned long long)prof_corr);    /* the near-edge search (inside the voting time) */
#endif
        }
#endif
        if (MODE == 0) {
            /* the items with a marker, dealt round-robin to the waves: every vote through the queue */
            for (uint32_t k0 = (uint32_t)wid * WAVE; k0 < n_runs; k0 += VOTE_THREADS) {
                const uint32_t k = k0 + (uint32_t)lane;
                oslamk_run rr;
                oslamk_uinfo ui;
                rr.slot_r = rr.first = 0;
                ui.start = ui.len = 0;
                if (k < n_runs) {
                    rr = runs[k];
                    ui = uinfo[rr.slot_r & RUN_SLOT_MASK];
                }
                unsigned long long fm = __ballot((ui.len & 0x7fffffffu) != 0u && ((ui.len | rr.first) >> 31));
                while (fm) {
                    const int j = __ffsll((long long)fm) - 1;
                    fm &= fm - 1ull;
                    sq_n = forced_item((lds_ctx *)sc, (lds_u32 *)acc, (lds_u32 *)s_tbl, (lds_u64 *)sq, sq_n, readlane_u(ui.start, j),
                                       readlane_u(ui.len, j) & 0x7fffffffu, readlane_u(rr.first, j) & 0x7fffffffu,
                                       (readlane_u(rr.slot_r, j) >> OSLAMK_RUN_SHIFT) + 1u, lane);
                }
            }
            if (sq_n) slow_queue_flush((lds_ctx *)sc, (lds_u32 *)acc, (lds_u32 *)s_tbl, (lds_u64 *)sq, sq_n, lane);
        }
#ifdef VOTE_PROF
        const long long pt1 = clock64();
#endif
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      /* the atomics issued from asm (VoteRegs::vote) */
        __syncthreads();
#ifdef VOTE_PROF
        const long long pt2 = clock64();
        if (lane == 0) {             /* wave cycles: pre-scan (with zeroing), voting, wait at the barrier behind it */
            atomicAdd(&a.counters->prof[0], (unsigned long long)(ptA - pt0));
            atomicAdd(&a.counters->prof[1], (unsigned long long)(pt1 - ptA));
            atomicAdd(&a.counters->prof[2], (unsigned long long)(pt2 - pt1));
        }
#endif


        /* ---- peak extraction: local max, non-empty cells, sum, emission ---- */
        /* the two counters of word w: of the model points m_base + row and m_base + 1023 + row */
        auto lower_of = [&](uint32_t w) -> uint32_t { return pass == 0 ? w & 0xffffu : pass == 1 ? w : 0u; };
        auto upper_of = [&](uint32_t w) -> uint32_t { return pass == 0 ? w >> 16 : pass == 2 ? w : 0u; };
        uint32_t lmax = 0, nz = 0;
        unsigned long long sum = 0;
#pragma unroll 2
        for (int c = tid; c < ACC_REAL_CELLS; c += VOTE_THREADS) {
            const uint32_t w = acc[c], v0 = lower_of(w), v1 = upper_of(w);
            lmax = max(lmax, max(v0, v1));
            nz += (v0 != 0) + (v1 != 0);
            sum += (unsigned long long)v0 + v1;
        }
        lmax = wave_max_u32(lmax);
        nz = wave_sum_u32(nz);
        sum = wave_sum_u64(sum);
        if (lane == 0) {
            s_wave[wid] = lmax;
            s_wave2[wid] = nz;
            s_sum[wid] = sum;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t m = 0, n = 0;
            unsigned long long tot = 0;
            for (int w = 0; w < VOTE_THREADS / WAVE; w++) {
                m = s_wave[w] > m ? s_wave[w] : m;
                n += s_wave2[w];
                tot += s_sum[w];
            }
            /* every vote cast is in a counter unless a 16-bit counter overflowed */
            s_redo = pass == 0 && tot != s_tot[0] - s_ctx.dropped;
#if defined(VOTE_DIAG_NOLOOP) || defined(VOTE_DIAG_NOATOM)
            s_redo = 0;                 /* timing-only builds cast no votes: nothing to check */
#endif
            if (s_redo) {
                a.redo[atomicAdd(&a.counters->redo_count, 1u)] = wg;
                atomicAdd(&a.counters->redo_total, 1u);
            }
            if (!s_redo) {
                if (pass <= 1) {                /* once per workgroup */
                    /* hits are counted once per reference point */
                    const unsigned long long h = slice == 0 ? (unsigned long long)a.hit_count[ref_local] : 0ull;
                    if (h) atomicAdd(&a.counters->hits, h);
                    if (s_tot[0]) atomicAdd(&a.counters->votes, s_tot[0]);
                    if (s_tot[1]) {
                        atomicAdd(&a.counters->entries, s_tot[1] & 0xffffffffffull);
                        atomicAdd(&a.counters->items, s_tot[1] >> 40);
                    }
                }
                uint32_t g = a.fixed_gmax;
                if (g == 0) {
                    const uint32_t old = atomicMax(&a.counters->gmax, m);
                    g = old > m ? old : m;
                }
                if (n) atomicAdd(&a.counters->nonzero_cells, (unsigned long long)n);
                s_g = g;
                s_lmax = m;
            }
        }
        __syncthreads();
        if (s_redo) return;                         /* workgroup-uniform: k_vote_wide takes over */

        if (a.acc_dump && ref_ord == a.dump_ref) {
            uint32_t *dst = a.acc_dump + (size_t)m_base * OSLAMK_NBIN;
    #pragma unroll 2
        for (int c = tid; c < ACC_REAL_CELLS; c += VOTE_THREADS) {
                const uint32_t w = acc[c];
                const int cell = c / ACC_STRIDE * OSLAMK_NBIN + c % ACC_STRIDE;
                if (pass <= 1) dst[cell] = lower_of(w);
                if (pass != 1) dst[cell + (int)PC_ROWS_PER_HALF * OSLAMK_NBIN] = upper_of(w);
                if (ACC_STRIDE < OSLAMK_NBIN && c % ACC_STRIDE == ACC_STRIDE - 1) {      /* the dump's last column */
                    if (pass <= 1) dst[cell + 1] = 0;
                    if (pass != 1) dst[cell + 1 + (int)PC_ROWS_PER_HALF * OSLAMK_NBIN] = 0;
                }
            }
        }

        /* cells with count > thresh * g (model.cu:164-167; g <= final maximum, so
         * this is a superset that the host filters with the final maximum) */
        const float bound = a.thresh * (float)s_g;
        if ((float)s_lmax > bound) {                 /* workgroup-uniform */
            uint32_t cnt = 0;
    #pragma unroll 2
        for (int c = tid; c < ACC_REAL_CELLS; c += VOTE_THREADS) {
                const uint32_t w = acc[c];
                cnt += ((float)lower_of(w) > bound) + ((float)upper_of(w) > bound);
            }
            /* exclusive scan of cnt over the workgroup */
            uint32_t incl = cnt;
            for (int o = 1; o < WAVE; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o, WAVE);
                if (lane >= o) incl += up;
            }
            if (lane == WAVE - 1) s_wave[wid] = incl;
            __syncthreads();
            if (tid == 0) {
                uint32_t run = 0;
                for (int w = 0; w < VOTE_THREADS / WAVE; w++) {
                    const uint32_t v = s_wave[w];
                    s_wave[w] = run;
                    run += v;
                }
                s_base = atomicAdd(&a.counters->out_count, run);
            }
            __syncthreads();
            uint32_t pos = s_base + s_wave[wid] + incl - cnt;
    #pragma unroll 2
        for (int c = tid; c < ACC_REAL_CELLS; c += VOTE_THREADS) {
                const uint32_t w = acc[c];
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
                    const uint32_t v = hf ? upper_of(w) : lower_of(w);
                    if ((float)v > bound) {
                        if (pos < a.out_cap) {
                            oslamk_cell cell;
                            const uint32_t m_r = m_base + (uint32_t)hf * PC_ROWS_PER_HALF + (uint32_t)(c / ACC_STRIDE);
                            cell.code = ((unsigned long long)r << 32) | (unsigned long long)((m_r << 6) |
                                                                         (uint32_t)(c % ACC_STRIDE));
                            cell.count = v;
                            cell.pad = 0;
                            a.out[pos] = cell;
                        }
                        pos++;
                    }
                }
            }
        }
    }
}

#endif /* OSLAM_VOTE_BODY_INC */
