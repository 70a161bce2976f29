// Microbenchmark: issue cost of the integer vector instructions the vote loop uses, gfx950.
// 16 waves per CU (4 per SIMD), each runs a dependent-free stream of N copies of one instruction.
// The "small patterns" rows are float instructions whose operands and results are all 32-bit patterns below 2^23 (zero
// or a denormal, worth n * 2^-149): exact integer arithmetic as long as f32 denormals are kept.  The program compares
// each of them bit for bit with the integer form it could replace and prints the number of differences.
#include <hip/hip_runtime.h>
#include <cstdio>
#define REP 64
#define ITER 2000
#define BODY(INSTR)                                                                                  \
    for (int i = 0; i < ITER; i++) {                                                                 \
        _Pragma("unroll") for (int k = 0; k < REP / 8; k++) {                                        \
            asm volatile(INSTR(0) INSTR(1) INSTR(2) INSTR(3) INSTR(4) INSTR(5) INSTR(6) INSTR(7)     \
                         : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]),   \
                           "+v"(r[6]), "+v"(r[7])                                                    \
                         : "v"(a), "v"(b));                                                          \
        }                                                                                            \
    }
#define I_MULHI24(n) "v_mul_hi_u32_u24 %" #n ", 0x1e00, %8\n"
#define I_MUL24(n) "v_mul_u32_u24 %" #n ", 0x1e00, %8\n"
#define I_MULHI32(n) "v_mul_hi_u32 %" #n ", %8, %9\n"
#define I_MULLO32(n) "v_mul_lo_u32 %" #n ", %8, %9\n"
#define I_SUB(n) "v_sub_u32 %" #n ", %8, %9\n"
#define I_LSHLADD(n) "v_lshl_add_u32 %" #n ", %8, 2, %9\n"
#define I_MIN3(n) "v_min3_u32 %" #n ", %8, %9, %" #n "\n"
#define I_MADU24(n) "v_mad_u32_u24 %" #n ", %8, %9, %" #n "\n"
#define I_MULF32(n) "v_mul_f32 %" #n ", %8, %9\n"
#define I_CVT(n) "v_cvt_f32_u32 %" #n ", %8\n"
#define I_FMA(n) "v_fma_f32 %" #n ", %8, %9, %" #n "\n"
#define I_MAD64(n) "v_mad_u64_u32 %" #n ", vcc, %8, %9, 0\n"
#define I_ADD(n) "v_add_u32 %" #n ", %8, %9\n"
#define I_LSHL(n) "v_lshlrev_b32 %" #n ", 2, %9\n"
#define I_AND(n) "v_and_b32 %" #n ", %8, %9\n"
#define I_MIN(n) "v_min_u32 %" #n ", %8, %9\n"
#define I_CNDMASK(n) "v_cndmask_b32 %" #n ", %8, %9, vcc\n"
#define I_CMP(n) "v_cmp_gt_u32 vcc, %8, %" #n "\n"
#define I_BFE(n) "v_bfe_u32 %" #n ", %8, 10, 1\n"
#define I_ADD3(n) "v_add3_u32 %" #n ", %8, %9, %" #n "\n"
#define I_READLANE(n) "v_readlane_b32 s20, %" #n ", 3\n"
#define I_MOV(n) "v_mov_b32 %" #n ", %8\n"
#define I_ADDLSHL(n) "v_add_lshl_u32 %" #n ", %8, %9, 2\n"
#define I_MAD64A(n) "v_mad_u64_u32 %" #n ", vcc, %8, 30, %" #n "\n"
// a = bin (0..30), b = row address, %10 = a scalar register with the literal (124.0 or 65535/1024)
#define I_FMA_ADDR(n) "v_fma_f32 %" #n ", %8, 4.0, %9\n"
#define I_MUL_ROW(n) "v_mul_f32 %" #n ", 0x42f80000, %8\n"
#define I_FMA_ROW(n) "v_fma_f32 %" #n ", %8, %10, %9\n"
#define I_FMA_INC(n) "v_fma_f32 %" #n ", %8, %10, 1\n"
#define I_FMAMK_ROW(n) "v_fmamk_f32 %" #n ", %8, 0x42f80000, %9\n"
#define I_SUB_S(n) "v_sub_u32 %" #n ", %10, %8\n"
#define I_MAX_F32(n) "v_max_f32 %" #n ", 1, %8\n"
#define BODY_S(INSTR, K)                                                                             \
    for (int i = 0; i < ITER; i++) {                                                                 \
        _Pragma("unroll") for (int k = 0; k < REP / 8; k++) {                                        \
            asm volatile(INSTR(0) INSTR(1) INSTR(2) INSTR(3) INSTR(4) INSTR(5) INSTR(6) INSTR(7)     \
                         : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]),   \
                           "+v"(r[6]), "+v"(r[7])                                                    \
                         : "v"(a), "v"(b), "s"(K));                                                  \
        }                                                                                            \
    }
template <int W>
__global__ __launch_bounds__(1024) void k(unsigned long long *cyc, uint32_t *sink)
{
    uint32_t r[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    uint32_t a = threadIdx.x * 2654435761u, b = threadIdx.x + 17;
    if (W == 24) { a = threadIdx.x % 31u; b = 64u + (threadIdx.x & 1023u) * 124u; }      /* bin, row address */
    if (W == 25 || W == 26 || W == 28) { a = threadIdx.x & 1023u; b = 64u; }                         /* row, accumulator base */
    if (W == 27) { a = (threadIdx.x & 1u) << 10; }                                        /* the half bit in place */
    __syncthreads();
    const long long t0 = clock64();
    if (W == 24) { BODY(I_FMA_ADDR) }
    if (W == 25) { BODY(I_MUL_ROW) }
    if (W == 26) { BODY_S(I_FMA_ROW, 0x42f80000u) }
    if (W == 27) { BODY_S(I_FMA_INC, 0x427fff00u) }
    if (W == 28) { BODY(I_FMAMK_ROW) }
    if (W == 29) { BODY_S(I_SUB_S, 0x12345678u) }
    if (W == 30) { BODY(I_MAX_F32) }
    if (W == 0) { BODY(I_MULHI24) }
    if (W == 1) { BODY(I_MUL24) }
    if (W == 2) { BODY(I_MULHI32) }
    if (W == 3) { BODY(I_MULLO32) }
    if (W == 4) { BODY(I_SUB) }
    if (W == 5) { BODY(I_LSHLADD) }
    if (W == 6) { BODY(I_MIN3) }
    if (W == 7) { BODY(I_MADU24) }
    if (W == 8) { BODY(I_MULF32) }
    if (W == 9) { BODY(I_CVT) }
    if (W == 10) { BODY(I_FMA) }
    if (W == 12) { BODY(I_ADD) }
    if (W == 13) { BODY(I_LSHL) }
    if (W == 14) { BODY(I_AND) }
    if (W == 15) { BODY(I_MIN) }
    if (W == 16) { for (int i = 0; i < ITER; i++) { _Pragma("unroll") for (int k = 0; k < REP / 8; k++) asm volatile(I_CNDMASK(0) I_CNDMASK(1) I_CNDMASK(2) I_CNDMASK(3) I_CNDMASK(4) I_CNDMASK(5) I_CNDMASK(6) I_CNDMASK(7) : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b) : "vcc"); } }
    if (W == 17) { for (int i = 0; i < ITER; i++) { _Pragma("unroll") for (int k = 0; k < REP / 8; k++) asm volatile(I_CMP(0) I_CMP(1) I_CMP(2) I_CMP(3) I_CMP(4) I_CMP(5) I_CMP(6) I_CMP(7) : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b) : "vcc"); } }
    if (W == 18) { BODY(I_BFE) }
    if (W == 19) { BODY(I_ADD3) }
    if (W == 20) { for (int i = 0; i < ITER; i++) { _Pragma("unroll") for (int k = 0; k < REP / 8; k++) asm volatile(I_READLANE(0) I_READLANE(1) I_READLANE(2) I_READLANE(3) I_READLANE(4) I_READLANE(5) I_READLANE(6) I_READLANE(7) : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]) : "v"(a), "v"(b) : "s20"); } }
    if (W == 21) { BODY(I_MOV) }
    if (W == 22) { BODY(I_ADDLSHL) }
    if (W == 23) {
        unsigned long long q[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        for (int i = 0; i < ITER; i++) {
#pragma unroll
            for (int k = 0; k < REP / 8; k++) {
                asm volatile(I_MAD64A(0) I_MAD64A(1) I_MAD64A(2) I_MAD64A(3) I_MAD64A(4) I_MAD64A(5) I_MAD64A(6) I_MAD64A(7)
                             : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7])
                             : "v"(a), "v"(b) : "vcc");
            }
        }
        r[0] += (uint32_t)(q[0] + q[1] + q[2] + q[3] + q[4] + q[5] + q[6] + q[7]);
    }
    if (W == 11) {
        unsigned long long q[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        for (int i = 0; i < ITER; i++) {
#pragma unroll
            for (int k = 0; k < REP / 8; k++) {
                asm volatile(I_MAD64(0) I_MAD64(1) I_MAD64(2) I_MAD64(3) I_MAD64(4) I_MAD64(5) I_MAD64(6) I_MAD64(7)
                             : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7])
                             : "v"(a), "v"(b) : "vcc");
            }
        }
        r[0] += (uint32_t)(q[0] + q[1] + q[2] + q[3] + q[4] + q[5] + q[6] + q[7]);
    }
    __syncthreads();
    const long long t1 = clock64();
    if (threadIdx.x == 0) cyc[blockIdx.x] = (unsigned long long)(t1 - t0);
    if (r[0] + r[1] + r[2] + r[3] + r[4] + r[5] + r[6] + r[7] == 0x1234567u) sink[0] = 1;
}
template <int W>
void run(const char *name, unsigned long long *d_cyc, uint32_t *d_sink)
{
    for (int rep = 0; rep < 2; rep++) { hipLaunchKernelGGL(k<W>, dim3(256), dim3(1024), 0, 0, d_cyc, d_sink); (void)hipDeviceSynchronize(); }
    unsigned long long h[256]; (void)hipMemcpy(h, d_cyc, sizeof h, hipMemcpyDeviceToHost);
    double s = 0; for (int i = 0; i < 256; i++) s += (double)h[i];
    s /= 256.0;
    // per SIMD: 4 waves x ITER x REP instructions
    printf("%-30s %6.2f cycles per wave-instruction per SIMD (4 waves per SIMD)\n", name, s / (4.0 * ITER * REP));
}
/* Every row, bin and half bit, at three accumulator bases: the float forms against the integer forms, bit for bit. */
__global__ void k_exact(uint32_t *diff)
{
    const uint32_t row = blockIdx.x, bin = threadIdx.x & 31u, base = (threadIdx.x >> 5) * 2048u;   /* 0, 2048, 4096, 6144 */
    if (bin > 30u) return;
    const uint32_t w = row | ((row & 1u) << 10) | (bin << 11);         /* an entry word: row, a half bit, bits above */
    uint32_t rowi, rowf, rowk, rowm, adi, adf, inci, incf, t;
    rowi = base + (w & 0x3ffu) * 124u;
    asm volatile("v_and_b32 %0, 0x3ff, %1\n\tv_fma_f32 %0, %0, %2, %3" : "=&v"(rowf) : "v"(w), "s"(0x42f80000u), "v"(base));
    asm volatile("v_and_b32 %0, 0x3ff, %1\n\tv_fmamk_f32 %0, %0, 0x42f80000, %2" : "=&v"(rowk) : "v"(w), "v"(base));
    asm volatile("v_and_b32 %0, 0x3ff, %1\n\tv_mul_f32 %0, 0x42f80000, %0" : "=&v"(rowm) : "v"(w));
    asm volatile("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(adi) : "v"(bin), "v"(rowi));
    asm volatile("v_fma_f32 %0, %1, 4.0, %2" : "=v"(adf) : "v"(bin), "v"(rowi));
    asm volatile("v_bfe_u32 %0, %1, 10, 1\n\tv_mad_u32_u24 %0, %0, %2, 1" : "=&v"(inci) : "v"(w), "s"(0xffffu));
    asm volatile("v_and_b32 %0, 0x400, %1\n\tv_fma_f32 %0, %0, %2, 1" : "=&v"(incf) : "v"(w), "s"(0x427fff00u));
    t = (rowi != rowf) + (rowi != rowk) + (rowm != (w & 0x3ffu) * 124u) + (adi != adf) + (inci != incf);
    if (inci != 1u && inci != 0x10000u) t++;
    if (t) atomicAdd(diff, t);
}
int main()
{
    unsigned long long *d_cyc; uint32_t *d_sink;
    (void)hipMalloc(&d_cyc, 256 * 8); (void)hipMalloc(&d_sink, 4);
    run<0>("v_mul_hi_u32_u24", d_cyc, d_sink);
    run<1>("v_mul_u32_u24", d_cyc, d_sink);
    run<2>("v_mul_hi_u32", d_cyc, d_sink);
    run<3>("v_mul_lo_u32", d_cyc, d_sink);
    run<4>("v_sub_u32", d_cyc, d_sink);
    run<5>("v_lshl_add_u32", d_cyc, d_sink);
    run<6>("v_min3_u32", d_cyc, d_sink);
    run<7>("v_mad_u32_u24", d_cyc, d_sink);
    run<8>("v_mul_f32", d_cyc, d_sink);
    run<9>("v_cvt_f32_u32", d_cyc, d_sink);
    run<10>("v_fma_f32", d_cyc, d_sink);
    run<11>("v_mad_u64_u32", d_cyc, d_sink);
    run<23>("v_mad_u64_u32 + vgpr addend", d_cyc, d_sink);
    run<12>("v_add_u32", d_cyc, d_sink);
    run<13>("v_lshlrev_b32", d_cyc, d_sink);
    run<14>("v_and_b32", d_cyc, d_sink);
    run<15>("v_min_u32", d_cyc, d_sink);
    run<16>("v_cndmask_b32", d_cyc, d_sink);
    run<17>("v_cmp_gt_u32", d_cyc, d_sink);
    run<18>("v_bfe_u32", d_cyc, d_sink);
    run<19>("v_add3_u32", d_cyc, d_sink);
    run<20>("v_readlane_b32", d_cyc, d_sink);
    run<21>("v_mov_b32", d_cyc, d_sink);
    run<22>("v_add_lshl_u32", d_cyc, d_sink);
    run<24>("v_fma_f32 bin * 4.0 + row address, small patterns", d_cyc, d_sink);
    run<25>("v_mul_f32 row * 124.0, small patterns", d_cyc, d_sink);
    run<26>("v_fma_f32 row * 124.0 (scalar register) + base, small patterns", d_cyc, d_sink);
    run<27>("v_fma_f32 x * 65535/1024 (scalar register) + 1, small patterns", d_cyc, d_sink);
    run<28>("v_fmamk_f32 row * 124.0 + base, small patterns", d_cyc, d_sink);
    run<29>("v_sub_u32, scalar register first", d_cyc, d_sink);
    run<30>("v_max_f32 with 1, small patterns", d_cyc, d_sink);
    (void)hipMemset(d_sink, 0, 4);
    hipLaunchKernelGGL(k_exact, dim3(1024), dim3(128), 0, 0, d_sink);
    uint32_t diff = 0;
    const hipError_t e = hipMemcpy(&diff, d_sink, 4, hipMemcpyDeviceToHost);
    printf("float forms against integer forms, 1024 rows x 31 bins x 4 bases: %u differences%s\n", diff, e == hipSuccess ? "" : " (copy failed)");
    return diff != 0 || e != hipSuccess;
}
