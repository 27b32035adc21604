// ubench8.hip — how much code can a computed-jump table hold before the jumps start to miss the instruction cache on gfx950?
// N identical 128-byte blocks (6 independent v_fma_f64 + the scalar work that picks the next block) visited in a pseudo-random
// cyclic order (a full-period LCG on the block index, every wave from its own start), 3 waves per SIMD on every CU: time per jump
// against the table's footprint N x 128 B.  Behind DESIGN.md 9 (blocks of two coordinate steps: 62 KB of blocks did not pay).
// Second part (step6 / step5 below): the sweep kernel's step in its two shapes, 6 vector instructions against 5 + s_nop.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench8.hip -o tools/ubench8 && tools/ubench8      (tools/ubench8 steps: the step shapes only)
#include <hip/hip_runtime.h>
#include <cstdio>
#define STR_(x) #x
#define STR(x) STR_(x)
#define JUMPS 20000

#define BODY(N)                                                                                             \
    "s_getpc_b64 s[20:21]\n"                                                                                \
    "Lh%=:\n"                                                                                               \
    "s_add_u32 s20, s20, Lt%=-Lh%=\n"                                                                       \
    "s_addc_u32 s21, s21, 0\n"                                                                              \
    "s_add_u32 s28, s20, " STR(N) "*128\n"                                                                  \
    "s_addc_u32 s29, s21, 0\n"                                                                              \
    "s_mov_b32 s22, %[start]\n"                                                                             \
    "s_and_b32 s22, s22, " STR(N) "-1\n"                                                                    \
    "s_mov_b32 s23, " STR(JUMPS) "\n"                                                                       \
    "s_lshl_b32 s24, s22, 7\n"                                                                              \
    "s_add_u32 s26, s20, s24\n"                                                                             \
    "s_addc_u32 s27, s21, 0\n"                                                                              \
    "s_setpc_b64 s[26:27]\n"                                                                                \
    ".p2align 7\n"                                                                                          \
    "Lt%=:\n"                                                                                               \
    ".rept " STR(N) "\n"                                                                                    \
    "v_fma_f64 %[a0], %[x], %[y], %[a0]\n v_fma_f64 %[a1], %[x], %[y], %[a1]\n v_fma_f64 %[a2], %[x], %[y], %[a2]\n" \
    "v_fma_f64 %[a3], %[x], %[y], %[a3]\n v_fma_f64 %[a0], %[x], %[y], %[a0]\n v_fma_f64 %[a1], %[x], %[y], %[a1]\n" \
    "s_mul_i32 s22, s22, 5\n"                                                                               \
    "s_add_u32 s22, s22, 1\n"                                                                               \
    "s_and_b32 s22, s22, " STR(N) "-1\n"                                                                    \
    "s_lshl_b32 s24, s22, 7\n"                                                                              \
    "s_add_u32 s26, s20, s24\n"                                                                             \
    "s_addc_u32 s27, s21, 0\n"                                                                              \
    "s_sub_u32 s23, s23, 1\n"                                                                               \
    "s_cmp_eq_u32 s23, 0\n"                                                                                 \
    "s_cselect_b32 s26, s28, s26\n"      /* the last jump goes behind the table */                          \
    "s_cselect_b32 s27, s29, s27\n"                                                                         \
    "s_setpc_b64 s[26:27]\n"                                                                                \
    ".p2align 7\n"                                                                                          \
    ".endr\n"                                                                                               \
    "Le%=:\n"

#define KERNEL(N)                                                                                           \
    __global__ void __launch_bounds__(256) k##N(double seed, double *out)                                   \
    {                                                                                                       \
        double a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + threadIdx.x, x = 1e-9, y = 0.5;         \
        const int start = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 4 + (threadIdx.x >> 6)) * 2654435761u >> 7)); \
        asm volatile(BODY(N)                                                                                \
                     : [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2), [a3] "+v"(a3)                           \
                     : [x] "v"(x), [y] "v"(y), [start] "s"(start)                                           \
                     : "s20", "s21", "s22", "s23", "s24", "s26", "s27", "s28", "s29", "scc");                             \
        if (a0 + a1 + a2 + a3 == 12345.678) out[0] = 1;                                                     \
    }
KERNEL(32)
KERNEL(64)
KERNEL(128)
KERNEL(256)
KERNEL(512)
KERNEL(1024)
KERNEL(2048)

// ---- lean blocks: 2 VALU + 8 scalar instructions, like the sweep kernel's step; tables up to 64 KB, aligned to 64 KiB so that the
// block address is base_lo + offset without a carry (as the sweep kernel forms it) ----------------------------------------------
#define LBODY(N)                                                                                            \
    "s_getpc_b64 s[20:21]\n"                                                                                \
    "Lh%=:\n"                                                                                               \
    "s_add_u32 s20, s20, Lt%=-Lh%=\n"                                                                       \
    "s_addc_u32 s21, s21, 0\n"                                                                              \
    "s_add_u32 s28, s20, " STR(N) "*128\n"                                                                  \
    "s_mov_b32 s27, s21\n"                                                                                  \
    "s_mov_b32 s22, %[start]\n"                                                                             \
    "s_and_b32 s22, s22, " STR(N) "-1\n"                                                                    \
    "s_mov_b32 s23, " STR(JUMPS) "\n"                                                                       \
    "s_lshl_b32 s24, s22, 7\n"                                                                              \
    "s_add_u32 s26, s20, s24\n"                                                                             \
    "s_setpc_b64 s[26:27]\n"                                                                                \
    ".p2align 16\n"                                                                                         \
    "Lt%=:\n"                                                                                               \
    ".rept " STR(N) "\n"                                                                                    \
    "v_fma_f64 %[a0], %[x], %[y], %[a0]\n v_fma_f64 %[a1], %[x], %[y], %[a1]\n"                             \
    "s_mul_i32 s22, s22, 5\n"                                                                               \
    "s_add_u32 s22, s22, 1\n"                                                                               \
    "s_and_b32 s22, s22, " STR(N) "-1\n"                                                                    \
    "s_lshl_b32 s24, s22, 7\n"                                                                              \
    "s_add_u32 s26, s20, s24\n"                                                                             \
    "s_sub_u32 s23, s23, 1\n"                                                                               \
    "s_cselect_b32 s26, s28, s26\n"      /* SCC = borrow: the jump after the last one goes behind the table */ \
    "s_setpc_b64 s[26:27]\n"                                                                                \
    ".p2align 7\n"                                                                                          \
    ".endr\n"

#define LKERNEL(N)                                                                                          \
    __global__ void __launch_bounds__(256) l##N(double seed, double *out)                                   \
    {                                                                                                       \
        double a0 = seed, a1 = seed + threadIdx.x, x = 1e-9, y = 0.5;                                        \
        const int start = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 4 + (threadIdx.x >> 6)) * 2654435761u >> 7)); \
        asm volatile(LBODY(N)                                                                               \
                     : [a0] "+v"(a0), [a1] "+v"(a1)                                                         \
                     : [x] "v"(x), [y] "v"(y), [start] "s"(start)                                           \
                     : "s20", "s21", "s22", "s23", "s24", "s26", "s27", "s28", "scc");                      \
        if (a0 + a1 == 12345.678) out[0] = 1;                                                               \
    }
LKERNEL(16)
LKERNEL(32)
LKERNEL(64)
LKERNEL(128)
LKERNEL(256)
LKERNEL(512)

// ---- blocks of the sweep kernel's own step (insider_cd_reg.hpp), in its two shapes: what is one VALU instruction of the step worth? --
// 31 step blocks, 128 bytes apart, each ending in s_setpc_b64 on its own successor pair held in SGPRs (absolute addresses, as the
// kernel's round-5 list), and a 32nd control block (count down, leave or jump on): one cycle = one "sweep" of 31 steps in the order
// k -> 5 k + 1 mod 32.  Steps 0..15 work on slot 0 (h0, b0, i0), 16..30 on slot 1, owner lane k % 16, as in the kernel.
//   SHAPE 6: exec narrow | clamp, sub, fma (dn), beta -= dn | exec full | two DPP fmacs          (the step as it is)
//   SHAPE 5: exec narrow | clamp, sub, fma (dn_s)           | s_nop 0, exec full | two DPP fmacs  (beta updated once behind the sweep)
#define SWEEPS 4000
#define S_LO "0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15"
#define S_HI "0,1,2,3,4,5,6,7,8,9,10,11,12,13,14"   /* slot 1: coordinate 16 + k, owner lane k */
#define S_FMACS(DN, PB)                                                                                     \
    "v_fmac_f64_dpp %[h0], " DN ", %[g0] row_newbcast:\\k row_mask:0xf bank_mask:0xf\n"                     \
    "v_fmac_f64_dpp %[h1], " DN ", %[g1] row_newbcast:\\k row_mask:0xf bank_mask:0xf\n"                     \
    "s_setpc_b64 s[" PB "+2*\\k:" PB "+1+2*\\k]\n"
#define S_STEP6(H, B, I, PB)                                                                                   \
    ".p2align 7\n"                                                                                          \
    "s_lshl_b64 exec, %[lm], \\k\n"                                                                          \
    "v_max_f64 %[dn0], " H ", " H " clamp\n"                                                                \
    "v_add_f64 %[dn0], " H ", -%[dn0]\n"                                                                    \
    "v_fma_f64 %[dn0], -%[dn0], " I ", " B "\n"                                                             \
    "v_fmac_f64 " B ", -1.0, %[dn0]\n"                                                                      \
    "s_mov_b64 exec, -1\n" S_FMACS("%[dn0]", PB)
#define S_STEP5(H, B, I, DN, PB)                                                                               \
    ".p2align 7\n"                                                                                          \
    "s_lshl_b64 exec, %[lm], \\k\n"                                                                          \
    "v_max_f64 " DN ", " H ", " H " clamp\n"                                                                \
    "v_add_f64 " DN ", " H ", -" DN "\n"                                                                    \
    "v_fma_f64 " DN ", -" DN ", " I ", " B "\n"                                                             \
    "s_nop 0\n"                                                                                             \
    "s_mov_b64 exec, -1\n" S_FMACS(DN, PB)
#define SBODY(LO, HI, TAIL)                                                                                 \
    "s_getpc_b64 s[98:99]\n"                                                                                \
    "Lh%=:\n"                                                                                               \
    "s_add_u32 s98, s98, Lt%=-Lh%=\n"                                                                       \
    "s_addc_u32 s99, s99, 0\n"                                                                              \
    ".irp k,0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31\n"                                                                      \
    "s_add_u32 s[34+2*\\k], s98, ((5*\\k+1)&31)*128\n"                                                      \
    "s_addc_u32 s[35+2*\\k], s99, 0\n"                                                                      \
    ".endr\n"                                                                                               \
    "s_mov_b32 s33, " STR(SWEEPS) "\n"                                                                      \
    "s_setpc_b64 s[98:99]\n"                                                                                \
    ".p2align 8\n"                                                                                          \
    "Lt%=:\n"                                                                                               \
    ".irp k," S_LO "\n" LO ".endr\n"                                                                        \
    ".irp k," S_HI "\n" HI ".endr\n"                                                                        \
    ".p2align 7\n" TAIL                                                                                     \
    "s_sub_u32 s33, s33, 1\n"                                                                               \
    "s_cmp_eq_u32 s33, 0\n"                                                                                 \
    "s_cbranch_scc1 Le%=\n"                                                                                 \
    "s_setpc_b64 s[96:97]\n"                                                                                \
    "Le%=:\n"
#define S_CLOB "s33", "s34", "s35", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", \
    "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", \
    "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "s88", "s89", "s90", \
    "s91", "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99", "scc"
#define SKERNEL(NAME, LO, HI, TAIL)                                                                         \
    __global__ void __launch_bounds__(256) NAME(double seed, double *out)                                   \
    {                                                                                                       \
        double h0 = 0.25 + 1e-3 * threadIdx.x, h1 = 1.5 - h0, b0 = 0.1 * seed, b1 = -b0, i0 = 1e-3, i1 = 2e-3, g0 = 1e-3, g1 = -1e-3; \
        double dn0 = 0.0, dn1 = 0.0;                                                                        \
        const unsigned long long lm = 0x0001000100010001ull;                                               \
        asm volatile(SBODY(LO, HI, TAIL)                                                                    \
                     : [h0] "+v"(h0), [h1] "+v"(h1), [b0] "+v"(b0), [b1] "+v"(b1), [dn0] "+v"(dn0), [dn1] "+v"(dn1) \
                     : [i0] "v"(i0), [i1] "v"(i1), [g0] "v"(g0), [g1] "v"(g1), [lm] "s"(lm)                  \
                     : S_CLOB);                                                                             \
        if (h0 + h1 + b0 + b1 == 12345.678) out[0] = 1;                                                     \
    }
SKERNEL(step6, S_STEP6("%[h0]", "%[b0]", "%[i0]", "34"), S_STEP6("%[h1]", "%[b1]", "%[i1]", "66"), "")
SKERNEL(step5, S_STEP5("%[h0]", "%[b0]", "%[i0]", "%[dn0]", "34"), S_STEP5("%[h1]", "%[b1]", "%[i1]", "%[dn1]", "66"),
        "v_fmac_f64 %[b0], -1.0, %[dn0]\n v_fmac_f64 %[b1], -1.0, %[dn1]\n")

template <typename F>
void run_steps(F kern, const char *name, double *d)
{
    for (int wps : {1, 3, 4}) {
        float best = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            hipEvent_t e0, e1;
            (void)hipEventCreate(&e0);
            (void)hipEventCreate(&e1);
            (void)hipEventRecord(e0);
            hipLaunchKernelGGL(kern, dim3(256 * wps), dim3(256), 0, 0, 1.5, d);
            (void)hipEventRecord(e1);
            (void)hipDeviceSynchronize();
            float ms;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (rep > 0 && ms < best) best = ms;   // (the first launch warms up)
        }
        printf("%s  waves/SIMD %d: %.3f ms  %.2f ns per block per wave  %.2f ns per block per SIMD\n", name, wps, best,
               best * 1e6 / SWEEPS / 32, best * 1e6 / SWEEPS / 32 / wps);
    }
}

template <typename F>
void run(F kern, int n, double *d)
{
    for (int wps : {1, 3, 4}) {   // waves per SIMD (blocks of 4 waves: one per SIMD of a CU)
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        hipLaunchKernelGGL(kern, dim3(256 * wps), dim3(256), 0, 0, 1.5, d);
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL(kern, dim3(256 * wps), dim3(256), 0, 0, 1.5, d);
        (void)hipEventRecord(e1);
        (void)hipDeviceSynchronize();
        float ms;
        (void)hipEventElapsedTime(&ms, e0, e1);
        printf("blocks %4d = %6.1f KB  waves/SIMD %d: %.3f ms  %.1f ns per jump per wave  %.2f ns per jump per SIMD\n", n, n * 128 / 1024.0,
               wps, ms, ms * 1e6 / JUMPS, ms * 1e6 / JUMPS / wps);
    }
}

int main(int argc, char **)
{
    double *d;
    (void)hipMalloc(&d, 1 << 16);
    printf("blocks of the sweep kernel's step, 31 steps + 1 control block per cycle:\n");
    run_steps(step6, "6 VALU (beta updated in the step)  ", d);
    run_steps(step5, "5 VALU + s_nop (beta updated once) ", d);
    run_steps(step6, "6 VALU (again)                     ", d);
    run_steps(step5, "5 VALU + s_nop (again)             ", d);
    if (argc > 1) return 0;   // any argument: the step shapes only
    printf("lean blocks (2 VALU + 8 scalar instructions):\n");
    run(l16, 16, d);
    run(l32, 32, d);
    run(l64, 64, d);
    run(l128, 128, d);
    run(l256, 256, d);
    run(l512, 512, d);
    printf("blocks of 6 VALU + 10 scalar instructions:\n");
    run(k32, 32, d);
    run(k64, 64, d);
    run(k128, 128, d);
    run(k256, 256, d);
    run(k512, 512, d);
    run(k1024, 1024, d);
    run(k2048, 2048, d);
    return 0;
}
