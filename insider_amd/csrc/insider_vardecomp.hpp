// insider_vardecomp.hpp — per-gene variance decomposition of a fitted model on the resident data set
// (insider_hip_variance_decomposition; host driver in insider_hip.hip, section "variance decomposition").
//
// For gene j and its selected entries S_j, with g_b(i, j) the contribution of covariate block b to the fit, f = sum_b g_b
// and r = x - f, one record of 4 + 3 B doubles: n_j, sum x, sum x^2, sum r^2, then per block sum g_b, sum g_b^2,
// sum r g_b.  A categorical block's contribution depends on the sample only through its level, so the fit is never
// formed as a product per sample: the level table T = [A_stack; B_c] C (SL x p, stored gene-major: T[j][0..SL)) comes
// first (k_mm_rows), then ONE streaming pass over X and the mask codes reads g_b(i, j) = T[j][stacked level of i] per
// categorical block and g_c(i, j) = sum_k z_ik T[j][SLcat + k] for the continuous one.
//
// k_vd_stats: a block of VD_WAVES waves owns GW consecutive genes; its waves split the samples (VD_SPL consecutive samples
// per lane and trip: one 32-byte X load and one 4-byte code load per gene; the lines of X / codes are padded to ldn, a
// multiple of CHUNK, so the loads of a trip never leave the line).  The level ids and z of a sample are loaded once for all
// GW genes.  The GW tables are staged in LDS (STAGED) or, when they do not fit, read from global memory (L2-resident).
// Every lane sums its records in registers in sample order; a __shfl_xor butterfly and a sum over the waves in wave order
// end the pass: fixed order, no atomics.  Blocks are accumulated BW at a time; with B > BW the pass runs again for the
// next window (the base slots are recomputed identically and rewritten).
#pragma once

namespace insider {

constexpr int VD_WAVES = 4;   // waves per block of k_vd_stats
constexpr int VD_SPL = 4;     // consecutive samples per lane and trip

// grid = ceil(p / GW) blocks of 64 VD_WAVES threads; dynamic LDS GW SL doubles when STAGED (none otherwise).
// sel_mask: 0 = every entry, else the code bit an entry must carry.  Blocks b0 .. b0 + BW - 1 (those < nblk) are
// accumulated; out holds p records of 4 + 3 nblk doubles.
template <int BW, int GW, bool STAGED>
__global__ void __launch_bounds__(64 * VD_WAVES) k_vd_stats(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const int *__restrict__ lev /*c x n, 0-based*/, const int *__restrict__ lvl_off, int c,
    const double *__restrict__ Zc /*m x n*/, int m, int SLcat, const double *__restrict__ T, int SL, int sel_mask,
    int nblk, int b0, double *__restrict__ out)
{
    constexpr int R = 4 + 3 * BW;
    extern __shared__ double s_tab[];
    __shared__ double s_red[VD_WAVES][GW * R];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j0 = (int64_t)blockIdx.x * GW;
    const int ng = (int)(p - j0 < GW ? p - j0 : GW);   // genes of this block (>= 1)
    if constexpr (STAGED) {
        for (int t = threadIdx.x; t < ng * SL; t += blockDim.x) s_tab[t] = T[(size_t)j0 * SL + t];
        __syncthreads();
    }
    // table entry s of gene gl (a gene beyond p reads the block's last gene: its records are never stored)
    auto tab = [&](int gl, int s) -> double {
        const int gc = gl < ng ? gl : ng - 1;
        if constexpr (STAGED) return s_tab[gc * SL + s];
        else return T[(size_t)(j0 + gc) * SL + s];
    };
    double acc[GW][R];
#pragma unroll
    for (int gl = 0; gl < GW; ++gl)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[gl][q] = 0.0;
    for (int i0 = (w * 64 + lane) * VD_SPL; i0 < n; i0 += 64 * VD_WAVES * VD_SPL) {
        double x[GW][VD_SPL];
        uint32_t cd[GW];
#pragma unroll
        for (int gl = 0; gl < GW; ++gl) {   // every load of the trip in flight before the arithmetic
            const size_t line = (size_t)(j0 + (gl < ng ? gl : ng - 1)) * ldn + i0;
#pragma unroll
            for (int h = 0; h < VD_SPL / 2; ++h) {
                const double2 v = *reinterpret_cast<const double2 *>(X + line + 2 * h);
                x[gl][2 * h] = v.x;
                x[gl][2 * h + 1] = v.y;
            }
            if constexpr (VD_SPL == 4) cd[gl] = *reinterpret_cast<const uint32_t *>(codes + line);
            else cd[gl] = *reinterpret_cast<const uint16_t *>(codes + line);
        }
#pragma unroll
        for (int s = 0; s < VD_SPL; ++s) {
            const int i = i0 + s;
            const bool in = i < n;
            const int ic = in ? i : n - 1;
            double f[GW], gb[GW][BW];
#pragma unroll
            for (int gl = 0; gl < GW; ++gl) {
                f[gl] = 0.0;
#pragma unroll
                for (int t = 0; t < BW; ++t) gb[gl][t] = 0.0;
            }
            for (int b = 0; b < c; ++b) {   // f = g_0 + g_1 + ... in block order
                const int id = lvl_off[b] + lev[(size_t)b * n + ic];
#pragma unroll
                for (int gl = 0; gl < GW; ++gl) {
                    const double g = tab(gl, id);
                    f[gl] += g;
#pragma unroll
                    for (int t = 0; t < BW; ++t)
                        if (b == b0 + t) gb[gl][t] = g;
                }
            }
            if (m > 0) {
                double gc[GW];
#pragma unroll
                for (int gl = 0; gl < GW; ++gl) gc[gl] = 0.0;
                for (int k = 0; k < m; ++k) {
                    const double z = Zc[(size_t)k * n + ic];
#pragma unroll
                    for (int gl = 0; gl < GW; ++gl) gc[gl] = fma(z, tab(gl, SLcat + k), gc[gl]);
                }
#pragma unroll
                for (int gl = 0; gl < GW; ++gl) {
                    f[gl] += gc[gl];
#pragma unroll
                    for (int t = 0; t < BW; ++t)
                        if (c == b0 + t) gb[gl][t] = gc[gl];
                }
            }
#pragma unroll
            for (int gl = 0; gl < GW; ++gl) {
                const int code = (int)(cd[gl] >> (8 * s)) & 0xff;
                const bool sel = in && gl < ng && (sel_mask == 0 || (code & sel_mask));
                const double xv = sel ? x[gl][s] : 0.0;
                const double r = sel ? x[gl][s] - f[gl] : 0.0;
                acc[gl][0] += sel ? 1.0 : 0.0;
                acc[gl][1] += xv;
                acc[gl][2] = fma(xv, xv, acc[gl][2]);
                acc[gl][3] = fma(r, r, acc[gl][3]);
#pragma unroll
                for (int t = 0; t < BW; ++t) {
                    const double g = sel ? gb[gl][t] : 0.0;
                    acc[gl][4 + 3 * t] += g;
                    acc[gl][5 + 3 * t] = fma(g, g, acc[gl][5 + 3 * t]);
                    acc[gl][6 + 3 * t] = fma(r, g, acc[gl][6 + 3 * t]);
                }
            }
        }
    }
    // lanes (butterfly), then waves (in wave order)
#pragma unroll
    for (int gl = 0; gl < GW; ++gl)
#pragma unroll
        for (int q = 0; q < R; ++q) {
            double v = acc[gl][q];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) s_red[w][gl * R + q] = v;
        }
    __syncthreads();
    const int rec = 4 + 3 * nblk;
    for (int t = threadIdx.x; t < ng * R; t += blockDim.x) {
        const int gl = t / R, q = t % R;
        const int slot = q < 4 ? q : q + 3 * b0;
        if (q >= 4 && b0 + (q - 4) / 3 >= nblk) continue;
        double v = s_red[0][t];
#pragma unroll
        for (int ww = 1; ww < VD_WAVES; ++ww) v += s_red[ww][t];
        out[(size_t)(j0 + gl) * rec + slot] = v;
    }
}

}  // namespace insider
