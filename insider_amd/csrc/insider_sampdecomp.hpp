// insider_sampdecomp.hpp — per-sample fit diagnostics of a fitted model on the resident data set
// (insider_hip_sample_decomposition; host driver in insider_hip.hip, section "sample decomposition").
//
// The record of insider_vardecomp.hpp along the other axis: for sample i and its selected entries S_i, with the same terms
// g_b(i, j), f = sum_b g_b (block order) and r = x - f, one record of 4 + 3 B doubles: n_i, sum x, sum x^2, sum r^2, then per
// block sum g_b, sum g_b^2, sum r g_b, all over the genes j in S_i.  The level table T = [A_stack; B_c] C (gene-major) is the
// one the per-gene call builds.
//
// k_sd_stats: X and the codes are gene-major (lines of ldn samples), so the lanes run along the samples: a block of
// SD_WAVES waves owns SD_TILE consecutive samples, SD_SPL per lane (one 16-byte X load and one 2-byte code load per lane and
// gene, 1 KiB contiguous per wave), and walks the genes of its slab, SD_GU genes' loads in flight at a time.  A lane keeps
// the stacked level ids of its samples (the first SD_CREG categorical blocks) and their z (the first SD_MREG continuous
// columns) in registers for the whole pass; blocks and columns beyond those are re-read per gene from lev / Zc (cache
// resident: SD_TILE entries per block).  The record is summed in registers in gene order.  A gene's terms come from its
// table T[j][.]: the tables of `gg` genes at a time are staged in LDS and shared by the block's waves (STAGED), or, when
// SD_GU tables do not fit the budget, read from global memory (L2-resident) — the same arithmetic in the same order, so the
// same bits.  Grid: sample tiles x gene slabs; every slab writes its partial records part[slab][i][R] and k_sd_reduce sums
// them in slab order: fixed order, no atomics.  Blocks are accumulated BW at a time; with B > BW the pass runs again for
// the next window (the base slots are recomputed identically and rewritten).
#pragma once

namespace insider {

constexpr int SD_WAVES = 4;   // waves per block of k_sd_stats
constexpr int SD_SPL = 2;     // consecutive samples per lane
constexpr int SD_GU = 4;      // genes whose loads are issued together
constexpr int SD_CREG = 8;    // categorical blocks whose level ids a lane keeps in registers
constexpr int SD_MREG = 4;    // continuous columns whose z a lane keeps in registers
constexpr int SD_TILE = 64 * SD_WAVES * SD_SPL;   // samples per block
constexpr int SD_GROUP_MAX = 64;                  // genes per staging step at most

// grid = (ceil(n / SD_TILE), slabs) blocks of 64 SD_WAVES threads; dynamic LDS gg SL doubles when STAGED (none otherwise, and
// gg = slab_len: one group).  Slab y owns the genes [y slab_len, min(p, (y + 1) slab_len)) (never empty).  sel_mask: 0 = every
// entry, else the code bit an entry must carry.  Blocks b0 .. b0 + BW - 1 are accumulated; part holds slabs x n records of
// R = 4 + 3 BW doubles.  ldn is even and >= n, so the two-sample loads of a lane with a sample < n never leave the line.
template <int BW, bool STAGED>
__global__ void __launch_bounds__(64 * SD_WAVES) k_sd_stats(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const int *__restrict__ lev /*c x n, 0-based*/, const int *__restrict__ lvl_off, int c,
    const double *__restrict__ Zc /*m x n*/, int m, int SLcat, const double *__restrict__ T, int SL, int sel_mask,
    int b0, int64_t slab_len, int gg, double *__restrict__ part)
{
    constexpr int R = 4 + 3 * BW;
    extern __shared__ double s_tab[];
    const int i0 = blockIdx.x * SD_TILE + (int)threadIdx.x * SD_SPL;
    const bool live = i0 < n;   // (a lane without samples only helps staging)
    const int64_t jb = (int64_t)blockIdx.y * slab_len;
    const int64_t je = jb + slab_len < p ? jb + slab_len : p;
    bool in[SD_SPL];
    int ic[SD_SPL], id[SD_SPL][SD_CREG];
    double z[SD_SPL][SD_MREG];
#pragma unroll
    for (int s = 0; s < SD_SPL; ++s) {
        in[s] = i0 + s < n;
        ic[s] = in[s] ? i0 + s : n - 1;
#pragma unroll
        for (int b = 0; b < SD_CREG; ++b) id[s][b] = b < c ? lvl_off[b] + lev[(size_t)b * n + ic[s]] : 0;
#pragma unroll
        for (int k = 0; k < SD_MREG; ++k) z[s][k] = k < m ? Zc[(size_t)k * n + ic[s]] : 0.0;
    }
    double acc[SD_SPL][R];
#pragma unroll
    for (int s = 0; s < SD_SPL; ++s)
#pragma unroll
        for (int q = 0; q < R; ++q) acc[s][q] = 0.0;
    for (int64_t g0 = jb; g0 < je; g0 += gg) {
        const int ng = (int)(je - g0 < gg ? je - g0 : gg);   // genes of this group (>= 1)
        if constexpr (STAGED) {
            for (int t = threadIdx.x; t < ng * SL; t += blockDim.x) s_tab[t] = T[(size_t)g0 * SL + t];
            __syncthreads();
        }
        auto tab = [&](int gl, int s) -> double {
            if constexpr (STAGED) return s_tab[gl * SL + s];
            else return T[(size_t)(g0 + gl) * SL + s];
        };
        if (live)
            for (int q0 = 0; q0 < ng; q0 += SD_GU) {
                double2 x[SD_GU];
                uint32_t cd[SD_GU];
#pragma unroll
                for (int u = 0; u < SD_GU; ++u) {   // every load of the step in flight before the arithmetic (a gene beyond
                                                    // the group reads the group's last gene: it is never accumulated)
                    const int gl = q0 + u < ng ? q0 + u : ng - 1;
                    const size_t line = (size_t)(g0 + gl) * ldn + i0;
                    x[u] = *reinterpret_cast<const double2 *>(X + line);
                    cd[u] = *reinterpret_cast<const uint16_t *>(codes + line);
                }
#pragma unroll
                for (int u = 0; u < SD_GU; ++u) {
                    const bool gv = q0 + u < ng;
                    const int gl = gv ? q0 + u : ng - 1;
#pragma unroll
                    for (int s = 0; s < SD_SPL; ++s) {
                        double f = 0.0, gb[BW];
#pragma unroll
                        for (int t = 0; t < BW; ++t) gb[t] = 0.0;
                        auto term = [&](int b, double g) {   // f = g_0 + g_1 + ... in block order
                            f += g;
#pragma unroll
                            for (int t = 0; t < BW; ++t)
                                if (b == b0 + t) gb[t] = g;
                        };
#pragma unroll
                        for (int b = 0; b < SD_CREG; ++b)
                            if (b < c) term(b, tab(gl, id[s][b]));
                        for (int b = SD_CREG; b < c; ++b) term(b, tab(gl, lvl_off[b] + lev[(size_t)b * n + ic[s]]));
                        if (m > 0) {
                            double gc = 0.0;
#pragma unroll
                            for (int k = 0; k < SD_MREG; ++k)
                                if (k < m) gc = fma(z[s][k], tab(gl, SLcat + k), gc);
                            for (int k = SD_MREG; k < m; ++k) gc = fma(Zc[(size_t)k * n + ic[s]], tab(gl, SLcat + k), gc);
                            term(c, gc);
                        }
                        const int code = (int)(cd[u] >> (8 * s)) & 0xff;
                        const bool sel = in[s] && gv && (sel_mask == 0 || (code & sel_mask));
                        const double xs = s == 0 ? x[u].x : x[u].y;
                        const double xv = sel ? xs : 0.0;
                        const double r = sel ? xs - f : 0.0;
                        acc[s][0] += sel ? 1.0 : 0.0;
                        acc[s][1] += xv;
                        acc[s][2] = fma(xv, xv, acc[s][2]);
                        acc[s][3] = fma(r, r, acc[s][3]);
#pragma unroll
                        for (int t = 0; t < BW; ++t) {
                            const double g = sel ? gb[t] : 0.0;
                            acc[s][4 + 3 * t] += g;
                            acc[s][5 + 3 * t] = fma(g, g, acc[s][5 + 3 * t]);
                            acc[s][6 + 3 * t] = fma(r, g, acc[s][6 + 3 * t]);
                        }
                    }
                }
            }
        if constexpr (STAGED) __syncthreads();   // the next group overwrites the tables
    }
#pragma unroll
    for (int s = 0; s < SD_SPL; ++s)
        if (in[s]) {
            double *o = part + ((size_t)blockIdx.y * n + (i0 + s)) * R;
#pragma unroll
            for (int q = 0; q < R; ++q) o[q] = acc[s][q];
        }
}

// out[i][slot] = sum over the slabs, in slab order, of part[slab][i][q]; one thread per (i, q), q < R = 4 + 3 BW of the pass
// that accumulated blocks b0 .. (slots of blocks >= nblk are not written); out holds n records of 4 + 3 nblk doubles
__global__ void __launch_bounds__(256) k_sd_reduce(const double *__restrict__ part, int slabs, int64_t n, int R, int nblk,
                                                   int b0, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * R) return;
    const int64_t i = t / R;
    const int q = (int)(t % R);
    if (q >= 4 && b0 + (q - 4) / 3 >= nblk) return;
    double v = part[t];
    for (int s = 1; s < slabs; ++s) v += part[(size_t)s * n * R + t];
    out[(size_t)i * (4 + 3 * nblk) + (q < 4 ? q : q + 3 * b0)] = v;
}

}  // namespace insider
