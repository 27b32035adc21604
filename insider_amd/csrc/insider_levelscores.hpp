// insider_levelscores.hpp — every sample scored against every level of one categorical covariate
// (insider_hip_level_scores; host driver in insider_hip.hip, section "level scores").
//
// For sample i, its selected genes S_i and candidate embeddings e_1 .. e_L (the rows of A[cov], or foreign rows),
//     sse[i][l] = sum_{j in S_i} (d_ij - e_l . C[:, j])^2,   d_ij = x_ij - u_{-cov}(i) . C[:, j],
// with u_{-cov}(i) the sum of the embeddings of every block but cov.  Expanded, with the candidate table Tc = cand C
// (gene-major, Tc[j][0 .. ldt), zero beyond L) and M the 0/1 selection,
//     sse = s0 - 2 P1 + P2,   s0[i] = sum_j M d^2,   P1 = (M .* d) Tc,   P2 = M (Tc .* Tc):
// two products whose contraction runs over the genes and whose output is sample x level, on v_mfma_f64_16x16x4 (operand
// map in insider_mm.hpp).
//
// k_ls_prod: a block of LS_WAVES waves owns 16 LS_WAVES consecutive samples, 16 per wave, one level window of at most QT
// tiles of 16 levels, and the genes of one slab, LS_GG = 16 at a time.  Lane (g = lane >> 4, t = lane & 15) reads sample t
// of its wave of the genes 4 s + g, s = 0 .. 3, of the group (X is gene-major: the 16 lanes of a group read 128 contiguous
// bytes), so product step s reduces over the genes 4 s + g.  The group's rows of the window of Tc and its rows of C (in the
// operand order of the fit) are staged in LDS and shared by the waves.
//   fit:  the 16 genes x 16 samples tile of u_{-cov} . C comes from the same instruction, A = C (row = gene), B = U_{-cov}
//         (row = sample, the lane's 4 KS values kept in registers for the whole pass): D[(lane >> 4) + 4 r][t] is gene
//         4 r + g of sample t — register r is exactly what the lane needs in product step r: no lane movement.  The
//         embedding U_{-cov} is k_build_R's (ph_prepare with every block but cov), so the fit costs the same whatever the
//         number of blocks, continuous columns or levels of the other covariates: no level table of the other blocks, no
//         register window over blocks, no LDS that grows with their level counts.
//   products: A = d (or the selection 1.0 / 0.0), B = Tc (or its square, formed on load), QT accumulator tiles each.
//   s0 and the count are summed per lane in gene order and across the four lanes of a sample at the end.
// One value per (sample, level) leaves the kernel: part[slab][i][l] = s0 - 2 P1 + P2 of the slab; k_ls_reduce sums the
// slabs in slab order: fixed order, no atomics.  With more than QT tiles of levels the grid's z runs over the windows (X
// is read once per window).
#pragma once

namespace insider {

constexpr int LS_WAVES = 4;              // waves per block of k_ls_prod: 16 samples each
constexpr int LS_TILE = 16 * LS_WAVES;   // samples per block
constexpr int LS_GG = 16;                // genes per staging step: one fit tile, four product steps
constexpr int LS_QT = 8;                 // level tiles per window at most (64 + 64 accumulator registers)

// the row pitch of the staged window of Tc: 16 (mod 32) doubles, so that the lane groups g and g + 1 of a 32-lane half
// (consecutive rows) fall on disjoint banks: one conflict-free ds_read_b64 per MFMA operand
constexpr int ls_pitch(int QT) { return QT % 2 ? 16 * QT : 16 * QT + 16; }
constexpr size_t ls_lds_bytes(int QT, int KS) { return ((size_t)LS_GG * ls_pitch(QT) + (size_t)4 * KS * 64) * sizeof(double); }

// grid = (ceil(n / LS_TILE), slabs, windows) blocks of 64 LS_WAVES threads; dynamic LDS ls_lds_bytes(QT, KS).  Slab y owns
// the genes [y slab_len, min(p, (y + 1) slab_len)) (never empty; a slab's last group may hold fewer than LS_GG genes).  Window z owns the
// columns [16 QT z, min(ldt, 16 QT (z + 1))) of Tc (p rows of ldt, ldt a multiple of 16).  U: n rows of 16 KS (zero beyond
// K), cp: p rows of 16 KS (zero beyond K).  sel_mask: 0 = every entry, else the code bit an entry must carry.  part holds
// slabs x n rows of ldt, cpart slabs x n counts (written by window 0).  ldn >= n.
template <int QT, int KS>
__global__ void __launch_bounds__(64 * LS_WAVES) k_ls_prod(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const double *__restrict__ U, const double *__restrict__ cp, int K, const double *__restrict__ Tc, int ldt,
    int sel_mask, int64_t slab_len, double *__restrict__ part, double *__restrict__ cpart)
{
    constexpr int WS = ls_pitch(QT), KPW = 16 * KS;
    extern __shared__ double s_ls[];
    double *s_t = s_ls, *s_c = s_ls + LS_GG * WS;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int i0 = (blockIdx.x * LS_WAVES + w) * 16;   // this wave's first sample
    const bool s_in = i0 + t < n;
    const int ic = s_in ? i0 + t : n - 1;              // (a sample beyond n reads the last one: never selected)
    const int col0 = blockIdx.z * 16 * QT;
    const int nt = (ldt - col0) / 16 < QT ? (ldt - col0) / 16 : QT;   // live tiles of this window (>= 1)
    const int ncol = 16 * nt;
    const int64_t jb = (int64_t)blockIdx.y * slab_len;
    const int64_t je = jb + slab_len < p ? jb + slab_len : p;
    const int ks4 = (K + 3) >> 2;
    double bu[4 * KS];   // B operand of the fit: U[sample t][4 s + g]
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s) bu[s] = U[(size_t)ic * KPW + 4 * s + g];
    d4 a1[QT], a2[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) a1[q] = a2[q] = d4{0.0, 0.0, 0.0, 0.0};
    double s0 = 0.0, cn = 0.0;
#pragma unroll 1
    for (int64_t g0 = jb; g0 < je; g0 += LS_GG) {
        // this lane's loads of the group are in flight while the block stages the operands (a gene beyond the slab reads
        // the slab's last gene: never selected)
        double x[4];
        uint32_t cd[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t j = g0 + 4 * s + g;
            const size_t line = (size_t)(j < je ? j : je - 1) * ldn + ic;
            x[s] = X[line];
            cd[s] = codes[line];
        }
        for (int e = threadIdx.x; e < LS_GG * ncol; e += 64 * LS_WAVES) {
            const int r = e / ncol, q = e % ncol;
            s_t[r * WS + q] = g0 + r < je ? Tc[(size_t)(g0 + r) * ldt + col0 + q] : 0.0;
        }
        for (int e = threadIdx.x; e < 4 * KS * 64; e += 64 * LS_WAVES) {   // s_c[step][lane] = C[4 step + (lane >> 4)][gene lane & 15]
            const int ln = e & 63, ks = e >> 6;
            const int64_t j = g0 + (ln & 15);
            s_c[e] = j < je ? cp[(size_t)j * KPW + 4 * ks + (ln >> 4)] : 0.0;
        }
        __syncthreads();
        d4 f = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 4 * KS; ++ks)
            if (ks < ks4) f = __builtin_amdgcn_mfma_f64_16x16x4f64(s_c[ks * 64 + lane], bu[ks], f, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool sel = s_in && g0 + 4 * s + g < je && (sel_mask == 0 || ((int)cd[s] & sel_mask));
            const double d = sel ? x[s] - f[s] : 0.0;
            const double m = sel ? 1.0 : 0.0;
            s0 = fma(d, d, s0);
            cn += m;
            const double *tr = s_t + (4 * s + g) * WS + t;
#pragma unroll
            for (int q = 0; q < QT; ++q)
                if (q < nt) {
                    const double b = tr[16 * q];
                    a1[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(d, b, a1[q], 0, 0, 0);
                    a2[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(m, b * b, a2[q], 0, 0, 0);
                }
        }
        __syncthreads();   // the next group overwrites the operands
    }
    // the four lanes of a sample, in a fixed order: every lane then holds the sums of sample t
    s0 += __shfl_xor(s0, 16); s0 += __shfl_xor(s0, 32);
    cn += __shfl_xor(cn, 16); cn += __shfl_xor(cn, 32);
    double sr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sr[r] = __shfl(s0, g + 4 * r);   // of sample g + 4 r, the row of accumulator register r
#pragma unroll
    for (int q = 0; q < QT; ++q)
        if (q < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = i0 + g + 4 * r;
                if (i < n)
                    part[((size_t)blockIdx.y * n + i) * ldt + col0 + 16 * q + t] = fma(-2.0, a1[q][r], sr[r] + a2[q][r]);
            }
        }
    if (blockIdx.z == 0 && g == 0 && s_in) cpart[(size_t)blockIdx.y * n + i0 + t] = cn;
}

// sse[l n + i] = max(0, sum over the slabs, in slab order, of part[slab][i][l]) (l < L; column-major, leading dimension n), and
// cnt[i] = the sum of the slabs' counts; one thread per (i, column of part), the columns fastest
__global__ void __launch_bounds__(256) k_ls_reduce(const double *__restrict__ part, const double *__restrict__ cpart,
                                                   int slabs, int64_t n, int ldt, int L, double *__restrict__ sse,
                                                   double *__restrict__ cnt)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * ldt) return;
    const int64_t i = t / ldt;
    const int l = (int)(t % ldt);
    if (l < L) {
        double v = part[t];
        for (int s = 1; s < slabs; ++s) v += part[(size_t)s * n * ldt + t];
        sse[(size_t)l * n + i] = v < 0.0 ? 0.0 : v;   // (the expanded form may cancel to a tiny negative sum: a sum of squares is not)
    }
    if (l == 0) {
        double v = cpart[i];
        for (int s = 1; s < slabs; ++s) v += cpart[(size_t)s * n + i];
        cnt[i] = v;
    }
}

}  // namespace insider
