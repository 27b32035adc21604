// insider_posthoc.hpp — glm_interaction() (R/glm_interaction.R:2-30) on the resident data set: the residual
// R = X - U C of the blocks a caller subtracts, and per sample the two quantities the per-group regression needs,
// w_i = C r_i (K) and ss_i = ||r_i||^2, from ONE streaming pass over X (insider_posthoc.hpp + the host driver in
// insider_hip.hip, section "post-hoc interaction GLM").
//
// Tile arithmetic (one wave per 16 samples, 16 genes at a time; X is gene-major, lines of pitch ldn):
//   R^T tile:  D[gene j0 + g + 4r][sample m0 + c16] = X[gene][sample] - sum_k C[k][gene] U[sample][k]
//              on v_mfma_f64_16x16x4 with A = C^T (row = gene), B = -U (row = sample), the accumulator started at X
//              (g = lane >> 4, c16 = lane & 15; the accumulator layout D[(lane >> 4) + 4 r][lane & 15]).
//   w tile:    D2[latent 16 t + g + 4 r'][sample c16] += sum_{gene} C[latent][gene] R[sample][gene]: MFMA step r takes
//              the accumulator register r of the R^T tile as its B operand unchanged (its reduction index, the gene
//              g + 4 r, sits on lane >> 4 where the operand wants it): no lane movement, no LDS round trip.
//   ss:        sum of the squared accumulator registers, summed over the four lane groups at the end.
// C is staged per block in LDS in the operand order of both products (one conflict-free ds_read_b64 per MFMA operand,
// as k_mm_rows2 stages W): s1[tile][step s][lane] = C[4 s + (lane >> 4)][j0 + (lane & 15)] (first product),
// s2[tile][t][r][lane] = C[16 t + (lane & 15)][j0 + (lane >> 4) + 4 r] (second product).
#pragma once

namespace insider {

constexpr int PH_WPB = 8;   // waves (tiles of 16 samples) per block of the post-hoc streaming kernels

// C (K x p column-major, i.e. p rows of K) -> cp (p rows of KPW, zero padded); nz[k] = 1 when row k of C has a non-zero
// entry (an aliased latent dimension has none).  Integer flags: the result does not depend on the order of the updates.
// The flags are gathered per block in LDS first: at most KPW device atomics per block.  blockDim.x = 256.
__global__ void __launch_bounds__(256) k_ph_pack_c(const double *__restrict__ src, int64_t p, int K, int KPW,
                                                   double *__restrict__ cp, int *__restrict__ nz)
{
    __shared__ int s_nz[64];
    if (threadIdx.x < 64) s_nz[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < p * KPW) {
        const int64_t j = t / KPW;
        const int k = (int)(t % KPW);
        const double v = k < K ? src[j * K + k] : 0.0;
        cp[t] = v;
        if (v != 0.0) s_nz[k] = 1;   // every writer stores the same value
    }
    __syncthreads();
    if (threadIdx.x < KPW && s_nz[threadIdx.x]) atomicOr(&nz[threadIdx.x], 1);
}

// stage GT tiles of 16 genes starting at j1 (genes >= jend read as zero) in the operand order of the first product
// (s1) and, when s2 != nullptr, of the second
template <int NB, int GT>
__device__ __forceinline__ void ph_stage_c(const double *__restrict__ cp, int K, int64_t j1, int64_t jend, double *s1,
                                           double *s2)
{
    constexpr int KPW = 16 * NB, S1 = GT * 4 * NB * 64;
    for (int i = threadIdx.x; i < S1; i += blockDim.x) {
        const int ln = i & 63, s = (i >> 6) % (4 * NB), tt = i / (64 * 4 * NB);
        const int k = 4 * s + (ln >> 4);
        const int64_t j = j1 + 16 * tt + (ln & 15);
        s1[i] = (k < K && j < jend) ? cp[j * KPW + k] : 0.0;
    }
    if (s2) {
        for (int i = threadIdx.x; i < S1; i += blockDim.x) {
            const int ln = i & 63, r = (i >> 6) & 3, t = (i >> 8) % NB, tt = i / (256 * NB);
            const int k = 16 * t + (ln & 15);
            const int64_t j = j1 + 16 * tt + (ln >> 4) + 4 * r;
            s2[i] = (k < K && j < jend) ? cp[j * KPW + k] : 0.0;
        }
    }
}

// -U[row][4 s + g] for the steps s < 4 NB (U rows of KPW, zero beyond K)
template <int NB>
__device__ __forceinline__ void ph_load_u(const double *__restrict__ U, int row, int g, double (&bu)[4 * NB])
{
#pragma unroll
    for (int s = 0; s < 4 * NB; ++s) bu[s] = -U[(size_t)row * (16 * NB) + 4 * s + g];
}

// acc (started at the X tile) -= C^T U^T over the ks = ceil(K / 4) steps: the R^T tile
template <int NB>
__device__ __forceinline__ void ph_resid_tile(const double *s1t /* s1 of this gene tile + lane */, const double (&bu)[4 * NB],
                                              int ks, d4 &acc)
{
#pragma unroll
    for (int s = 0; s < 4 * NB; ++s)
        if (s < ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(s1t[s * 64], bu[s], acc, 0, 0, 0);
}

// Per-sample w_i = C r_i and ss_i = ||r_i||^2 over the genes of slab blockIdx.y ([y * slab_len, min(+slab_len, p))):
// part[(y * n + i) * (K + 1) + k] (k < K: w, k = K: ss).  grid = (ceil(ceil(n / 16) / PH_WPB), slabs); dynamic LDS
// 2 GT 4 NB 64 doubles.  slab_len is a multiple of 16 GT.  Every sum runs in a fixed order: no atomics.
template <int NB, int GT>
__global__ void __launch_bounds__(64 * PH_WPB) k_resid_stats(const double *__restrict__ X, int64_t ldn, int n, int64_t p,
                                                             const double *__restrict__ U, const double *__restrict__ cp,
                                                             int K, int64_t slab_len, double *__restrict__ part)
{
    extern __shared__ double s_c[];
    double *s1 = s_c, *s2 = s_c + GT * 4 * NB * 64;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, c16 = lane & 15;
    const int m0 = (blockIdx.x * PH_WPB + w) * 16;
    const bool active = m0 < n;   // wave-uniform; inactive waves still take part in the staging
    const int row = m0 + c16 < n ? m0 + c16 : n - 1;
    const int ks = (K + 3) >> 2;
    double bu[4 * NB];
    ph_load_u<NB>(U, row, g, bu);
    const int64_t jb = (int64_t)blockIdx.y * slab_len;
    const int64_t je = jb + slab_len < p ? jb + slab_len : p;
    d4 acc2[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) acc2[t] = d4{0.0, 0.0, 0.0, 0.0};
    double ssl = 0.0;
    for (int64_t j1 = jb; j1 < je; j1 += 16 * GT) {
        __syncthreads();   // the previous round's operands have been read
        ph_stage_c<NB, GT>(cp, K, j1, je, s1, s2);
        __syncthreads();
        if (!active) continue;
        d4 acc[GT];
#pragma unroll
        for (int tt = 0; tt < GT; ++tt)   // every X load of the round in flight before the first MFMA
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t j = j1 + 16 * tt + g + 4 * r;
                acc[tt][r] = j < je ? X[j * ldn + row] : 0.0;
            }
#pragma unroll
        for (int tt = 0; tt < GT; ++tt) {
            if (j1 + 16 * tt >= je) break;   // wave-uniform
            ph_resid_tile<NB>(s1 + tt * 4 * NB * 64 + lane, bu, ks, acc[tt]);
#pragma unroll
            for (int r = 0; r < 4; ++r) ssl += acc[tt][r] * acc[tt][r];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t = 0; t < NB; ++t)
                    acc2[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(s2[((tt * NB + t) * 4 + r) * 64 + lane], acc[tt][r],
                                                                   acc2[t], 0, 0, 0);
        }
    }
    if (!active) return;
    ssl += __shfl_xor(ssl, 16);
    ssl += __shfl_xor(ssl, 32);
    const int i = m0 + c16;
    if (i >= n) return;
    double *out = part + ((size_t)blockIdx.y * n + i) * (K + 1);
#pragma unroll
    for (int t = 0; t < NB; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 16 * t + g + 4 * r;
            if (k < K) out[k] = acc2[t][r];
        }
    if (g == 0) out[K] = ssl;
}

// Residual rows [rb, re) x genes [jb, je) -> out column-major (row i - rb, gene j - jb; leading dimension ldo).
// grid = (ceil(ceil((re - rb) / 16) / PH_WPB), ceil((je - jb) / (16 GT))); dynamic LDS GT 4 NB 64 doubles.
template <int NB, int GT>
__global__ void __launch_bounds__(64 * PH_WPB) k_resid_write(const double *__restrict__ X, int64_t ldn, int64_t rb,
                                                             int64_t re, const double *__restrict__ U,
                                                             const double *__restrict__ cp, int K, int64_t jb, int64_t je,
                                                             double *__restrict__ out, int64_t ldo)
{
    extern __shared__ double s_c[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, c16 = lane & 15;
    const int64_t m0 = rb + ((int64_t)blockIdx.x * PH_WPB + w) * 16;
    const int64_t j1 = jb + (int64_t)blockIdx.y * 16 * GT;
    ph_stage_c<NB, GT>(cp, K, j1, je, s_c, nullptr);
    __syncthreads();
    if (m0 >= re) return;   // wave-uniform, after the block's only barrier
    const int64_t i = m0 + c16;
    const int row = (int)(i < re ? i : re - 1);
    const int ks = (K + 3) >> 2;
    double bu[4 * NB];
    ph_load_u<NB>(U, row, g, bu);
    d4 acc[GT];
#pragma unroll
    for (int tt = 0; tt < GT; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t j = j1 + 16 * tt + g + 4 * r;
            acc[tt][r] = j < je ? X[j * ldn + row] : 0.0;
        }
#pragma unroll
    for (int tt = 0; tt < GT; ++tt) {
        if (j1 + 16 * tt >= je) break;
        ph_resid_tile<NB>(s_c + tt * 4 * NB * 64 + lane, bu, ks, acc[tt]);
        if (i < re) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t j = j1 + 16 * tt + g + 4 * r;
                if (j < je) out[(j - jb) * ldo + (i - rb)] = acc[tt][r];
            }
        }
    }
}

// Stage 1 of the per-group sums: one wave per chunk of <= PH_CHUNK members of one group (the chunks of a group are
// consecutive), lanes = columns of the per-sample statistics (ldw = K + 1 <= 64).  cpart[chunk][ldw].
constexpr int PH_CHUNK = 32;
__global__ void __launch_bounds__(256) k_ph_chunk_sums(const double *__restrict__ stats, int ldw,
                                                       const int *__restrict__ members, const int *__restrict__ ch_begin,
                                                       const int *__restrict__ ch_end, int nchunks,
                                                       double *__restrict__ cpart)
{
    const int ch = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (ch >= nchunks || lane >= ldw) return;
    const int b = ch_begin[ch], e = ch_end[ch];
    double s = 0.0;
#pragma unroll 8
    for (int q = b; q < e; ++q) s += stats[(size_t)members[q] * ldw + lane];
    cpart[(size_t)ch * ldw + lane] = s;
}

// Stage 2: gsum[grp][ldw] = sum of the group's chunks, four waves striding over them, combined in wave order.
__global__ void __launch_bounds__(256) k_ph_group_sums(const double *__restrict__ cpart, int ldw,
                                                       const int *__restrict__ grp_chunk, double *__restrict__ gsum)
{
    __shared__ double red[4][64];
    const int grp = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = grp_chunk[grp], e = grp_chunk[grp + 1];
    double s = 0.0;
    if (lane < ldw) {
#pragma unroll 4
        for (int ch = b + w; ch < e; ch += 4) s += cpart[(size_t)ch * ldw + lane];
    }
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && lane < ldw) gsum[(size_t)grp * ldw + lane] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// One wave: the Cholesky factor L of G = C C' reduced to the latent dimensions whose row of C is not zero
// (nz[k] != 0, kept in increasing order: rank r), and diag(G_r^-1).  A pivot that is not larger than r eps times its
// dimension's diagonal entry (singular to working precision) sets info[0] = 1 + its position.
//   L: r x r, pitch 64 (lower triangle); dinv: r; info[1] = r, info[2 + q] = latent index of reduced position q.
__global__ void __launch_bounds__(64) k_glm_factor(const double *__restrict__ Gm, const int *__restrict__ nz, int K,
                                                   double *__restrict__ Lout, double *__restrict__ dinv,
                                                   int *__restrict__ info)
{
    __shared__ double A[64][65];
    __shared__ double Xi[64][65];
    __shared__ int idx[64];
    __shared__ int s_r;
    const int lane = threadIdx.x;
    if (lane == 0) {
        int r = 0;
        for (int k = 0; k < K; ++k)
            if (nz[k]) idx[r++] = k;
        s_r = r;
    }
    __syncthreads();
    const int r = s_r;
    for (int i = 0; i < r; ++i) A[i][lane] = lane < r ? Gm[(size_t)idx[i] * K + idx[lane]] : 0.0;
    __syncthreads();
    const double tol = r * 2.220446049250313e-16;
    int bad = 0;
    for (int j = 0; j < r; ++j) {
        const double d = A[j][j];
        if (!(d > tol * Gm[(size_t)idx[j] * K + idx[j]])) { bad = j + 1; break; }   // uniform over the wave
        const double ljj = sqrt(d);
        __syncthreads();
        if (lane == j) A[j][j] = ljj;
        else if (lane > j && lane < r) A[lane][j] /= ljj;
        __syncthreads();
        if (lane > j && lane < r)
            for (int k = j + 1; k <= lane; ++k) A[lane][k] -= A[lane][j] * A[k][j];
        __syncthreads();
    }
    if (lane == 0) {
        info[0] = bad;
        info[1] = r;
    }
    if (lane < r) info[2 + lane] = idx[lane];
    if (bad) return;
    // column `lane` of L^-1 (rows lane .. r-1), and the sum of its squares = diag(G_r^-1)[lane]
    if (lane < r) {
        double x = 1.0 / A[lane][lane];
        Xi[lane][lane] = x;
        double d = x * x;
        for (int i = lane + 1; i < r; ++i) {
            double s = 0.0;
            for (int j = lane; j < i; ++j) s += A[i][j] * Xi[j][lane];
            x = -s / A[i][i];
            Xi[i][lane] = x;
            d += x * x;
        }
        dinv[lane] = d;
    }
    for (int i = 0; i < r; ++i)
        if (lane <= i) Lout[(size_t)i * 64 + lane] = A[i][lane];
}

// One wave per group: beta = G_r^-1 mean(w) (forward and back substitution with L, lane q = reduced dimension q),
// RSS = max(ss - m beta'mean(w), 0) (= ss - m beta' G beta; for residual rows in the row space of C the difference cancels
// to rounding noise of either sign, and a negative one is returned as 0: se = 0, not NaN), dof = m p - r,
// se = sqrt(RSS / dof diag(G_r^-1) / m).  Outputs G x K column-major (row grp); aliased dimensions NaN; an empty group
// gives zeros and dof 0.
__global__ void __launch_bounds__(64) k_glm_groups(const double *__restrict__ gsum, int ldw, const int *__restrict__ gptr,
                                                   int K, int64_t p, const int *__restrict__ nz, const double *__restrict__ L,
                                                   const double *__restrict__ dinv, const int *__restrict__ info, int G,
                                                   double *__restrict__ coeff, double *__restrict__ se,
                                                   double *__restrict__ dof)
{
    const int grp = blockIdx.x, lane = threadIdx.x;
    if (info[0]) return;
    const int r = info[1];
    const int m = gptr[grp + 1] - gptr[grp];
    if (m == 0) {
        if (lane < K) { coeff[grp + (size_t)lane * G] = 0.0; se[grp + (size_t)lane * G] = 0.0; }
        if (lane == 0) dof[grp] = 0.0;
        return;
    }
    const double nan = __builtin_nan("");
    if (lane < K && !nz[lane]) { coeff[grp + (size_t)lane * G] = nan; se[grp + (size_t)lane * G] = nan; }
    const int kq = lane < r ? info[2 + lane] : 0;
    const double wbar = lane < r ? gsum[(size_t)grp * ldw + kq] / m : 0.0;
    double b = wbar;
    for (int j = 0; j < r; ++j) {   // L y = wbar
        const double yj = __shfl(b, j) / L[(size_t)j * 64 + j];
        if (lane == j) b = yj;
        else if (lane > j && lane < r) b -= L[(size_t)lane * 64 + j] * yj;
    }
    for (int j = r - 1; j >= 0; --j) {   // L' beta = y
        const double bj = __shfl(b, j) / L[(size_t)j * 64 + j];
        if (lane == j) b = bj;
        else if (lane < j) b -= L[(size_t)j * 64 + lane] * bj;
    }
    double dot = lane < r ? b * wbar : 0.0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) dot += __shfl_xor(dot, o);
    const double diff = gsum[(size_t)grp * ldw + K] - m * dot;
    const double rss = diff < 0.0 ? 0.0 : diff;   // (the expanded form may cancel to a tiny negative sum: a sum of squares is not)
    const double dofv = (double)m * (double)p - r;
    if (lane < r) {
        coeff[grp + (size_t)kq * G] = b;
        se[grp + (size_t)kq * G] = sqrt(rss / dofv * dinv[lane] / m);
    }
    if (lane == 0) dof[grp] = dofv;
}

}  // namespace insider
