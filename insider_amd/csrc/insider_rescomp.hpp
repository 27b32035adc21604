// insider_rescomp.hpp — the masked, standardised residual of a fitted model as an operator on a caller's block of vectors
// (insider_hip_residual_products; host driver in insider_hip.hip, section "residual products").
//
// With f = u(i) . C[:, j] the fit (u(i) the total per-sample embedding of k_build_R, every block subtracted), M the 0/1
// selection and, per gene, a centre c_j and an inverse scale s_j (0 for a gene whose scale is not finite or not > 0: an
// all-zero column),
//     r_ij = M_ij (x_ij - f_ij - c_j) s_j,
// the two thin products of one step of a subspace iteration on R, against Q (n x q, q <= 64, padded to QT tiles of 16
// columns) and on v_mfma_f64_16x16x4 (operand map in insider_mm.hpp):
//     Z = R' Q (p x q),  rss_j = sum_i r_ij^2     k_rc_back: a block owns genes and walks every sample,
//     Y = R Z  (n x q)                            k_rc_fwd + k_rc_reduce: sample tiles x gene slabs.
// R is never stored: each pass streams X and the mask codes once (9 bytes per entry) and forms the fit of a 16 x 16 tile
// with the same instruction, K deep, so a pass costs the same whatever the number of blocks, continuous columns or levels.
//
// k_rc_back: a block of RC_WAVES waves owns 16 RC_WAVES consecutive genes, 16 per wave, and walks the samples RC_CHUNK at
// a time; the chunk's rows of Q and of U are staged in LDS and shared by the waves.  Lane (g = lane >> 4, t = lane & 15)
// reads four consecutive samples 16 s + 4 g .. + 3 of gene t of its wave (32 bytes of X, 4 mask codes), so product step e
// of a trip of 16 samples reduces over the samples 4 g + e, and the staged rows of Q follow the same map.  The contraction
// of Z runs over the samples, so the lane's row index must be the gene: the fit is A = U (row = sample, permuted so that
// D[(lane >> 4) + 4 e][t] is sample 4 g + e of gene t), B = C (the lane's 4 KS values of gene t, in registers for the whole
// pass) — the layout of k_fd_prod.  A gene's products and its rss are summed in sample order inside one block: no partials.
//
// k_rc_fwd: the contraction of Y runs over the genes, so the lane's row index is the sample: the layout of k_ls_prod.  A
// block of RC_WAVES waves owns 16 RC_WAVES consecutive samples and the genes of one slab, RC_GG at a time; lane (g, t)
// reads sample t of its wave of the genes 4 s + g.  The fit is A = C (row = gene; the group's rows staged in LDS in operand
// order), B = U (row = sample, the lane's 4 KS values in registers): D[(lane >> 4) + 4 r][t] is gene 4 r + g of sample t,
// register r is what product step r needs.  The group's rows of Z are staged beside.  part[slab][i][0 .. 16 QT) leaves the
// kernel; k_rc_reduce sums the slabs in slab order: fixed order, no atomics.
#pragma once

namespace insider {

constexpr int RC_WAVES = 4;               // waves per block of both kernels
constexpr int RC_CHUNK = 32;              // k_rc_back: samples staged per step (two trips of 16)
constexpr int RC_GENES = 16 * RC_WAVES;   // k_rc_back: genes per block
constexpr int RC_TILE = 16 * RC_WAVES;    // k_rc_fwd: samples per block
constexpr int RC_GG = 16;                 // k_rc_fwd: genes per staging step: one fit tile, four product steps

// row pitches of the staged operands, one conflict-free ds_read_b64 per MFMA operand: k_rc_back reads rows 4 g + e at column t
// (pitch 4 mod 16) and the rows of U at column g (pitch 2 mod 16); k_rc_fwd reads rows 4 s + g at column t (16 mod 32)
constexpr int rc_back_pitch(int QT) { return 16 * QT + 4; }
constexpr int rc_u_pitch(int KS) { return 16 * KS + 2; }
constexpr int rc_fwd_pitch(int QT) { return QT % 2 ? 16 * QT : 16 * QT + 16; }
constexpr size_t rc_back_lds(int QT, int KS) { return (size_t)RC_CHUNK * (rc_back_pitch(QT) + rc_u_pitch(KS)) * sizeof(double); }
constexpr size_t rc_fwd_lds(int QT, int KS) { return ((size_t)RC_GG * rc_fwd_pitch(QT) + (size_t)4 * KS * 64) * sizeof(double); }

// cs[2 j] = center[j] (0 without one), cs[2 j + 1] = 1 / scale[j] (1 without one; 0 when scale[j] is not finite or not > 0)
__global__ void __launch_bounds__(256) k_rc_center_scale(const double *__restrict__ center, const double *__restrict__ scale,
                                                         int64_t p, double *__restrict__ cs)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= p) return;
    const double s = scale ? scale[j] : 1.0;
    cs[2 * j] = center ? center[j] : 0.0;
    cs[2 * j + 1] = (s > 0.0 && s < __builtin_inf()) ? 1.0 / s : 0.0;   // (NaN fails both comparisons)
}

// Qd[i][c] = Q[c n + i] (c < q; column-major in, n rows of ldq out, zero beyond q): one thread per (i, c), c fastest
__global__ void __launch_bounds__(256) k_rc_pack_q(const double *__restrict__ Q, int64_t n, int q, int ldq,
                                                   double *__restrict__ Qd)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * ldq) return;
    const int64_t i = t / ldq;
    const int c = (int)(t % ldq);
    Qd[t] = c < q ? Q[(size_t)c * n + i] : 0.0;
}

// out[c rows + r] = in[r ld + c] (c < q): the device rows as the caller's column-major matrix; one thread per (c, r), r fastest
__global__ void __launch_bounds__(256) k_rc_unpack(const double *__restrict__ in, int64_t rows, int q, int ld,
                                                   double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * q) return;
    const int64_t r = t % rows;
    const int c = (int)(t / rows);
    out[t] = in[(size_t)r * ld + c];
}

// grid = ceil(p / RC_GENES) blocks of 64 RC_WAVES threads; dynamic LDS rc_back_lds(QT, KS).  U: n rows of 16 KS (zero beyond
// K), cp: p rows of 16 KS (zero beyond K), Qd: n rows of 16 QT, cs: p pairs (centre, inverse scale).  sel_mask: 0 = every
// entry, else the code bit an entry must carry.  ldn is a multiple of 4 >= n.  Zd: p rows of 16 QT, rss: p.
template <int QT, int KS>
__global__ void __launch_bounds__(64 * RC_WAVES) k_rc_back(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const double *__restrict__ U, const double *__restrict__ cp, int K, const double *__restrict__ Qd,
    const double *__restrict__ cs, int sel_mask, double *__restrict__ Zd, double *__restrict__ rss)
{
    constexpr int WS = rc_back_pitch(QT), RS = rc_u_pitch(KS), LDQ = 16 * QT, KPW = 16 * KS;
    extern __shared__ double s_rc[];
    double *s_w = s_rc, *s_r = s_rc + RC_CHUNK * WS;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int64_t jw = (int64_t)blockIdx.x * RC_GENES + 16 * w;   // this wave's first gene
    const bool gene_in = jw + t < p;
    const int64_t jl = gene_in ? jw + t : p - 1;                    // (a gene beyond p reads the last gene: never stored)
    const int sig = 4 * (t & 3) + (t >> 2);                          // the staged row of U behind A-operand row t
    const int K4 = (K + 3) & ~3;
    double cb[4 * KS];   // B operand of the fit: C[4 s + g][gene t]
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s) cb[s] = cp[(size_t)jl * KPW + 4 * s + g];
    const double cen = cs[2 * jl], inv = cs[2 * jl + 1];
    d4 acc[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
    double ss = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += RC_CHUNK) {
        // this lane's loads of the chunk are in flight while the block stages the operands
        double x[RC_CHUNK / 16][4];
        uint32_t cd[RC_CHUNK / 16];
#pragma unroll
        for (int s = 0; s < RC_CHUNK / 16; ++s) {
            const int is = i0 + 16 * s + 4 * g;
            cd[s] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) x[s][e] = 0.0;
            if (is < n) {   // (is + 3 < ldn: the line holds the four)
                const size_t line = (size_t)jl * ldn + is;
                cd[s] = *reinterpret_cast<const uint32_t *>(codes + line);
                const double2 lo = *reinterpret_cast<const double2 *>(X + line);
                const double2 hi = *reinterpret_cast<const double2 *>(X + line + 2);
                x[s][0] = lo.x; x[s][1] = lo.y; x[s][2] = hi.x; x[s][3] = hi.y;
            }
        }
        for (int e = threadIdx.x; e < RC_CHUNK * LDQ; e += 64 * RC_WAVES) {
            const int r = e / LDQ, q = e % LDQ;
            s_w[r * WS + q] = i0 + r < n ? Qd[(size_t)(i0 + r) * LDQ + q] : 0.0;
        }
        for (int e = threadIdx.x; e < RC_CHUNK * K4; e += 64 * RC_WAVES) {
            const int r = e / K4, k = e % K4;
            s_r[r * RS + k] = i0 + r < n ? U[(size_t)(i0 + r) * KPW + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < RC_CHUNK / 16; ++s) {
            if (i0 + 16 * s >= n) continue;   // block-uniform
            d4 f = d4{0.0, 0.0, 0.0, 0.0};
            const double *rr = s_r + (16 * s + sig) * RS + g;
#pragma unroll
            for (int ks = 0; ks < 4 * KS; ++ks)
                if (4 * ks < K4) f = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[4 * ks], cb[ks], f, 0, 0, 0);
            double a[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int code = (int)(cd[s] >> (8 * e)) & 0xff;
                const bool sel = gene_in && i0 + 16 * s + 4 * g + e < n && (sel_mask == 0 || (code & sel_mask));
                a[e] = sel ? (x[s][e] - f[e] - cen) * inv : 0.0;
                ss = fma(a[e], a[e], ss);
            }
            const double *wr = s_w + (16 * s + 4 * g) * WS + t;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < QT; ++q)
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], wr[e * WS + 16 * q], acc[q], 0, 0, 0);
        }
        __syncthreads();   // the next chunk overwrites the operands
    }
#pragma unroll
    for (int q = 0; q < QT; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t j = jw + g + 4 * r;
            if (j < p) Zd[(size_t)j * LDQ + 16 * q + t] = acc[q][r];
        }
    }
    // the four lanes of a gene, in a fixed order
    ss += __shfl_xor(ss, 16); ss += __shfl_xor(ss, 32);
    if (g == 0 && gene_in) rss[jw + t] = ss;
}

// grid = (ceil(n / RC_TILE), slabs) blocks of 64 RC_WAVES threads; dynamic LDS rc_fwd_lds(QT, KS).  Slab y owns the genes
// [y slab_len, min(p, (y + 1) slab_len)) (never empty; a slab's last group may hold fewer than RC_GG genes).  Zd: p rows of
// 16 QT; U, cp, cs, sel_mask as in k_rc_back.  part holds slabs x n rows of 16 QT.  ldn >= n.
template <int QT, int KS>
__global__ void __launch_bounds__(64 * RC_WAVES) k_rc_fwd(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const double *__restrict__ U, const double *__restrict__ cp, int K, const double *__restrict__ Zd,
    const double *__restrict__ cs, int sel_mask, int64_t slab_len, double *__restrict__ part)
{
    constexpr int WS = rc_fwd_pitch(QT), LDQ = 16 * QT, KPW = 16 * KS;
    extern __shared__ double s_rc[];
    double *s_t = s_rc, *s_c = s_rc + RC_GG * WS;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int i0 = (blockIdx.x * RC_WAVES + w) * 16;   // this wave's first sample
    const bool s_in = i0 + t < n;
    const int ic = s_in ? i0 + t : n - 1;              // (a sample beyond n reads the last one: never selected)
    const int64_t jb = (int64_t)blockIdx.y * slab_len;
    const int64_t je = jb + slab_len < p ? jb + slab_len : p;
    const int ks4 = (K + 3) >> 2;
    double bu[4 * KS];   // B operand of the fit: U[sample t][4 s + g]
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s) bu[s] = U[(size_t)ic * KPW + 4 * s + g];
    d4 acc[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int64_t g0 = jb; g0 < je; g0 += RC_GG) {
        // this lane's loads of the group are in flight while the block stages the operands (a gene beyond the slab reads
        // the slab's last gene: never selected)
        double x[4], cen[4], inv[4];
        uint32_t cd[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t j = g0 + 4 * s + g;
            const int64_t jc = j < je ? j : je - 1;
            const size_t line = (size_t)jc * ldn + ic;
            x[s] = X[line];
            cd[s] = codes[line];
            cen[s] = cs[2 * jc];
            inv[s] = cs[2 * jc + 1];
        }
        for (int e = threadIdx.x; e < RC_GG * LDQ; e += 64 * RC_WAVES) {
            const int r = e / LDQ, q = e % LDQ;
            s_t[r * WS + q] = g0 + r < je ? Zd[(size_t)(g0 + r) * LDQ + q] : 0.0;
        }
        for (int e = threadIdx.x; e < 4 * KS * 64; e += 64 * RC_WAVES) {   // s_c[step][lane] = C[4 step + (lane >> 4)][gene lane & 15]
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
            const double d = sel ? (x[s] - f[s] - cen[s]) * inv[s] : 0.0;
            const double *tr = s_t + (4 * s + g) * WS + t;
#pragma unroll
            for (int q = 0; q < QT; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(d, tr[16 * q], acc[q], 0, 0, 0);
        }
        __syncthreads();   // the next group overwrites the operands
    }
#pragma unroll
    for (int q = 0; q < QT; ++q) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + g + 4 * r;
            if (i < n) part[((size_t)blockIdx.y * n + i) * LDQ + 16 * q + t] = acc[q][r];
        }
    }
}

// Y[c n + i] = the sum over the slabs, in slab order, of part[slab][i][c] (c < q; column-major, leading dimension n); one
// thread per (i, column of part), the columns fastest
__global__ void __launch_bounds__(256) k_rc_reduce(const double *__restrict__ part, int slabs, int64_t n, int ldq, int q,
                                                   double *__restrict__ Y)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * ldq) return;
    const int64_t i = t / ldq;
    const int c = (int)(t % ldq);
    if (c >= q) return;
    double v = part[t];
    for (int s = 1; s < slabs; ++s) v += part[(size_t)s * n * ldq + t];
    Y[(size_t)c * n + i] = v;
}

}  // namespace insider
