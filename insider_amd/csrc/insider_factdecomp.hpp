// insider_factdecomp.hpp — per-factor decomposition of a fitted model on the resident data set
// (insider_hip_factor_decomposition; host driver in insider_hip.hip, section "factor decomposition").
//
// The record of insider_vardecomp.hpp split along the latent axis: block b (a covariate, or b = B, the total) has the
// per-sample embedding u_b(i) in R^K, factor k contributes h_{b,k}(i, j) = u_b(i)[k] C[k][j] through it, and for gene j and
// its selected entries S_j the record holds n_j, sum x, sum x^2, sum r^2 (r = x - sum_k h_{B,k}), then per (b, k)
// sum h, sum h^2, sum r h.  C[k][j] leaves every sum of gene j as a constant, so with W = [U_0 | ... | U_{B-1} | U_B]
// (n x (B + 1) K) and M_j the 0/1 selection of gene j the device forms three small products per gene,
//     P1_j = (M_j .* r_j)' W,   P2_j = M_j' W,   P3_j = M_j' (W .* W),
// on v_mfma_f64_16x16x4 (operand map in insider_mm.hpp), and k_fd_finish scales them by C[k][j] and C[k][j]^2.
//
// k_fd_build_w writes Wall = [W | W .* W] (rows padded with zeros to a multiple of FD_CHUNK, each half padded with zero
// columns to ldq, a multiple of 16).
//
// k_fd_prod: a block of FD_WAVES waves owns 16 FD_WAVES consecutive genes, 16 per wave, and walks the samples FD_CHUNK at
// a time.  The chunk's rows of the column window of Wall (16 QT columns) are staged in LDS and shared by the waves.  Lane
// (g = lane >> 4, t = lane & 15) reads four consecutive samples 16 s + 4 g .. + 3 of gene t of its wave (32 bytes of X, 4
// mask codes), so MFMA step e of a trip of 16 samples reduces over the samples 4 g + e: the staged rows follow the same map.
//   HEAVY: the fit of the 16 x 16 tile comes from the MFMA too, f = U_B C over K in steps of 4, with the rows of U_B
//   (staged beside the window) permuted so that D[(lane >> 4) + 4 e][t] is sample 4 g + e of gene t: the lane that holds x
//   holds f.  r = x - f on the selected entries and 0 elsewhere is the A operand of P1, and the base slots are summed per
//   lane in sample order and across the four lanes of a gene at the end.
//   LIGHT: the A operand is the selection itself (1.0 / 0.0), the window runs over both halves of Wall: P2 and P3.  Only the
//   mask codes are read.
// Every sum runs in a fixed order without atomics.  With more than QT tiles of 16 columns the pass runs again for the next
// window; the heavy pass needs the B K columns of the covariate blocks only (the total's sum h and sum r h are the sums over
// the blocks in block order, k_fd_finish), the light pass all of them (sum h_B^2 carries the cross terms between blocks).
#pragma once

namespace insider {

constexpr int FD_WAVES = 4;    // waves per block of k_fd_prod: 16 genes each
constexpr int FD_CHUNK = 32;   // samples staged per step (two trips of 16)
constexpr int FD_GENES = 16 * FD_WAVES;

// Wall[i][b K + k] = u_b(i)[k] (b < c: Ast row of the level; b = c with m > 0: sum_j z_ij B_c[j][k]; then the total, the sum in
// block order), Wall[i][ldq + q] = Wall[i][q]^2.  One thread per (i, k), i < n; Wall (rows x 2 ldq) was zeroed before.
__global__ void __launch_bounds__(256) k_fd_build_w(const int *__restrict__ lev /*c x n, 0-based*/,
                                                    const int *__restrict__ lvl_off, int c, int n,
                                                    const double *__restrict__ Ast, int KPW, const double *__restrict__ Zc,
                                                    int m, int SLcat, int K, int ldq, double *__restrict__ Wall)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n * K) return;
    const int i = (int)(t / K), k = (int)(t % K);
    double *w = Wall + (size_t)i * 2 * ldq;
    double tot = 0.0;
    for (int b = 0; b < c; ++b) {
        const double u = Ast[(size_t)(lvl_off[b] + lev[(size_t)b * n + i]) * KPW + k];
        w[b * K + k] = u;
        w[ldq + b * K + k] = u * u;
        tot += u;
    }
    int nb = c;
    if (m > 0) {
        double u = 0.0;
        for (int j = 0; j < m; ++j) u = fma(Zc[(size_t)j * n + i], Ast[(size_t)(SLcat + j) * KPW + k], u);
        w[c * K + k] = u;
        w[ldq + c * K + k] = u * u;
        tot += u;
        nb = c + 1;
    }
    w[nb * K + k] = tot;
    w[ldq + nb * K + k] = tot * tot;
}

// grid = ceil(p / FD_GENES) blocks of 64 FD_WAVES threads.  Window: the columns wcol0 .. wcol0 + 16 nt of Wall (row pitch ldw,
// nt <= QT live tiles); the products land in P[j][pcol0 ..) (row pitch ldp).  HEAVY: rcol = the first column of the total
// block in Wall, Cd = C as p rows of K, KS = ceil(K / 16), base = p x 4 (n_j, sum x, sum x^2, sum r^2; every window writes
// the same values).  sel_mask: 0 = every entry, else the code bit an entry must carry.  ldn is a multiple of CHUNK >= n, Wall
// has at least round_up(n, FD_CHUNK) rows.  Dynamic LDS: FD_CHUNK (16 QT + 4) doubles, + FD_CHUNK (16 KS + 2) when HEAVY.
template <int QT, int KS, bool HEAVY>
__global__ void __launch_bounds__(64 * FD_WAVES) k_fd_prod(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const double *__restrict__ Wall, int ldw, int wcol0, int nt, int rcol, const double *__restrict__ Cd, int K,
    int sel_mask, double *__restrict__ P, int ldp, int pcol0, double *__restrict__ base)
{
    constexpr int WS = 16 * QT + 4;   // row pitches of the staged operands: one conflict-free ds_read_b64 per MFMA
    constexpr int RS = 16 * KS + 2;
    extern __shared__ double s_fd[];
    double *s_w = s_fd, *s_r = s_fd + FD_CHUNK * WS;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int64_t jw = (int64_t)blockIdx.x * FD_GENES + 16 * w;   // this wave's first gene
    const bool gene_in = jw + t < p;
    const int64_t jl = gene_in ? jw + t : p - 1;                    // (a gene beyond p reads the last gene: never stored)
    const int sig = 4 * (t & 3) + (t >> 2);                          // the staged row of U_B behind A-operand row t
    const int K4 = (K + 3) & ~3;
    double cb[4 * KS];   // B operand of the fit: C[4 s + g][gene t]
    if constexpr (HEAVY) {
#pragma unroll
        for (int s = 0; s < 4 * KS; ++s) cb[s] = 4 * s + g < K ? Cd[(size_t)jl * K + 4 * s + g] : 0.0;
    }
    d4 acc[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
    double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    const int ncol = 16 * nt;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += FD_CHUNK) {
        // this lane's loads of the chunk are in flight while the block stages the operands
        double x[FD_CHUNK / 16][4];
        uint32_t cd[FD_CHUNK / 16];
#pragma unroll
        for (int s = 0; s < FD_CHUNK / 16; ++s) {
            const int is = i0 + 16 * s + 4 * g;
            cd[s] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) x[s][e] = 0.0;
            if (is < n) {   // (is + 3 < ldn: the line holds the four)
                const size_t line = (size_t)jl * ldn + is;
                cd[s] = *reinterpret_cast<const uint32_t *>(codes + line);
                if constexpr (HEAVY) {
                    const double2 lo = *reinterpret_cast<const double2 *>(X + line);
                    const double2 hi = *reinterpret_cast<const double2 *>(X + line + 2);
                    x[s][0] = lo.x; x[s][1] = lo.y; x[s][2] = hi.x; x[s][3] = hi.y;
                }
            }
        }
        for (int e = threadIdx.x; e < FD_CHUNK * ncol; e += 64 * FD_WAVES) {
            const int r = e / ncol, q = e % ncol;
            s_w[r * WS + q] = Wall[(size_t)(i0 + r) * ldw + wcol0 + q];
        }
        if constexpr (HEAVY) {
            for (int e = threadIdx.x; e < FD_CHUNK * K4; e += 64 * FD_WAVES) {
                const int r = e / K4, k = e % K4;
                s_r[r * RS + k] = Wall[(size_t)(i0 + r) * ldw + rcol + k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < FD_CHUNK / 16; ++s) {
            if (i0 + 16 * s >= n) continue;   // block-uniform
            double a[4];
            if constexpr (HEAVY) {
                d4 f = d4{0.0, 0.0, 0.0, 0.0};
                const double *rr = s_r + (16 * s + sig) * RS + g;
#pragma unroll
                for (int ks = 0; ks < 4 * KS; ++ks)
                    if (4 * ks < K4) f = __builtin_amdgcn_mfma_f64_16x16x4f64(rr[4 * ks], cb[ks], f, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int code = (int)(cd[s] >> (8 * e)) & 0xff;
                    const bool sel = gene_in && i0 + 16 * s + 4 * g + e < n && (sel_mask == 0 || (code & sel_mask));
                    const double xv = sel ? x[s][e] : 0.0;
                    a[e] = sel ? x[s][e] - f[e] : 0.0;
                    b0 += sel ? 1.0 : 0.0;
                    b1 += xv;
                    b2 = fma(xv, xv, b2);
                    b3 = fma(a[e], a[e], b3);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int code = (int)(cd[s] >> (8 * e)) & 0xff;
                    const bool sel = gene_in && i0 + 16 * s + 4 * g + e < n && (sel_mask == 0 || (code & sel_mask));
                    a[e] = sel ? 1.0 : 0.0;
                }
            }
            const double *wr = s_w + (16 * s + 4 * g) * WS + t;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < QT; ++q)
                    if (q < nt) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[e], wr[e * WS + 16 * q], acc[q], 0, 0, 0);
        }
        __syncthreads();   // the next chunk overwrites the operands
    }
#pragma unroll
    for (int q = 0; q < QT; ++q)
        if (q < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t j = jw + g + 4 * r;
                if (j < p) P[(size_t)j * ldp + pcol0 + 16 * q + t] = acc[q][r];
            }
        }
    if constexpr (HEAVY) {
        // the four lanes of a gene, in a fixed order
        b0 += __shfl_xor(b0, 16); b0 += __shfl_xor(b0, 32);
        b1 += __shfl_xor(b1, 16); b1 += __shfl_xor(b1, 32);
        b2 += __shfl_xor(b2, 16); b2 += __shfl_xor(b2, 32);
        b3 += __shfl_xor(b3, 16); b3 += __shfl_xor(b3, 32);
        if (g == 0 && gene_in) {
            double *o = base + (size_t)(jw + t) * 4;
            o[0] = b0; o[1] = b1; o[2] = b2; o[3] = b3;
        }
    }
}

// out record of gene j from P[j] = [P1 | P2 | P3] (three runs of ldq) and base[j]: one thread per (j, k).  For b < nb the
// slots at 4 + 3 (b K + k) are C[k][j] P2, C[k][j]^2 P3, C[k][j] P1; the total block b = nb sums the blocks' first and third
// slot in block order and takes its second from its own column of P3.  C[k][j] = 0 gives slots that are 0.
__global__ void __launch_bounds__(256) k_fd_finish(const double *__restrict__ P, int ldq, const double *__restrict__ base,
                                                   const double *__restrict__ Cd, int64_t p, int K, int nb,
                                                   double *__restrict__ out)
{
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= p * K) return;
    const int64_t j = tid / K;
    const int k = (int)(tid % K);
    const int rec = 4 + 3 * (nb + 1) * K;
    const double *pj = P + (size_t)j * 3 * ldq;
    double *o = out + (size_t)j * rec;
    if (k == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = base[(size_t)j * 4 + q];
    }
    const double cv = Cd[(size_t)j * K + k], cc = cv * cv;
    double th = 0.0, trh = 0.0;
    for (int b = 0; b < nb; ++b) {
        const int q = b * K + k;
        const double sh = cv * pj[ldq + q], srh = cv * pj[q];
        o[4 + 3 * q] = sh;
        o[5 + 3 * q] = cc * pj[2 * ldq + q];
        o[6 + 3 * q] = srh;
        th += sh;
        trh += srh;
    }
    const int q = nb * K + k;
    o[4 + 3 * q] = th;
    o[5 + 3 * q] = cc * pj[2 * ldq + q];
    o[6 + 3 * q] = trh;
}

}  // namespace insider
