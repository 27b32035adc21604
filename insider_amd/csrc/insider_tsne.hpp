// insider_tsne.hpp — exact t-SNE of a neighbour graph on the device (insider_hip_tsne; host driver in insider_hip.hip, section
// "t-SNE").  include/insider_hip.h states the definitions; this file states how the device meets them.
//
// Dead points are COMPACTED AWAY on the host before the upload: the device sees the n = Na alive points under their compact
// numbers (the neighbour indices are renumbered with them), so no kernel tests for a dead point and every pair distance is
// finite.  The host scatters the results back and writes NaN for the dead.
//
// k_ts_calibrate: one thread per row, the fixed 100 bisection steps on H(beta); the row's k distances are re-read from
// global memory every step (the k-th of 64 stays in L1; the calibration is N k 100 exponentials once, against N^2 pair terms
// per iteration of the loop).  Sums run in slot order.  k_ts_joint gathers P_ij = (p_j|i + p_i|j) / (2 n) once: PF per forward
// slot (the mate slot of the reverse direction, if any, comes from the host's transpose), PR per reverse-only entry.
//
// k_ts_repulse, the hot path: grid (row tiles of 512, j-slabs), 256 threads, every lane owns TS_R = 2 rows for the whole
// kernel (two independent reciprocal chains per staged point, four with the unrolled loop).  The slab's y_j go through LDS
// 1024 points (16 KB) at a time; all lanes read the same address (a broadcast, no bank conflict).  Per pair, plain fp64
// VALU: dx, dy as differences, d = fma(dx, dx, fma(dy, dy, 1)), w = 1 / d by v_rcp_f64 and two Newton steps (d >= 1 is
// finite: no special cases; the result is within 1 ulp, and exactly 1 for d = 1), then sw += w, fx = fma(w w, dx, fx),
// fy likewise.  The self pair is left out, not subtracted afterwards: its 1 would sit in every row's sum of w and cost the
// small w of a wide map their last bits.  Only a chunk that holds rows of the block's own tile can meet it (a block-uniform
// test per chunk): there the same loop runs with one compare and select per pair (w = 0 for j = i), every other chunk runs
// the bare loop.  part[slab][i] = (sw, fx, fy).
//
// k_ts_reduce adds a row's slabs in slab order into rep[i] and leaves one partial of sum_i sw per block (its 256 rows added
// in row order by one thread); k_ts_fold, one block, adds partials in a fixed order (thread t the partials t, t + 256, ...,
// thread 0 the 256 results in thread order): Z, and later the sums of the new coordinates and of the rows' KL terms.
//
// k_ts_step: 16 lanes per row (a hub's reverse list can be long).  Lane l takes the forward slots l, l + 16, ... and then the
// reverse-only entries l, l + 16, ... of the row; an xor butterfly over the 16 lanes adds the partial attractive sums and KL
// terms.  Lane 0 forms the gradient with Z and applies the gain / velocity / position update (no contraction: every product
// and sum is rounded as written).  A block of 16 rows leaves one partial (sum x, sum y, sum KL); k_ts_centre subtracts the
// mean of the folded sums and files the KL on recording iterations.
//
// No floating-point atomics anywhere and no kernel waits on another block: every sum has one order.
#pragma once

namespace insider {

constexpr int TS_MAX_K = 64;          // neighbours per row
constexpr int TS_MAX_SLABS = 64;
constexpr int TS_R = 2;               // rows per lane of k_ts_repulse
constexpr int TS_TILE = 256 * TS_R;   // rows per block
constexpr int TS_CHUNK = 1024;        // staged points per trip
constexpr int TS_BLOCKS = 2048;       // the grid size the library's choice of slabs aims at: eight blocks per compute unit, so
                                      // that the last blocks to finish leave little of the card idle
constexpr int TS_MIN_SLAB = 256;      // ... with at least this many points per slab
constexpr int TS_STEPS = 100;         // bisection steps of the calibration
constexpr int TS_ROWS = 16;           // rows per block of k_ts_step (16 lanes each)

// One thread per row i < n.  idx / d2: n x k, filled slots first.  beta[i]: the last beta (1 for a uniform row);
// pc[i][s] = p_s|i, 0 at open slots.
__global__ void __launch_bounds__(256) k_ts_calibrate(const int32_t *__restrict__ idx, const double *__restrict__ d2, int n, int k,
                                                      double perplexity, double *__restrict__ beta, double *__restrict__ pc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t *ri = idx + (size_t)i * k;
    const double *rd = d2 + (size_t)i * k;
    double *rp = pc + (size_t)i * k;
    int m = 0;
    while (m < k && ri[m] >= 0) ++m;
    for (int s = m; s < k; ++s) rp[s] = 0.0;
    if (m == 0) {
        beta[i] = 1.0;
        return;
    }
    if (perplexity >= (double)m) {
        const double u = 1.0 / (double)m;
        for (int s = 0; s < m; ++s) rp[s] = u;
        beta[i] = 1.0;
        return;
    }
    double dmin = rd[0];
    for (int s = 1; s < m; ++s) dmin = fmin(dmin, rd[s]);
    const double target = log(perplexity);
    double b = 1.0, lo = 0.0, hi = __builtin_inf();
#pragma unroll 1
    for (int step = 0; step < TS_STEPS; ++step) {
        double S = 0.0, T = 0.0;
        for (int s = 0; s < m; ++s) {
            const double d = rd[s] - dmin, e = exp(-b * d);
            S += e;
            T += d * e;
        }
        const double H = log(S) + b * T / S;
        if (H > target) {
            lo = b;
            b = hi == __builtin_inf() ? b * 2.0 : (b + hi) * 0.5;
        } else {
            hi = b;
            b = (lo + b) * 0.5;
        }
    }
    double S = 0.0;
    for (int s = 0; s < m; ++s) S += exp(-b * (rd[s] - dmin));
    for (int s = 0; s < m; ++s) rp[s] = exp(-b * (rd[s] - dmin)) / S;
    beta[i] = b;
}

// PF[e] = (pc[e] + pc[mate[e]]) / (2 n) per forward slot e < n k (mate < 0: the reverse direction is absent; open slots
// give 0), PR[e] = pc[ro_flat[e]] / (2 n) per reverse-only entry e < nro.
__global__ void __launch_bounds__(256) k_ts_joint(const double *__restrict__ pc, const int32_t *__restrict__ mate, int64_t nk,
                                                  const int32_t *__restrict__ ro_flat, int64_t nro, double two_n,
                                                  double *__restrict__ PF, double *__restrict__ PR)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nk) {
        const int32_t m = mate[e];
        PF[e] = (pc[e] + (m >= 0 ? pc[m] : 0.0)) / two_n;
    }
    if (e < nro) PR[e] = (0.0 + pc[ro_flat[e]]) / two_n;
}

// 1 / d for finite d >= 1: v_rcp_f64 and two Newton steps
__device__ __forceinline__ double ts_rcp(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(r, fma(-d, r, 1.0), r);
    return fma(r, fma(-d, r, 1.0), r);
}

// The cnt staged points against the TS_R rows of a lane.  SELF: the chunk holds rows of this block; self[r] is the place of
// row r in it (anything outside 0..cnt-1 when it is not there) and that one pair counts w = 0.
template <bool SELF>
__device__ __forceinline__ void ts_pairs(const double2 *s_y, int cnt, const double (&xi)[TS_R], const double (&yi)[TS_R],
                                         const int (&self)[TS_R], double (&sw)[TS_R], double (&fx)[TS_R], double (&fy)[TS_R])
{
#pragma unroll 4
    for (int e = 0; e < cnt; ++e) {
        const double2 yj = s_y[e];
#pragma unroll
        for (int r = 0; r < TS_R; ++r) {
            const double dx = xi[r] - yj.x, dy = yi[r] - yj.y;
            double w = ts_rcp(fma(dx, dx, fma(dy, dy, 1.0)));
            if (SELF) w = e == self[r] ? 0.0 : w;
            const double w2 = w * w;
            sw[r] += w;
            fx[r] = fma(w2, dx, fx[r]);
            fy[r] = fma(w2, dy, fy[r]);
        }
    }
}

// grid = (ceil(n / TS_TILE), slabs), 256 threads.  Slab s covers the points [s slab_len, min(n, (s + 1) slab_len)) (possibly
// none).  part[(s n + i) 3 ..] = (sum w, sum w^2 dx, sum w^2 dy) of row i over the slab's points j != i in ascending index.
__global__ void __launch_bounds__(256) k_ts_repulse(const double2 *__restrict__ Y, int n, int slab_len, double *__restrict__ part)
{
    __shared__ double2 s_y[TS_CHUNK];
    const int tid = threadIdx.x;
    const int row0 = blockIdx.x * TS_TILE;
    const int64_t j0 = (int64_t)blockIdx.y * slab_len;
    const int j1 = (int)(j0 + slab_len < n ? j0 + slab_len : n);
    double xi[TS_R], yi[TS_R], sw[TS_R], fx[TS_R], fy[TS_R];
#pragma unroll
    for (int r = 0; r < TS_R; ++r) {
        const int i = row0 + r * 256 + tid;
        const double2 v = i < n ? Y[i] : double2{0.0, 0.0};
        xi[r] = v.x;
        yi[r] = v.y;
        sw[r] = fx[r] = fy[r] = 0.0;
    }
#pragma unroll 1
    for (int c0 = (int)j0; c0 < j1; c0 += TS_CHUNK) {
        const int cnt = j1 - c0 < TS_CHUNK ? j1 - c0 : TS_CHUNK;
        __syncthreads();   // the last chunk is consumed
        for (int e = tid; e < cnt; e += 256) s_y[e] = Y[c0 + e];
        __syncthreads();
        int self[TS_R];
#pragma unroll
        for (int r = 0; r < TS_R; ++r) self[r] = row0 + r * 256 + tid - c0;
        if (c0 < row0 + TS_TILE && c0 + cnt > row0) ts_pairs<true>(s_y, cnt, xi, yi, self, sw, fx, fy);   // block-uniform
        else ts_pairs<false>(s_y, cnt, xi, yi, self, sw, fx, fy);
    }
#pragma unroll
    for (int r = 0; r < TS_R; ++r) {
        const int i = row0 + r * 256 + tid;
        if (i < n) {
            double *o = part + ((size_t)blockIdx.y * n + i) * 3;
            o[0] = sw[r];
            o[1] = fx[r];
            o[2] = fy[r];
        }
    }
}

// One thread per row i < n: rep[i] = the slabs' partials added in slab order; zpart[block] = the block's 256 sums of w added
// in row order (rows >= n count 0).
__global__ void __launch_bounds__(256) k_ts_reduce(const double *__restrict__ part, int slabs, int n, double *__restrict__ rep,
                                                   double *__restrict__ zpart)
{
    __shared__ double s_w[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double a = 0.0, b = 0.0, c = 0.0;
    if (i < n) {
        for (int s = 0; s < slabs; ++s) {
            const double *p = part + ((size_t)s * n + i) * 3;
            a += p[0];
            b += p[1];
            c += p[2];
        }
        rep[(size_t)i * 3 + 0] = a;
        rep[(size_t)i * 3 + 1] = b;
        rep[(size_t)i * 3 + 2] = c;
    }
    s_w[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int e = 0; e < 256; ++e) sum += s_w[e];
        zpart[blockIdx.x] = sum;
    }
}

// One block: out[c] = the sum over e < cnt of part[e nc + c], c < nc <= 3; thread t adds e = t, t + 256, ... in that order,
// thread 0 the 256 results in thread order.
__global__ void __launch_bounds__(256) k_ts_fold(const double *__restrict__ part, int cnt, int nc, double *__restrict__ out)
{
    __shared__ double s_s[3][256];
    for (int c = 0; c < nc; ++c) {
        double sum = 0.0;
        for (int e = threadIdx.x; e < cnt; e += 256) sum += part[(size_t)e * nc + c];
        s_s[c][threadIdx.x] = sum;
    }
    __syncthreads();
    if ((int)threadIdx.x < nc) {
        double sum = 0.0;
        for (int e = 0; e < 256; ++e) sum += s_s[threadIdx.x][e];
        out[threadIdx.x] = sum;
    }
}

// grid = ceil(n / 16) blocks of 256 threads, 16 lanes per row.  zsum[0] = Z (k_ts_fold of zpart).  update != 0: the
// iteration's step with exaggeration a, momentum mu and step eta on (V, G), the new position going to Ynew (another buffer:
// other rows still read Y); update == 0: nothing moves and the gradient (under a) goes to grad.  record != 0: the row's KL term is formed.  spart[block] = (sum x, sum y, sum KL) of the block's rows
// in row order, x and y AFTER the update.  zout (may be NULL): Z, written by block 0.
__global__ void __launch_bounds__(256) k_ts_step(const int32_t *__restrict__ idx, const double *__restrict__ PF,
                                                 const int32_t *__restrict__ ro_ptr, const int32_t *__restrict__ ro_src,
                                                 const double *__restrict__ PR, const double *__restrict__ rep,
                                                 const double *__restrict__ zsum, int n, int k, double a, double mu, double eta,
                                                 int update, int record, const double2 *__restrict__ Y, double2 *__restrict__ Ynew,
                                                 double2 *__restrict__ V, double2 *__restrict__ G, double2 *__restrict__ grad,
                                                 double *__restrict__ spart, double *__restrict__ zout)
{
    __shared__ double s_p[TS_ROWS][3];
    const int row = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int i = blockIdx.x * TS_ROWS + row;
    const double Z = zsum[0];
    if (zout && blockIdx.x == 0 && threadIdx.x == 0) zout[0] = Z;
    double ax = 0.0, ay = 0.0, kl = 0.0;
    double2 yi = double2{0.0, 0.0};
    if (i < n) {
        yi = Y[i];
        const int32_t *ri = idx + (size_t)i * k;
        const double *rp = PF + (size_t)i * k;
        for (int s = l; s < k; s += 16) {
            const int j = ri[s];
            if (j < 0) break;   // filled slots come first
            const double P = rp[s];
            const double2 yj = Y[j];
            const double dx = yi.x - yj.x, dy = yi.y - yj.y;
            const double d = fma(dx, dx, fma(dy, dy, 1.0));
            const double t = P / d;
            ax = fma(t, dx, ax);
            ay = fma(t, dy, ay);
            if (record && P > 0.0) kl = fma(P, log(P * Z * d), kl);
        }
        for (int e = ro_ptr[i] + l; e < ro_ptr[i + 1]; e += 16) {
            const double P = PR[e];
            const double2 yj = Y[ro_src[e]];
            const double dx = yi.x - yj.x, dy = yi.y - yj.y;
            const double d = fma(dx, dx, fma(dy, dy, 1.0));
            const double t = P / d;
            ax = fma(t, dx, ax);
            ay = fma(t, dy, ay);
            if (record && P > 0.0) kl = fma(P, log(P * Z * d), kl);
        }
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        ax += __shfl_xor(ax, m);
        ay += __shfl_xor(ay, m);
        kl += __shfl_xor(kl, m);
    }
    double px = 0.0, py = 0.0;
    if (l == 0 && i < n) {
#pragma clang fp contract(off)
        const double gx = 4.0 * (a * ax - rep[(size_t)i * 3 + 1] / Z), gy = 4.0 * (a * ay - rep[(size_t)i * 3 + 2] / Z);
        if (update) {
            double2 v = V[i], g = G[i];
            g.x = (gx > 0.0) != (v.x > 0.0) ? g.x + 0.2 : g.x * 0.8;
            g.y = (gy > 0.0) != (v.y > 0.0) ? g.y + 0.2 : g.y * 0.8;
            g.x = g.x < 0.01 ? 0.01 : g.x;
            g.y = g.y < 0.01 ? 0.01 : g.y;
            v.x = mu * v.x - (eta * g.x) * gx;
            v.y = mu * v.y - (eta * g.y) * gy;
            yi.x = yi.x + v.x;
            yi.y = yi.y + v.y;
            G[i] = g;
            V[i] = v;
            Ynew[i] = yi;
        } else {
            grad[i] = double2{gx, gy};
        }
        px = yi.x;
        py = yi.y;
    }
    if (l == 0) {
        s_p[row][0] = px;
        s_p[row][1] = py;
        s_p[row][2] = i < n ? kl : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double sum = 0.0;
        for (int r = 0; r < TS_ROWS; ++r) sum += s_p[r][threadIdx.x];
        spart[(size_t)blockIdx.x * 3 + threadIdx.x] = sum;
    }
}

// One thread per row: y -= (sums[0], sums[1]) / n.  klout (may be NULL): sums[2], written by thread 0.
__global__ void __launch_bounds__(256) k_ts_centre(const double *__restrict__ sums, int n, double2 *__restrict__ Y,
                                                   double *__restrict__ klout)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (klout && i == 0) klout[0] = sums[2];
    if (i >= n) return;
    const double mx = sums[0] / (double)n, my = sums[1] / (double)n;
    double2 y = Y[i];
    y.x -= mx;
    y.y -= my;
    Y[i] = y;
}

}  // namespace insider
