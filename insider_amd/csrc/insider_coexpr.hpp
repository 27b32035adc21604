// insider_coexpr.hpp — top-k correlated partners among N deep vectors (insider_hip_gram_topk) and among the genes or the
// samples of a fitted model's residual (insider_hip_coexpression; host drivers in insider_hip.hip, section "co-expression").
//
// N vectors of `depth` doubles are standardised (correlation: centred by their own mean and divided by the root of the centred
// sum of squares; cosine: divided by the root of the sum of squares; dot: left alone), so that the score of a pair is the plain
// dot product of the two standardised vectors, and every vector gets its k best partners among all the others, in descending
// score, equal scores by ascending index (-0.0 == 0.0): the order, the open slots (-1 / NaN) and the selection of
// insider_neighbors.hpp.  The N x N scores never exist.
//
// Operand order.  P[tile][d][c]: tiles of 16 vectors (c = vector & 15), d < Dpad = depth rounded up to CX_DC, zero beyond the
// depth, and N rounded up to whole groups of CX_QB / CX_BG vectors (zero and dead beyond N).  The CX_DC deep chunk of a tile is
// 16 CX_DC contiguous doubles, and MFMA step s of a chunk reads its 64 doubles 64 s .. 64 s + 63 (lane = 16 (d & 3) + c: the
// operand map of insider_mm.hpp), for the A operand (queries) and the B operand (base) alike.
//
// k_cx_prep copies the caller's vectors (column-major, depth x N) into operand order and standardises them; k_cx_stage writes
// the raw working residual of insider_rescomp.hpp, r = (x - f - centre) / scale, in operand order for the requested axis in one
// streaming pass over X and the mask codes (the fit of a 16 x 16 tile on the f64 matrix instruction from the total embedding,
// the layout of k_rc_fwd), an unselected entry as NaN; k_cx_norm then standardises the staged vectors in place (selected
// entries are centred by the mean over the selected entries, unselected ones become 0).  A thread owns a vector and every sum
// runs in index order with separately rounded products and sums: what a vector becomes depends on that vector alone.  A vector
// with fewer than two selected entries or a (centred) sum of squares that is not > 0 is dead: all zero, nobody's partner, its
// own row all open slots.
//
// k_cx_topk.  A block of CX_WAVES waves owns CX_QB = 16 CX_WAVES queries, one tile per wave, and walks the base in ascending
// index, CX_BG = 16 CX_BT vectors at a time.  For a (query group, base group) pair the depth runs in chunks of CX_DC: the
// chunk of both groups is copied flat into LDS (it is already in operand order: one conflict-free ds_read_b64 per MFMA operand)
// while the next chunk's global loads are in flight in registers, and every wave runs 1 x CX_BT accumulators of
// v_mfma_f64_16x16x4 (C/D map: column = lane & 15, row = (lane >> 4) + 4 register).  The score of a pair is one accumulator
// chain over the depth in ascending order, chunks and steps included, wherever the pair falls in tiles, windows or the grid;
// the padded depth adds exact zeros.  When the depth loop of a pair of groups ends the CX_BT finished tiles go, in ascending
// base order, through the selection of insider_neighbors.hpp (threshold compare, append at ballot positions, nn_merge).
//
// LDS: 8 (CX_QB + CX_BG) CX_DC = 32 KB of operands, CX_WAVES 16 (k + NN_CAP) 12 bytes of lists and buffers (32 KB at k = 10,
// 72 KB at k = 64) and 4 CX_BG bytes of flags.  Above 64 KB the launch sets the function attribute.  Registers: 292 VGPRs, no
// scratch (the compiler keeps a chunk's 40 LDS operands in flight beside 32 accumulator and 32 prefetch registers; held to
// 256 it spills 36), so a CU runs one block, one wave per SIMD: the wave's 32 products per chunk keep its matrix pipe busy
// and the register prefetch hides the global latency.  No floating-point atomics anywhere.
#pragma once

namespace insider {

constexpr int CX_WAVES = 4;              // waves per block of k_cx_topk: one query tile each
constexpr int CX_QB = 16 * CX_WAVES;     // queries per block
constexpr int CX_BT = 4;                 // base tiles per step: the accumulators of a wave
constexpr int CX_BG = 16 * CX_BT;        // base vectors per step
constexpr int CX_DC = 32;                // depth chunk staged in LDS (8 product steps)
constexpr int CX_TC = 16 * CX_DC;        // doubles of one tile's chunk
constexpr int CX_PAD = CX_QB > CX_BG ? CX_QB : CX_BG;   // N is padded to whole groups (CX_QB and CX_BG divide it)

static_assert(CX_TC == 2 * 64 * CX_WAVES, "a thread copies one pair of doubles per tile chunk");
static_assert(CX_PAD % CX_QB == 0 && CX_PAD % CX_BG == 0, "one padding serves the query and the base groups");

constexpr size_t cx_topk_lds(int k)
{
    return (size_t)(CX_QB + CX_BG) * CX_DC * sizeof(double) + (size_t)CX_WAVES * 16 * (k + NN_CAP) * (sizeof(double) + sizeof(int)) +
           (size_t)CX_BG * sizeof(int);
}

// Standardise the vector o[16 d], d < depth, in place (metric 0: correlation, 1: cosine; a NaN is an unselected entry and
// becomes `fill`, as does every entry of a dead vector).  Returns whether the vector is alive.
__device__ __forceinline__ int cx_standardise(double *o, int64_t depth, int metric, double fill = 0.0)
{
    double sum = 0.0, mean = 0.0;
    int64_t m = 0;
    for (int64_t d = 0; d < depth; ++d) {
        const double v = o[16 * d];
        if (v == v) {
            sum = __dadd_rn(sum, v);
            ++m;
        }
    }
    if (metric == 0) mean = sum / (double)m;
    double ss = 0.0;
    for (int64_t d = 0; d < depth; ++d) {
        const double v = o[16 * d];
        if (v == v) {
            const double c = v - mean;
            ss = __dadd_rn(ss, __dmul_rn(c, c));
        }
    }
    const bool ok = (metric != 0 || m >= 2) && ss > 0.0;   // (NaN fails the comparison)
    const double nrm = sqrt(ss);
    for (int64_t d = 0; d < depth; ++d) {
        const double v = o[16 * d];
        o[16 * d] = ok && v == v ? (v - mean) / nrm : fill;
    }
    return ok ? 1 : 0;
}

// One thread per vector j < npad.  V: depth x n, column-major; P: zero on entry; metric 0 / 1 / 2 = correlation / cosine / dot.
__global__ void __launch_bounds__(64) k_cx_prep(const double *__restrict__ V, int64_t depth, int64_t n, int64_t npad,
                                                int64_t Dpad, int metric, double *__restrict__ P, int *__restrict__ alive)
{
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= npad) return;
    int ok = 0;
    if (j < n) {
        double *o = P + (size_t)(j >> 4) * Dpad * 16 + (j & 15);
        const double *c = V + (size_t)j * depth;
        for (int64_t d = 0; d < depth; ++d) o[16 * d] = c[d];
        ok = metric == 2 ? 1 : cx_standardise(o, depth, metric);
    }
    alive[j] = ok;
}

// One thread per staged vector j < npad: the correlation standardisation over the selected entries, in place.
__global__ void __launch_bounds__(64) k_cx_norm(double *__restrict__ P, int64_t depth, int64_t n, int64_t npad, int64_t Dpad,
                                                int *__restrict__ alive)
{
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= npad) return;
    alive[j] = j < n ? cx_standardise(P + (size_t)(j >> 4) * Dpad * 16 + (j & 15), depth, 0) : 0;
}

// grid = (ceil(n / RC_TILE), slabs) blocks of 64 RC_WAVES threads; dynamic LDS 4 KS 64 doubles.  The arguments and the fit
// are those of k_rc_fwd (insider_rescomp.hpp): lane (g, t) holds sample t of its wave of the genes g0 + 4 s + g.  axis 0: the
// vectors are the genes (P[gene >> 4][sample][gene & 15]); axis 1: the samples (P[sample >> 4][gene][sample & 15]).  Entries
// inside the matrix are written, an unselected one as NaN; P is zero on entry.
template <int KS>
__global__ void __launch_bounds__(64 * RC_WAVES) k_cx_stage(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const double *__restrict__ U, const double *__restrict__ cp, int K, const double *__restrict__ cs, int sel_mask,
    int64_t slab_len, int axis, int64_t Dpad, double *__restrict__ P)
{
    constexpr int KPW = 16 * KS;
    extern __shared__ double s_cxs[];
    double *s_c = s_cxs;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int i0 = (blockIdx.x * RC_WAVES + w) * 16;   // this wave's first sample
    const bool s_in = i0 + t < n;
    const int ic = s_in ? i0 + t : n - 1;              // (a sample beyond n reads the last one: never written)
    const int64_t jb = (int64_t)blockIdx.y * slab_len;
    const int64_t je = jb + slab_len < p ? jb + slab_len : p;
    const int ks4 = (K + 3) >> 2;
    double bu[4 * KS];   // B operand of the fit: U[sample t][4 s + g]
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s) bu[s] = U[(size_t)ic * KPW + 4 * s + g];
#pragma unroll 1
    for (int64_t g0 = jb; g0 < je; g0 += 16) {
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
            const int64_t j = g0 + 4 * s + g;
            if (!s_in || j >= je) continue;
            const bool sel = sel_mask == 0 || ((int)cd[s] & sel_mask);
            const double v = sel ? (x[s] - f[s] - cen[s]) * inv[s] : __builtin_nan("");
            const int64_t i = i0 + t;
            const size_t o = axis == 0 ? ((size_t)(j >> 4) * Dpad + i) * 16 + (j & 15) : ((size_t)(i >> 4) * Dpad + j) * 16 + (i & 15);
            P[o] = v;
        }
        __syncthreads();   // the next group overwrites the operand
    }
}

// this thread's pair of doubles of the chunk ch of the CX_WAVES query tiles from tile tq and of the CX_BT base tiles from tb
__device__ __forceinline__ void cx_fetch(const double *__restrict__ P, int64_t Dpad, int64_t tq, int64_t tb, int64_t ch,
                                         d2 (&pre)[CX_WAVES + CX_BT])
{
    const size_t off = (size_t)ch * CX_TC + 2 * threadIdx.x;
#pragma unroll
    for (int u = 0; u < CX_WAVES; ++u) pre[u] = *reinterpret_cast<const d2 *>(P + (size_t)(tq + u) * Dpad * 16 + off);
#pragma unroll
    for (int u = 0; u < CX_BT; ++u) pre[CX_WAVES + u] = *reinterpret_cast<const d2 *>(P + (size_t)(tb + u) * Dpad * 16 + off);
}

// grid = the query groups of CX_QB that meet the window [first, first + count), blocks of 64 CX_WAVES threads, dynamic LDS
// cx_topk_lds(k).  P / alive: npad vectors (a multiple of CX_PAD) of Dpad (a multiple of CX_DC) in operand order.  A query is
// never its own partner.  idx_out / score_out: count x k, query-major, row = query - first; open slots hold -1 / NaN.
__global__ void __launch_bounds__(64 * CX_WAVES) k_cx_topk(const double *__restrict__ P, const int *__restrict__ alive,
                                                           int64_t npad, int64_t Dpad, int k, int64_t first, int64_t count,
                                                           int32_t *__restrict__ idx_out, double *__restrict__ score_out)
{
    extern __shared__ double s_cx[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int per = 16 * (k + NN_CAP);
    double *s_q = s_cx, *s_b = s_cx + CX_QB * CX_DC;
    double *lst_s = s_b + CX_BG * CX_DC + w * per, *buf_s = lst_s + 16 * k;
    int *s_alive = reinterpret_cast<int *>(s_b + CX_BG * CX_DC + CX_WAVES * per);
    int *lst_i = s_alive + CX_BG + w * per, *buf_i = lst_i + 16 * k;

    const int64_t qg = (first / CX_QB + blockIdx.x) * CX_QB;   // this block's first query (qg + CX_QB <= npad)
    const int64_t q0 = qg + 16 * w;                              // this wave's
    bool qok[4];
    int64_t selfj[4];
    int cnt[4], nl[4];
    double thr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t qi = q0 + g + 4 * r;
        qok[r] = qi >= first && qi < first + count && alive[qi] != 0;
        selfj[r] = qi;
        cnt[r] = nl[r] = 0;
        thr[r] = 0.0;
    }
    const int64_t nch = Dpad / CX_DC;
    d2 pre[CX_WAVES + CX_BT];
    cx_fetch(P, Dpad, qg >> 4, 0, 0, pre);
#pragma unroll 1
    for (int64_t j0 = 0; j0 < npad; j0 += CX_BG) {
        d4 acc[CX_BT];
#pragma unroll
        for (int u = 0; u < CX_BT; ++u) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int64_t ch = 0; ch < nch; ++ch) {
            __syncthreads();   // the last chunk is consumed, the last group selected
#pragma unroll
            for (int u = 0; u < CX_WAVES; ++u) *reinterpret_cast<d2 *>(s_q + u * CX_TC + 2 * threadIdx.x) = pre[u];
#pragma unroll
            for (int u = 0; u < CX_BT; ++u) *reinterpret_cast<d2 *>(s_b + u * CX_TC + 2 * threadIdx.x) = pre[CX_WAVES + u];
            if (ch == 0 && threadIdx.x < CX_BG) s_alive[threadIdx.x] = alive[j0 + threadIdx.x];
            __syncthreads();
            // the next chunk (of this pair of groups, or the first of the next) is in flight during the products
            const bool last = ch + 1 == nch;
            const int64_t jn = last ? j0 + CX_BG : j0;
            if (jn < npad) cx_fetch(P, Dpad, qg >> 4, jn >> 4, last ? 0 : ch + 1, pre);
            const double *ql = s_q + w * CX_TC + lane, *bl = s_b + lane;
#pragma unroll
            for (int s = 0; s < CX_DC / 4; ++s) {
                const double a = ql[64 * s];
#pragma unroll
                for (int u = 0; u < CX_BT; ++u)
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bl[u * CX_TC + 64 * s], acc[u], 0, 0, 0);
            }
        }
        // the finished scores of the CX_BT tiles, in ascending base order: lane (g, t), register r = (query g + 4 r, column t).
        // One copy of the selection code: the tile's accumulator is picked by compares, not by a register index.
#pragma unroll 1
        for (int u = 0; u < CX_BT; ++u) {
            d4 sc = acc[0];
#pragma unroll
            for (int v = 1; v < CX_BT; ++v)
                if (u == v) sc = acc[v];
            const int64_t j = j0 + u * 16 + t;
            const bool eb = s_alive[u * 16 + t] != 0;
            bool spill = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = eb && qok[r] && j != selfj[r] && (nl[r] < k || sc[r] > thr[r]);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
                if (m == 0) continue;   // wave-uniform
                const unsigned grp = (unsigned)(m >> (16 * g)) & 0xffffu;
                if (ok) {
                    const int pos = cnt[r] + __popc(grp & ((1u << t) - 1u));   // < NN_CAP: cnt <= NN_CAP - 16 before the tile
                    buf_s[(g + 4 * r) * NN_CAP + pos] = sc[r];
                    buf_i[(g + 4 * r) * NN_CAP + pos] = (int)j;
                }
                cnt[r] += __popc(grp);
                spill = spill || cnt[r] > NN_CAP - 16;
            }
            if (__builtin_amdgcn_ballot_w64(spill)) nn_merge(lst_s, lst_i, buf_s, buf_i, k, lane, cnt, nl, thr);
        }
    }
    nn_merge(lst_s, lst_i, buf_s, buf_i, k, lane, cnt, nl, thr);
    wave_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int n = __builtin_amdgcn_readlane(nl[r], 16 * gq);
            const int q = gq + 4 * r;
            const int64_t qi = q0 + q;
            if (qi >= first && qi < first + count && lane < k) {
                const size_t o = (size_t)(qi - first) * k + lane;
                idx_out[o] = lane < n ? lst_i[q * k + lane] : -1;
                score_out[o] = lane < n ? lst_s[q * k + lane] : __builtin_nan("");
            }
        }
    }
}

}  // namespace insider
