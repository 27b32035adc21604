// insider_coexpr_pc.hpp — pairwise-complete top-k correlated partners among N deep vectors with missing entries
// (insider_hip_gram_topk_pairwise, insider_hip_coexpression_pairwise; host drivers in insider_hip.hip, section "co-expression").
//
// Definition.  A pair of vectors a, b of depth D has values v and selection indicators m in {0, 1}; J = the positions selected
// in both.  With z = m v (0 where unselected) and q = z z the six sums over the whole depth
//     N   = m_a'm_b = |J|         Sab = z_a'z_b
//     Sa  = z_a'm_b = sum_J a      Sb  = m_a'z_b = sum_J b
//     Saa = q_a'm_b = sum_J a a    Sbb = m_a'q_b = sum_J b b
// give cov = Sab - Sa Sb / N, va = Saa - Sa Sa / N, vb = Sbb - Sb Sb / N and score = cov / sqrt(va vb): Pearson's r over the
// jointly selected positions, not clipped.  The sums run over the STAGED values: every vector is first standardised over its
// own selected entries exactly as cx_standardise (insider_coexpr.hpp) does for the zero-filled score, which the score does not
// see (it is invariant under an affine map of either vector) and which keeps the cancellation in va and vb mild; a vector that
// is dead by that rule (fewer than two selected entries, no variance) is dead here.
// A pair is eligible when both vectors are alive, a != b, N >= min_overlap, va > floor Saa and vb > floor Sbb, with
// floor = 16 (D + 8) 2^-52: va computed this way errs by at most (3 D + 3) 2^-53 Saa to first order (D roundings in each of the
// two sums, the square, the quotient and the difference), so a vector that is exactly constant on J lands under the floor and
// one with Saa / va below about 10^12 lands above it.  N is a sum of 0 / 1 products and is exact.
//
// Operands: one staged buffer in the operand order of insider_coexpr.hpp, P[tile][d][c], in which an unselected entry is NaN.
// The three operands of a vector (z, q, m) are derived in registers after the ds_read: one compare / select, one multiply and
// one select per loaded double against 6 CXP_BT matrix instructions per query operand, so a NaN never reaches a matrix
// instruction and global and LDS traffic are those of one product, not of three.  A padded position (d >= depth, up to Dpad)
// and a padded vector (>= N, up to npad) are unselected, NaN, not a selected 0: k_cx_std_pc writes them.
//
// k_cx_std_pc: one thread per vector; copies the caller's column (NaN = missing) when there is one, standardises the selected
// entries with cx_standardise's sums (fill = NaN: unselected entries and dead vectors stay unselected) and writes the padding.
//
// k_cx_topk_pc is the product kernel of k_cx_topk: the same flat LDS copy with register prefetch, one conflict-free
// ds_read_b64 per operand, v_mfma_f64_16x16x4.  A block of CX_WAVES waves owns CX_QB queries and walks the base CXP_BG =
// 16 CXP_BT vectors at a time; per (query tile, base tile) six accumulator chains run over the depth in ascending order, and
// the epilogue, written symmetrically in a and b (products of the two sides commute, each side's own terms are formed alike),
// gives score(a, b) and score(b, a) the same bits.  The selection is that of insider_neighbors.hpp with the pair's N as the
// payload of nn_merge_t<true>.  No floating-point atomics.
//
// Registers: 438 VGPRs, no scratch (tools/kernel_regs.sh): 6 CXP_BT 4 doubles of accumulators = 96 at CXP_BT = 2, 24 of
// prefetch, and the compiler keeps a chunk's 24 loaded operands and the z, q, m derived from them in flight; CX_BT = 4 would
// need 192 for the accumulators alone.  One wave per SIMD, as k_cx_topk.  LDS: 8 (CX_QB + CXP_BG) CX_DC = 24 KB of operands, CX_WAVES 16 (k + NN_CAP) 16 bytes of lists and buffers (42 KB at
// k = 10, 96 KB at k = 64) and 4 CXP_BG bytes of flags: 120.1 KB at k = 64.
#pragma once

namespace insider {

constexpr int CXP_BT = 2;               // base tiles per step of k_cx_topk_pc: 6 CXP_BT accumulators per wave
constexpr int CXP_BG = 16 * CXP_BT;     // base vectors per step

static_assert(CX_PAD % CXP_BG == 0, "the padding of N serves the base groups of the pairwise form");

constexpr size_t cx_topk_pc_lds(int k)
{
    return (size_t)(CX_QB + CXP_BG) * CX_DC * sizeof(double) +
           (size_t)CX_WAVES * 16 * (k + NN_CAP) * (sizeof(double) + 2 * sizeof(int)) + (size_t)CXP_BG * sizeof(int);
}

// One thread per vector j < npad.  V: depth x n, column-major, NaN = missing, or nullptr: P already holds the vectors (NaN =
// unselected; k_cx_stage).  Writes every double of the vector's Dpad: the standardised selected entries, NaN elsewhere.
__global__ void __launch_bounds__(64) k_cx_std_pc(const double *__restrict__ V, int64_t depth, int64_t n, int64_t npad,
                                                  int64_t Dpad, double *__restrict__ P, int *__restrict__ alive)
{
    const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (j >= npad) return;
    double *o = P + (size_t)(j >> 4) * Dpad * 16 + (j & 15);
    const double nan = __builtin_nan("");
    int ok = 0;
    int64_t d0 = 0;
    if (j < n) {
        if (V) {
            const double *c = V + (size_t)j * depth;
            for (int64_t d = 0; d < depth; ++d) o[16 * d] = c[d];
        }
        ok = cx_standardise(o, depth, 0, nan);
        d0 = depth;
    }
    for (int64_t d = d0; d < Dpad; ++d) o[16 * d] = nan;
    alive[j] = ok;
}

// this thread's pair of doubles of the chunk ch of the CX_WAVES query tiles from tile tq and of the CXP_BT base tiles from tb
__device__ __forceinline__ void cxp_fetch(const double *__restrict__ P, int64_t Dpad, int64_t tq, int64_t tb, int64_t ch,
                                          d2 (&pre)[CX_WAVES + CXP_BT])
{
    const size_t off = (size_t)ch * CX_TC + 2 * threadIdx.x;
#pragma unroll
    for (int u = 0; u < CX_WAVES; ++u) pre[u] = *reinterpret_cast<const d2 *>(P + (size_t)(tq + u) * Dpad * 16 + off);
#pragma unroll
    for (int u = 0; u < CXP_BT; ++u) pre[CX_WAVES + u] = *reinterpret_cast<const d2 *>(P + (size_t)(tb + u) * Dpad * 16 + off);
}

// grid = the query groups of CX_QB that meet the window [first, first + count), blocks of 64 CX_WAVES threads, dynamic LDS
// cx_topk_pc_lds(k).  P / alive: k_cx_std_pc's output, npad vectors (a multiple of CX_PAD) of Dpad (a multiple of CX_DC).
// vfloor = 16 (depth + 8) 2^-52.  idx_out / score_out / overlap_out: count x k, query-major, row = query - first; open slots
// hold -1 / NaN / -1.
__global__ void __launch_bounds__(64 * CX_WAVES) k_cx_topk_pc(const double *__restrict__ P, const int *__restrict__ alive,
                                                              int64_t npad, int64_t Dpad, int64_t min_overlap, double vfloor,
                                                              int k, int64_t first, int64_t count,
                                                              int32_t *__restrict__ idx_out, double *__restrict__ score_out,
                                                              int32_t *__restrict__ overlap_out)
{
    extern __shared__ double s_cxp[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int per = 16 * (k + NN_CAP);
    double *s_q = s_cxp, *s_b = s_cxp + CX_QB * CX_DC;
    double *lst_s = s_b + CXP_BG * CX_DC + w * per, *buf_s = lst_s + 16 * k;
    int *s_alive = reinterpret_cast<int *>(s_b + CXP_BG * CX_DC + CX_WAVES * per);
    int *lst_i = s_alive + CXP_BG + w * per, *buf_i = lst_i + 16 * k;
    int *lst_p = s_alive + CXP_BG + (CX_WAVES + w) * per, *buf_p = lst_p + 16 * k;

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
    d2 pre[CX_WAVES + CXP_BT];
    cxp_fetch(P, Dpad, qg >> 4, 0, 0, pre);
#pragma unroll 1
    for (int64_t j0 = 0; j0 < npad; j0 += CXP_BG) {
        // per base tile: z_a'z_b, z_a'm_b, m_a'z_b, q_a'm_b, m_a'q_b, m_a'm_b
        d4 zz[CXP_BT], zm[CXP_BT], mz[CXP_BT], qm[CXP_BT], mq[CXP_BT], mm[CXP_BT];
#pragma unroll
        for (int u = 0; u < CXP_BT; ++u) zz[u] = zm[u] = mz[u] = qm[u] = mq[u] = mm[u] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int64_t ch = 0; ch < nch; ++ch) {
            __syncthreads();   // the last chunk is consumed, the last group selected
#pragma unroll
            for (int u = 0; u < CX_WAVES; ++u) *reinterpret_cast<d2 *>(s_q + u * CX_TC + 2 * threadIdx.x) = pre[u];
#pragma unroll
            for (int u = 0; u < CXP_BT; ++u) *reinterpret_cast<d2 *>(s_b + u * CX_TC + 2 * threadIdx.x) = pre[CX_WAVES + u];
            if (ch == 0 && threadIdx.x < CXP_BG) s_alive[threadIdx.x] = alive[j0 + threadIdx.x];
            __syncthreads();
            // the next chunk (of this pair of groups, or the first of the next) is in flight during the products
            const bool last = ch + 1 == nch;
            const int64_t jn = last ? j0 + CXP_BG : j0;
            if (jn < npad) cxp_fetch(P, Dpad, qg >> 4, jn >> 4, last ? 0 : ch + 1, pre);
            const double *ql = s_q + w * CX_TC + lane, *bl = s_b + lane;
#pragma unroll
            for (int s = 0; s < CX_DC / 4; ++s) {
                const double a = ql[64 * s];
                const bool sa = a == a;   // (NaN: unselected)
                const double za = sa ? a : 0.0, ma = sa ? 1.0 : 0.0, qa = __dmul_rn(za, za);
#pragma unroll
                for (int u = 0; u < CXP_BT; ++u) {
                    const double b = bl[u * CX_TC + 64 * s];
                    const bool sb = b == b;
                    const double zb = sb ? b : 0.0, mb = sb ? 1.0 : 0.0, qb = __dmul_rn(zb, zb);
                    zz[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(za, zb, zz[u], 0, 0, 0);
                    zm[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(za, mb, zm[u], 0, 0, 0);
                    mz[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, zb, mz[u], 0, 0, 0);
                    qm[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(qa, mb, qm[u], 0, 0, 0);
                    mq[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, qb, mq[u], 0, 0, 0);
                    mm[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, mb, mm[u], 0, 0, 0);
                }
            }
        }
        // the finished sums of the CXP_BT tiles, in ascending base order: lane (g, t), register r = (query g + 4 r, column t).
        // One copy of the epilogue and the selection: the tile's accumulators are picked by compares, not by a register index.
#pragma unroll 1
        for (int u = 0; u < CXP_BT; ++u) {
            d4 Sab = zz[0], Sa = zm[0], Sb = mz[0], Saa = qm[0], Sbb = mq[0], Nn = mm[0];
#pragma unroll
            for (int v = 1; v < CXP_BT; ++v)
                if (u == v) { Sab = zz[v]; Sa = zm[v]; Sb = mz[v]; Saa = qm[v]; Sbb = mq[v]; Nn = mm[v]; }
            const int64_t j = j0 + u * 16 + t;
            const bool eb = s_alive[u * 16 + t] != 0;
            bool spill = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // symmetric in a and b: every product of the two sides commutes, each side's own terms are formed alike
                const double nn = Nn[r];
                const double cov = __dsub_rn(Sab[r], __ddiv_rn(__dmul_rn(Sa[r], Sb[r]), nn));
                const double va = __dsub_rn(Saa[r], __ddiv_rn(__dmul_rn(Sa[r], Sa[r]), nn));
                const double vb = __dsub_rn(Sbb[r], __ddiv_rn(__dmul_rn(Sb[r], Sb[r]), nn));
                const double sc = __ddiv_rn(cov, __dsqrt_rn(__dmul_rn(va, vb)));
                const bool el = eb && qok[r] && j != selfj[r] && (int64_t)nn >= min_overlap && va > __dmul_rn(vfloor, Saa[r]) &&
                                vb > __dmul_rn(vfloor, Sbb[r]);
                const bool ok = el && (nl[r] < k || sc > thr[r]);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
                if (m == 0) continue;   // wave-uniform
                const unsigned grp = (unsigned)(m >> (16 * g)) & 0xffffu;
                if (ok) {
                    const int pos = cnt[r] + __popc(grp & ((1u << t) - 1u));   // < NN_CAP: cnt <= NN_CAP - 16 before the tile
                    buf_s[(g + 4 * r) * NN_CAP + pos] = sc;
                    buf_i[(g + 4 * r) * NN_CAP + pos] = (int)j;
                    buf_p[(g + 4 * r) * NN_CAP + pos] = (int)nn;
                }
                cnt[r] += __popc(grp);
                spill = spill || cnt[r] > NN_CAP - 16;
            }
            if (__builtin_amdgcn_ballot_w64(spill)) nn_merge_t<true>(lst_s, lst_i, lst_p, buf_s, buf_i, buf_p, k, lane, cnt, nl, thr);
        }
    }
    nn_merge_t<true>(lst_s, lst_i, lst_p, buf_s, buf_i, buf_p, k, lane, cnt, nl, thr);
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
                overlap_out[o] = lane < n ? lst_p[q * k + lane] : -1;
            }
        }
    }
}

}  // namespace insider
