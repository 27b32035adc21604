// insider_neighbors.hpp — top-k nearest neighbours of embeddings (insider_hip_neighbors; host driver in insider_hip.hip,
// section "neighbours").
//
// Queries Q (K x nq) and base B (K x nb), one embedding = K contiguous doubles.  For every query the k base columns with the
// largest score, score = q.b (dot) or q.b / (|q| |b|) (cosine), listed in descending order, equal scores by ascending base
// index (a strict total order, -0.0 == 0.0): the answer is a pure function of the inputs.  The nq x nb scores never exist.
//
// k_nn_prep rewrites a matrix once, column by column, into MFMA operand order: tiles of 16 columns, tile t0 holding
// P[t0][k][c] (k < K4 = K rounded up to 4, zero beyond K; c = column & 15), so that the operand of MFMA step s of a tile is
// the 64 consecutive doubles P[t0][4 s ..][..] (lane = 16 (k & 3) + c, the map of insider_mm.hpp).  Under cosine a column is
// divided by its own norm here (sum of squares in index order, one sqrt), so the product is the score itself, and a column of
// norm 0 is marked dead; under dot the copy is plain.  Whatever a column becomes depends on that column alone.
//
// k_nn_topk: a wave owns 16 queries (A operand, up to 4 KS doubles per lane kept for the whole kernel), a block of NW waves
// streams the base NT tiles at a time through LDS (a flat copy: the staged tile is already in operand order, one conflict-free
// ds_read_b64 per MFMA, shared by the NW waves).  One chain of K4 / 4 v_mfma_f64_16x16x4 gives the 16 x 16 scores:
// lane (g = lane >> 4, t = lane & 15), register r holds (query g + 4 r, base column t of the tile).  The chain of a pair is the
// same instruction sequence wherever the pair falls, so scores do not depend on tiles, windows or launch geometry.
//
// Selection.  The 16 lanes of group g hold, per register r, everything about query g + 4 r: the length of its sorted list
// (<= k), the list's k-th score once it is full (the threshold) and the fill of its candidate buffer.  The base runs in
// ascending index order, so a candidate enters the top k only if the list is not full or its score is GREATER than the
// threshold (an equal score has a higher index than every entry of the list): one compare.  Survivors are appended to the
// query's buffer of NN_CAP slots in LDS at ballot / popcount positions (no atomics).  When a buffer could overflow on the next
// tile (fill > NN_CAP - 16), and once at the end, the wave merges: per query with a non-empty buffer, every element of list +
// buffer (<= k + NN_CAP <= 96, two per lane) counts the elements that come before it in the total order and moves to that
// rank if it is < k.  A stale threshold only lets more candidates through; the merged list is the exact top k of what was seen.
//
// LDS: 8 NT 16 K4 bytes of base + NW 16 (k + NN_CAP) 12 bytes of lists and buffers (+ 64 NT bytes of flags): the host picks
// NT = 4 (K4 <= 32) or 2 and NW = 4, or 2 when that would pass 64 KB (k > 32 or so).  The result does not depend on either.
#pragma once

namespace insider {

constexpr int NN_CAP = 32;        // candidate slots per query between two merges (>= 32: a tile adds up to 16)
constexpr int NN_MAX_TOPK = 64;   // k <= 64: list + buffer <= 128 elements, two per lane in the merge

// One thread per column j < npad (npad: a multiple of the tile sizes the reader needs, columns >= n are zero and dead).
__global__ void __launch_bounds__(256) k_nn_prep(const double *__restrict__ src /*K x n, column-major*/, int64_t n, int64_t npad,
                                                 int K, int K4, int metric, double *__restrict__ P, int *__restrict__ alive)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= npad) return;
    double *o = P + (size_t)(j >> 4) * 16 * K4 + (j & 15);
    const double *c = src + (size_t)j * K;
    int ok = j < n;
    double nrm = 1.0;
    if (ok && metric == 0) {
        double ss = 0.0;
        for (int k = 0; k < K; ++k) ss = fma(c[k], c[k], ss);
        nrm = sqrt(ss);
        ok = nrm > 0.0;
    }
    for (int k = 0; k < K4; ++k) o[16 * k] = ok && k < K ? (metric == 0 ? c[k] / nrm : c[k]) : 0.0;
    alive[j] = ok;
}

// a comes before b in the order of the result
__device__ __forceinline__ bool nn_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// Merge the candidate buffers of the wave's 16 queries into their sorted lists.  cnt / nl / thr: the per-lane copies (group g,
// register r: query g + 4 r) of buffer fill, list length and threshold.  PAY: every element carries an int of its own
// (lst_p / buf_p, laid out as lst_i / buf_i) that moves with it and takes no part in the order.
template <bool PAY>
__device__ __forceinline__ void nn_merge_t(double *lst_s, int *lst_i, int *lst_p, double *buf_s, int *buf_i, int *buf_p, int k,
                                           int lane, int (&cnt)[4], int (&nl)[4], double (&thr)[4])
{
    const int g = lane >> 4;
    wave_sync();   // the appended candidates are visible to the whole wave
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int c = __builtin_amdgcn_readlane(cnt[r], 16 * gq);
            if (c == 0) continue;   // wave-uniform
            const int n = __builtin_amdgcn_readlane(nl[r], 16 * gq);
            const int q = gq + 4 * r, tot = n + c;
            double *ls = lst_s + q * k, *bs = buf_s + q * NN_CAP;
            int *li = lst_i + q * k, *bi = buf_i + q * NN_CAP;
            int *lp = PAY ? lst_p + q * k : nullptr, *bp = PAY ? buf_p + q * NN_CAP : nullptr;
            const int e0 = lane, e1 = lane + 64;
            const bool v0 = e0 < tot, v1 = e1 < tot;
            double s0 = 0.0, s1 = 0.0;
            int i0 = 0, i1 = 0, p0 = 0, p1 = 0;
            if (v0) { s0 = e0 < n ? ls[e0] : bs[e0 - n]; i0 = e0 < n ? li[e0] : bi[e0 - n]; }
            if (v1) { s1 = e1 < n ? ls[e1] : bs[e1 - n]; i1 = e1 < n ? li[e1] : bi[e1 - n]; }
            if constexpr (PAY) {
                if (v0) p0 = e0 < n ? lp[e0] : bp[e0 - n];
                if (v1) p1 = e1 < n ? lp[e1] : bp[e1 - n];
            }
            int r0 = 0, r1 = 0;
            for (int e = 0; e < n; ++e) {
                const double se = ls[e];
                const int ie = li[e];
                r0 += nn_before(se, ie, s0, i0) ? 1 : 0;
                r1 += nn_before(se, ie, s1, i1) ? 1 : 0;
            }
            for (int e = 0; e < c; ++e) {
                const double se = bs[e];
                const int ie = bi[e];
                r0 += nn_before(se, ie, s0, i0) ? 1 : 0;
                r1 += nn_before(se, ie, s1, i1) ? 1 : 0;
            }
            wave_sync();   // every lane has read before any lane writes
            if (v0 && r0 < k) { ls[r0] = s0; li[r0] = i0; }
            if (v1 && r1 < k) { ls[r1] = s1; li[r1] = i1; }
            if constexpr (PAY) {
                if (v0 && r0 < k) lp[r0] = p0;
                if (v1 && r1 < k) lp[r1] = p1;
            }
            wave_sync();
            const int nn = tot < k ? tot : k;
            const double th = ls[k - 1];   // (read by all, used when the list is full)
            if (g == gq) {
                cnt[r] = 0;
                nl[r] = nn;
                thr[r] = th;
            }
        }
    }
}

// the merge without a payload
__device__ __forceinline__ void nn_merge(double *lst_s, int *lst_i, double *buf_s, int *buf_i, int k, int lane, int (&cnt)[4],
                                         int (&nl)[4], double (&thr)[4])
{
    nn_merge_t<false>(lst_s, lst_i, nullptr, buf_s, buf_i, nullptr, k, lane, cnt, nl, thr);
}

// grid = ceil(nq / (16 NW)) blocks of 64 NW threads.  Qp / Bp: k_nn_prep's output for the queries (padded to 16) and the base
// (nbpad columns, a multiple of 16 NT).  self_offset >= 0: query i never takes base column self_offset + i.  idx_out /
// score_out: nq x k, query-major; open slots hold -1 / NaN.  KS = ceil(K4 / 16).
// Dynamic LDS (doubles first): NT 16 K4 doubles, NW 16 (k + NN_CAP) doubles, NT 16 ints, NW 16 (k + NN_CAP) ints.
template <int KS>
__global__ void __launch_bounds__(256) k_nn_topk(const double *__restrict__ Qp, const int *__restrict__ qalive, int64_t nq,
                                                 const double *__restrict__ Bp, const int *__restrict__ balive, int64_t nbpad,
                                                 int K4, int NT, int k, int64_t self_offset, int32_t *__restrict__ idx_out,
                                                 double *__restrict__ score_out)
{
    extern __shared__ double s_nn[];
    const int NW = blockDim.x >> 6;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    const int per = 16 * (k + NN_CAP);
    double *s_b = s_nn;
    double *lst_s = s_nn + NT * 16 * K4 + w * per, *buf_s = lst_s + 16 * k;
    int *s_alive = reinterpret_cast<int *>(s_nn + NT * 16 * K4 + NW * per);
    int *lst_i = s_alive + NT * 16 + w * per, *buf_i = lst_i + 16 * k;

    const int64_t q0 = ((int64_t)blockIdx.x * NW + w) * 16;   // this wave's first query
    const bool active = q0 < nq;                               // wave-uniform
    double a[4 * KS];
    bool qok[4];
    int64_t selfj[4];
    int cnt[4], nl[4];
    double thr[4];
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s) a[s] = active && 4 * s < K4 ? Qp[(size_t)q0 * K4 + 64 * s + lane] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t qi = q0 + g + 4 * r;
        qok[r] = qi < nq && qalive[qi] != 0;
        selfj[r] = self_offset >= 0 ? self_offset + qi : -1;
        cnt[r] = nl[r] = 0;
        thr[r] = 0.0;
    }
    const int nstage = NT * 16 * K4;
#pragma unroll 1
    for (int64_t j0 = 0; j0 < nbpad; j0 += 16 * NT) {
        __syncthreads();   // the tiles of the last step are consumed
        const double *src = Bp + (size_t)j0 * K4;
        for (int e = threadIdx.x; e < nstage; e += blockDim.x) s_b[e] = src[e];
        if (threadIdx.x < 16 * NT) s_alive[threadIdx.x] = balive[j0 + threadIdx.x];
        __syncthreads();
        if (!active) continue;
#pragma unroll 1
        for (int tile = 0; tile < NT; ++tile) {
            const double *bl = s_b + tile * 16 * K4 + lane;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4 * KS; ++s)
                if (4 * s < K4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bl[64 * s], acc, 0, 0, 0);
            const int64_t j = j0 + tile * 16 + t;
            const bool eb = s_alive[tile * 16 + t] != 0;
            bool spill = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = eb && qok[r] && j != selfj[r] && (nl[r] < k || acc[r] > thr[r]);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
                if (m == 0) continue;   // wave-uniform
                const unsigned grp = (unsigned)(m >> (16 * g)) & 0xffffu;
                if (ok) {
                    const int pos = cnt[r] + __popc(grp & ((1u << t) - 1u));   // < NN_CAP: cnt <= NN_CAP - 16 before the tile
                    buf_s[(g + 4 * r) * NN_CAP + pos] = acc[r];
                    buf_i[(g + 4 * r) * NN_CAP + pos] = (int)j;
                }
                cnt[r] += __popc(grp);
                spill = spill || cnt[r] > NN_CAP - 16;
            }
            if (__builtin_amdgcn_ballot_w64(spill)) nn_merge(lst_s, lst_i, buf_s, buf_i, k, lane, cnt, nl, thr);
        }
    }
    if (!active) return;
    nn_merge(lst_s, lst_i, buf_s, buf_i, k, lane, cnt, nl, thr);
    wave_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int n = __builtin_amdgcn_readlane(nl[r], 16 * gq);
            const int q = gq + 4 * r;
            if (q0 + q < nq && lane < k) {
                const size_t o = (size_t)(q0 + q) * k + lane;
                idx_out[o] = lane < n ? lst_i[q * k + lane] : -1;
                score_out[o] = lane < n ? lst_s[q * k + lane] : __builtin_nan("");
            }
        }
    }
}

}  // namespace insider
