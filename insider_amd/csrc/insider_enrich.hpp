// insider_enrich.hpp — preranked gene-set enrichment with a permutation null (insider_hip_enrichment; host driver in
// insider_hip.hip, section "enrichment").  The contract (ranking, weights, the score of a position set, the null draws, the
// counts) is stated in include/insider_hip.h; the draws come from include/insider_sample.h.
//
// The host ranks each profile once (a stable sort) and uploads, per profile, rank_of_gene (int32, p) and the absolute score
// by rank position (double, p).  Everything behind that runs here, and both kernels score a position set with the SAME
// device function, so an observed set and a null draw that hold the same positions get the same bits:
//   gs_sort   a wave sorts its positions ascending in LDS (bitonic, padded to a power of two M2 >= 64 with INT_MAX);
//   gs_score  64 positions at a time: a wave prefix sum of the weights (shuffles, carried from chunk to chunk), then per
//             element the two deviations P_i / N - miss_i / (p - m) and P_{i-1} / N - miss_i / (p - m), each two fp64
//             divisions and one subtraction as the contract writes them, and a wave reduction to the extremes with the
//             smallest index among equals.  The weighted form runs the prefix sum twice, first for N alone, so no P_i is
//             kept: N is the carry behind the last element, hence P_m / N = 1 exactly.  N = 0 switches the set to w = 1.
// k_gs_observed: one wave (a block of 64) per (profile, set): gather the positions through rank_of_gene, sort, score; writes
//   es, peak and hits_nonzero.
// k_gs_null: one block of NW waves per (profile, distinct set size m).  Every wave generates a draw of its own (element j of
//   draw b is phi(j), one per lane), sorts and scores it; the scores of up to GS_CHUNK draws sit in LDS, then one thread per
//   set of that size walks them in draw order and adds to n_same / n_ge / sum_same (a compensated sum) of its (profile, set).  The
//   R x sizes x nperm null table never exists in memory, nothing is accumulated with atomics, and each sum runs in draw order
//   whatever the geometry: repeated calls, calls on some of the profiles and calls on some of the sets return the same bits.
// The host launches both kernels once per M2 (64 .. 4096), so a launch's LDS is the size its sets need: 4 M2 bytes per wave,
// + 8 GS_CHUNK for k_gs_null.  All waves of a block sort the same M2, so the block barriers inside gs_sort are uniform.
#pragma once

#include "../../include/insider_sample.h"

namespace insider {

constexpr int GS_MAX_SET = 4096;   // largest set: 16 KB of positions per wave
constexpr int GS_CHUNK = 1024;     // null scores kept in LDS between two counting passes
constexpr int GS_PAD = 0x7fffffff; // sorts behind every position (positions are < p <= INT32_MAX)

struct GsScore {
    double es;
    int peak, hits;
};

// a[0 .. M2) ascending; a is private to the calling wave, every wave of the block calls with the same M2 (block barriers).
__device__ __forceinline__ void gs_sort(int *a, int M2, int lane)
{
    for (int k = 2; k <= M2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = lane; q < (M2 >> 1); q += 64) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const int x = a[i], y = a[l];
                if ((x > y) == ((i & k) == 0)) {
                    a[i] = y;
                    a[l] = x;
                }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ double gs_wave_scan(double v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// The enrichment score of the sorted positions a[0 .. m) of a profile with p genes; aw: the profile's |score| by position.
// HITS: also count the positions whose score is not 0.  Every lane returns the same record.
template <bool HITS>
__device__ __forceinline__ GsScore gs_score(const int *a, int m, int64_t p, const double *__restrict__ aw, bool weighted, int lane)
{
    GsScore out;
    out.hits = 0;
    double N = (double)m;
    if (weighted || HITS) {
        double carry = 0.0;
        for (int c = 0; c < m; c += 64) {
            const int idx = c + lane;
            const double w = idx < m ? aw[a[idx]] : 0.0;
            if (HITS) out.hits += __popcll(__ballot(w != 0.0));
            if (weighted) carry = __shfl(carry + gs_wave_scan(w, lane), 63, 64);
        }
        if (weighted) {
            if (carry == 0.0) weighted = false;   // a set of all-zero weight: the classic statistic
            else N = carry;
        }
    }
    const double D = (double)(p - m);
    double hi = -INFINITY, lo = INFINITY, carry = 0.0;
    int ihi = GS_PAD, ilo = GS_PAD;
    for (int c = 0; c < m; c += 64) {
        const int idx = c + lane;
        const bool live = idx < m;
        const int t = live ? a[idx] : 0;
        double P, Pprev;
        if (weighted) {
            P = carry + gs_wave_scan(live ? aw[t] : 0.0, lane);
            Pprev = __shfl_up(P, 1, 64);
            if (lane == 0) Pprev = carry;
            carry = __shfl(P, 63, 64);
        } else {
            P = (double)(idx + 1);
            Pprev = (double)idx;
        }
        if (live) {
            const double miss = (double)(t - idx) / D;
            const double dh = P / N - miss, dl = Pprev / N - miss;
            if (dh > hi) { hi = dh; ihi = idx; }
            if (dl < lo) { lo = dl; ilo = idx; }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double oh = __shfl_xor(hi, d, 64), ol = __shfl_xor(lo, d, 64);
        const int oih = __shfl_xor(ihi, d, 64), oil = __shfl_xor(ilo, d, 64);
        if (oh > hi || (oh == hi && oih < ihi)) { hi = oh; ihi = oih; }
        if (ol < lo || (ol == lo && oil < ilo)) { lo = ol; ilo = oil; }
    }
    const bool up = hi >= -lo;
    out.es = up ? hi : lo;
    out.peak = a[up ? ihi : ilo];
    return out;
}

// Grid-stride over the (profile, set) pairs of one M2 class: sets[0 .. nsets) are the ids of its sets.
__global__ void __launch_bounds__(64) k_gs_observed(const int32_t *__restrict__ rank, const double *__restrict__ aw, int64_t p,
                                                    const int64_t *__restrict__ set_ptr, const int32_t *__restrict__ set_genes,
                                                    const int32_t *__restrict__ sets, int nsets, int64_t ntask, int M2,
                                                    int weighted, int64_t S, double *__restrict__ es, int32_t *__restrict__ peak,
                                                    int32_t *__restrict__ hits)
{
    extern __shared__ int gs_lds[];
    const int lane = threadIdx.x;
    for (int64_t task = blockIdx.x; task < ntask; task += gridDim.x) {
        const int64_t r = task / nsets;
        const int s = sets[task % nsets];
        const int64_t g0 = set_ptr[s];
        const int m = (int)(set_ptr[s + 1] - g0);
        const int32_t *rk = rank + (size_t)r * p;
        for (int i = lane; i < M2; i += 64) gs_lds[i] = i < m ? rk[set_genes[g0 + i]] : GS_PAD;
        __syncthreads();
        gs_sort(gs_lds, M2, lane);
        const GsScore g = gs_score<true>(gs_lds, m, p, aw + (size_t)r * p, weighted != 0, lane);
        if (lane == 0) {
            const size_t o = (size_t)r * S + s;
            es[o] = g.es;
            peak[o] = g.peak;
            hits[o] = g.hits;
        }
        __syncthreads();
    }
}

// Grid-stride over the (profile, size) pairs of one M2 class: sizes[0 .. nsz) are its distinct set sizes, the sets of size
// sizes[z] are size_sets[size_ptr[z] .. size_ptr[z + 1]).  es holds the observed scores (k_gs_observed ran before).
template <int NW>
__global__ void __launch_bounds__(64 * NW) k_gs_null(const double *__restrict__ aw, int64_t p, uint32_t half, uint64_t seed,
                                                     int nperm, const int32_t *__restrict__ sizes,
                                                     const int32_t *__restrict__ size_ptr, const int32_t *__restrict__ size_sets,
                                                     int nsz, int64_t ntask, int M2, int weighted, int64_t S,
                                                     const double *__restrict__ es, int32_t *__restrict__ n_ge,
                                                     int32_t *__restrict__ n_same, double *__restrict__ sum_same)
{
    extern __shared__ int gs_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *a = gs_lds + wave * M2;
    double *draws = (double *)(gs_lds + NW * M2);
    for (int64_t task = blockIdx.x; task < ntask; task += gridDim.x) {
        const int64_t r = task / nsz;
        const int z = (int)(task % nsz);
        const int m = sizes[z];
        const double *awr = aw + (size_t)r * p;
        for (int c0 = 0; c0 < nperm; c0 += GS_CHUNK) {
            const int cn = min(GS_CHUNK, nperm - c0);
            for (int d0 = 0; d0 < cn; d0 += NW) {   // every wave takes every trip: the barriers are the block's
                const int d = d0 + wave;
                const uint32_t key = insider_sample_key(seed, (uint32_t)(c0 + d));
                for (int i = lane; i < M2; i += 64)
                    a[i] = i < m ? (int)insider_sample_phi(key, half, (uint32_t)p, (uint32_t)i) : GS_PAD;
                __syncthreads();
                gs_sort(a, M2, lane);
                const GsScore g = gs_score<false>(a, m, p, awr, weighted != 0, lane);
                if (lane == 0 && d < cn) draws[d] = g.es;
                __syncthreads();
            }
            for (int q = size_ptr[z] + tid; q < size_ptr[z + 1]; q += 64 * NW) {
                const size_t o = (size_t)r * S + size_sets[q];
                const double obs = es[o], mag = fabs(obs);
                const bool pos = obs >= 0.0;
                int ng = c0 ? n_ge[o] : 0, ns = c0 ? n_same[o] : 0;
                double sum = c0 ? sum_same[o] : 0.0, comp = 0.0;   // compensated: the sum is good to an ulp or two of itself
                for (int d = 0; d < cn; ++d) {
                    const double e = draws[d];
                    if ((e >= 0.0) == pos) {
                        ++ns;
                        const double t = sum + e;
                        comp += fabs(sum) >= fabs(e) ? (sum - t) + e : (e - t) + sum;
                        sum = t;
                        ng += fabs(e) >= mag;
                    }
                }
                n_ge[o] = ng;
                n_same[o] = ns;
                sum_same[o] = sum + comp;
            }
            __syncthreads();
        }
    }
}

}   // namespace insider
