// insider_hclust.hpp — agglomerative clustering of embeddings on the device (insider_hip_hclust; host driver in
// insider_hip.hip, section "agglomerative clustering").  include/insider_hip.h states the definitions and the tie rule; this
// file states how the device meets them.
//
// Linkages.  Exactly two are offered, the ones that are REDUCIBLE (merging A and B never brings the new cluster closer to a
// third than the nearer of A and B was, so a cluster whose nearest neighbour was not merged keeps it) and whose distance is a
// function of the clusters' sums S and sizes n (so a cluster is D + 1 numbers, and a distance is one dot product of two means
// mu = S / n): average linkage of cosine distances, d = 1 - mu_A . mu_B over unit members, and Ward, d = n_A n_B / (n_A + n_B)
// |mu_A - mu_B|^2.  Single and complete linkage are not functions of the sums (they need the members); centroid and median
// linkage are functions of the sums but not reducible (a merge can move a centroid closer to a third cluster, so heights
// invert and kept neighbours go wrong).  None of the four is offered.
//
// State per cluster id c < 2 N - 1 (ids < N are the points, the r-th merge of the run is N + r): S[c] (D doubles, id-major),
// n[c], alive[c], nn[c], nn_d[c].  A cluster is STALE when it is alive and nn[c] is -1 or no longer alive: staleness is read
// off nn and alive, there is no flag to keep in step.
//
// One round (the loop is the host's, bounded by max_rounds; no kernel waits on another block):
//   lists     k_hc_count / k_hc_offsets / k_hc_compact, mode 0: the alive ids and the stale ids, each in ascending id (an
//             ordered compaction: counts per block of 256 ids, one block scans the counts, ranks by ballot; no atomics);
//   k_hc_cprep  twice: the means of the alive clusters (the base) and of the stale ones (the queries) in MFMA operand order
//             (tiles of 16, K4 = D rounded up to 4), beside each its id, n and h = |mu|^2 (separately rounded products in index
//             order); padding columns are zero and masked by index;
//   k_hc_nn<KS>  a wave owns 16 queries (A operand, up to 4 KS doubles per lane for the whole kernel), a block of 4 waves
//             streams the base NT tiles at a time through LDS; one chain of K4 / 4 v_mfma_f64_16x16x4 per tile gives
//             mu_q . mu_c (lane g = lane >> 4, t = lane & 15, register r: query g + 4 r, base column t); the epilogue forms d
//             from the per-row and per-column (n, h); each lane keeps its best under a strict < (the base ascends in id, so
//             the lower id stays), itself excluded by id; one xor-butterfly over the 16 lanes of a query merges under the total
//             order (d ascending, id ascending).  No LDS lists, no atomics.  d is bitwise symmetric in (A, B): the chain
//             multiplies the same pairs of coordinates in the same order either way and the epilogue is symmetric in its
//             operands, so two clusters always agree on their distance;
//   pairs     the same three kernels, mode 1: the ids a with nn[a] = b > a and nn[b] = a, ascending;
//   k_hc_merge  a wave per pair: record (a, b, nn_d[a], n_a + n_b), S_new = S_a + S_b, a and b die, the new id is alive with
//             nn = -1 (stale by the rule above, like every cluster whose nn just died).
// The host reads one record of three ints per round.
#pragma once

namespace insider {

constexpr int HC_NW = 4;          // waves per block of k_hc_nn: 64 queries per block
constexpr int HC_MAX_D = 63;      // coordinates of a point (one lane per coordinate in k_hc_merge)

// |v|^2 of D strided doubles, products and sums rounded one by one in index order (what numpy's ss + v * v gives)
__device__ __forceinline__ double hc_sumsq(const double *v, int D, int stride)
{
#pragma clang fp contract(off)
    double ss = 0.0;
    for (int d = 0; d < D; ++d) {
        const double x = v[(size_t)d * stride];
        const double xx = x * x;
        ss = ss + xx;
    }
    return ss;
}

// grid = D blocks of 256 threads: mean[d] = (the sum of coordinate d over the n points) / n; thread i adds the points
// i, i + 256, ... in that order, thread 0 the 256 results in thread order.
__global__ void __launch_bounds__(256) k_hc_mean(const double *__restrict__ X /*D x n*/, int64_t n, int D, double *__restrict__ mean)
{
    __shared__ double s_s[256];
    const int d = blockIdx.x;
    double sum = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) sum += X[(size_t)j * D + d];
    s_s[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = 0.0;
        for (int e = 0; e < 256; ++e) sum += s_s[e];
        mean[d] = sum / (double)n;
    }
}

// One thread per point j < n of the id-major matrix S (the points are its first n rows of D): cosine (metric 0) x = p / |p|
// in place, a point of norm 0 is dead; Euclidean (metric 1) x = p - mean.  size = 1, nn = -1.
__global__ void __launch_bounds__(256) k_hc_points(double *__restrict__ S, int64_t n, int D, int metric,
                                                   const double *__restrict__ mean, int32_t *__restrict__ size,
                                                   int32_t *__restrict__ alive, int32_t *__restrict__ nn)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double *c = S + (size_t)j * D;
    int ok = 1;
    if (metric == 0) {
        const double nrm = sqrt(hc_sumsq(c, D, 1));
        ok = nrm > 0.0;
        if (ok)
            for (int d = 0; d < D; ++d) c[d] = c[d] / nrm;
    } else {
        for (int d = 0; d < D; ++d) c[d] = c[d] - mean[d];
    }
    size[j] = 1;
    alive[j] = ok;
    nn[j] = -1;
}

// What id c contributes to the lists.  mode 0: bit 0 = alive, bit 1 = stale (alive, and force or nn = -1 or nn dead).
// mode 1: bit 0 = the lower id of a reciprocal pair.  nn holds -1 or an id < top.
__device__ __forceinline__ int hc_flags(int mode, int force, int64_t c, int64_t top, const int32_t *alive, const int32_t *nn)
{
    if (c >= top || !alive[c]) return 0;
    const int b = nn[c];
    if (mode == 0) return 1 | ((force || b < 0 || !alive[b]) ? 2 : 0);
    return (int64_t)b > c && nn[b] == (int32_t)c ? 1 : 0;
}

// grid = ceil(top / 256) blocks of 256: bc[2 blk + i] = the ids of block blk with bit i.
__global__ void __launch_bounds__(256) k_hc_count(int mode, int force, int64_t top, const int32_t *__restrict__ alive,
                                                  const int32_t *__restrict__ nn, int *__restrict__ bc)
{
    const int f = hc_flags(mode, force, (int64_t)blockIdx.x * 256 + threadIdx.x, top, alive, nn);
    const int c0 = __syncthreads_count(f & 1), c1 = __syncthreads_count(f & 2);
    if (threadIdx.x == 0) {
        bc[2 * (size_t)blockIdx.x] = c0;
        bc[2 * (size_t)blockIdx.x + 1] = c1;
    }
}

// One block: bc becomes its exclusive prefix over the nb blocks (both columns), tot[0..1] the totals; thread i owns a run of
// ceil(nb / 256) consecutive blocks.
__global__ void __launch_bounds__(256) k_hc_offsets(int *__restrict__ bc, int64_t nb, int *__restrict__ tot)
{
    __shared__ int s_t[2][256];
    const int64_t per = (nb + 255) / 256, lo = threadIdx.x * per, hi = lo + per < nb ? lo + per : nb;
    int own0 = 0, own1 = 0;
    for (int64_t e = lo; e < hi; ++e) {
        own0 += bc[2 * e];
        own1 += bc[2 * e + 1];
    }
    s_t[0][threadIdx.x] = own0;
    s_t[1][threadIdx.x] = own1;
    __syncthreads();
    int run0 = 0, run1 = 0;
    for (int e = 0; e < (int)threadIdx.x; ++e) {
        run0 += s_t[0][e];
        run1 += s_t[1][e];
    }
    for (int64_t e = lo; e < hi; ++e) {
        const int c0 = bc[2 * e], c1 = bc[2 * e + 1];
        bc[2 * e] = run0;
        bc[2 * e + 1] = run1;
        run0 += c0;
        run1 += c1;
    }
    if (threadIdx.x == 255) {   // (its run is the last, possibly empty: run = the grand total)
        tot[0] = run0;
        tot[1] = run1;
    }
}

// grid as k_hc_count, bc = k_hc_offsets' output: list0 / list1 = the ids with bit 0 / bit 1, ascending (list1 may be NULL
// when the mode sets no bit 1).  Rank inside the block: lower lanes by ballot, lower waves through LDS.
__global__ void __launch_bounds__(256) k_hc_compact(int mode, int force, int64_t top, const int32_t *__restrict__ alive,
                                                    const int32_t *__restrict__ nn, const int *__restrict__ bc,
                                                    int32_t *__restrict__ list0, int32_t *__restrict__ list1)
{
    __shared__ int s_w[2][4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int f = hc_flags(mode, force, c, top, alive, nn);
    const unsigned long long m0 = __builtin_amdgcn_ballot_w64((f & 1) != 0), m1 = __builtin_amdgcn_ballot_w64((f & 2) != 0);
    if (lane == 0) {
        s_w[0][w] = __popcll(m0);
        s_w[1][w] = __popcll(m1);
    }
    __syncthreads();
    int r0 = bc[2 * (size_t)blockIdx.x], r1 = bc[2 * (size_t)blockIdx.x + 1];
    for (int e = 0; e < w; ++e) {
        r0 += s_w[0][e];
        r1 += s_w[1][e];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (f & 1) list0[r0 + __popcll(m0 & below)] = (int32_t)c;
    if (f & 2) list1[r1 + __popcll(m1 & below)] = (int32_t)c;
}

// One thread per column j < cntpad (cnt clusters listed, cntpad >= cnt a multiple of 16 and within the arrays):
// the mean of cluster list[j] in operand order (the layout of k_nn_prep), its id, n (as a double) and h = |mu|^2; columns
// beyond cnt are zero with id -1.
__global__ void __launch_bounds__(256) k_hc_cprep(const int32_t *__restrict__ list, int cnt, int cntpad,
                                                  const double *__restrict__ S, const int32_t *__restrict__ size, int D, int K4,
                                                  double *__restrict__ Cp, int32_t *__restrict__ cid, double *__restrict__ cn,
                                                  double *__restrict__ ch)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= cntpad) return;
    double *o = Cp + (size_t)(j >> 4) * 16 * K4 + (j & 15);
    const bool ok = j < cnt;
    const int id = ok ? list[j] : -1;
    const double n = ok ? (double)size[id] : 1.0;
    const double *s = S + (size_t)(ok ? id : 0) * D;
    for (int d = 0; d < K4; ++d) o[16 * d] = ok && d < D ? s[d] / n : 0.0;
    cid[j] = id;
    cn[j] = n;
    ch[j] = hc_sumsq(o, D, 16);
}

// a comes before b: distance ascending, id ascending
__device__ __forceinline__ bool hc_before(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// grid = ceil(ns / 64) blocks of 256 threads.  Qp / qid / qn / qh: k_hc_cprep's output for the ns stale clusters (padded to
// 16), Cp / cid / cn / ch: for the na alive ones (napad columns, a multiple of 16 NT, columns >= na masked).  Writes nn and nn_d of every query (-1 / +inf when it has no finite candidate).
// KS = ceil(K4 / 16).  Dynamic LDS: NT 16 K4 doubles of means, NT 16 doubles of n and of h, NT 16 ints of ids.
template <int KS>
__global__ void __launch_bounds__(256) k_hc_nn(const double *__restrict__ Qp, const int32_t *__restrict__ qid,
                                               const double *__restrict__ qn, const double *__restrict__ qh,
                                               int ns, const double *__restrict__ Cp,
                                               const int32_t *__restrict__ cid, const double *__restrict__ cn,
                                               const double *__restrict__ ch, int na, int napad, int K4,
                                               int NT, int metric, int32_t *__restrict__ nn, double *__restrict__ nn_d)
{
    extern __shared__ double s_hc[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    double *s_b = s_hc, *s_n = s_hc + NT * 16 * K4, *s_h = s_n + NT * 16;
    int *s_id = reinterpret_cast<int *>(s_h + NT * 16);

    const int q0 = (blockIdx.x * HC_NW + w) * 16;   // this wave's first query
    const bool active = q0 < ns;                      // wave-uniform
    double a[4 * KS];
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s) a[s] = active && 4 * s < K4 ? Qp[(size_t)q0 * K4 + 64 * s + lane] : 0.0;
    double bd[4], mn[4], mh[4];
    int bi[4], me[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + g + 4 * r;
        const bool ok = qi < ns;
        me[r] = ok ? qid[qi] : -1;
        mn[r] = ok ? qn[qi] : 1.0;
        mh[r] = ok ? qh[qi] : 0.0;
        bd[r] = __builtin_inf();
        bi[r] = -1;
    }
    const int nstage = NT * 16 * K4;
#pragma unroll 1
    for (int j0 = 0; j0 < napad; j0 += 16 * NT) {
        __syncthreads();   // the tiles of the last step are consumed
        const double *src = Cp + (size_t)j0 * K4;
        for (int e = threadIdx.x; e < nstage; e += 256) s_b[e] = src[e];
        if (threadIdx.x < 16 * NT) {
            s_n[threadIdx.x] = cn[j0 + threadIdx.x];
            s_h[threadIdx.x] = ch[j0 + threadIdx.x];
            s_id[threadIdx.x] = cid[j0 + threadIdx.x];
        }
        __syncthreads();
        if (!active) continue;
#pragma unroll 1
        for (int tile = 0; tile < NT; ++tile) {
            const double *bl = s_b + tile * 16 * K4 + lane;
            d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4 * KS; ++s)
                if (4 * s < K4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bl[64 * s], acc, 0, 0, 0);
            const int j = j0 + tile * 16 + t;
            const int id = s_id[tile * 16 + t];
            const double nc = s_n[tile * 16 + t], hc = s_h[tile * 16 + t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double d;
                if (metric == 1) {
                    const double wgt = (mn[r] * nc) / (mn[r] + nc);
                    d = fmax(0.0, wgt * ((mh[r] + hc) - 2.0 * acc[r]));
                } else {
                    d = 1.0 - acc[r];
                }
                const bool take = j < na && id != me[r] && d < bd[r];
                bd[r] = take ? d : bd[r];
                bi[r] = take ? id : bi[r];
            }
        }
    }
    if (!active) return;
    // the 16 lanes of a group hold the bests of disjoint parts of the base: a butterfly merges them
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const double od = __shfl_xor(bd[r], m);
            const int oi = __shfl_xor(bi[r], m);
            const bool theirs = oi >= 0 && (bi[r] < 0 || hc_before(od, oi, bd[r], bi[r]));
            bd[r] = theirs ? od : bd[r];
            bi[r] = theirs ? oi : bi[r];
        }
    }
    if (t == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (me[r] >= 0) {
                nn[me[r]] = bi[r];
                nn_d[me[r]] = bd[r];
            }
        }
    }
}

// grid = ceil(maxpairs / 4) blocks of 256 threads, a wave per pair r < *npairs_dev (waves beyond leave): a = pairs[r],
// b = nn[a], the new cluster N + base + r.  lane = coordinate (D <= 63); lane 0 writes the record and the state.
__global__ void __launch_bounds__(256) k_hc_merge(const int32_t *__restrict__ pairs, const int *__restrict__ npairs_dev, int64_t N,
                                                  int base, int D, double *__restrict__ S, int32_t *__restrict__ size,
                                                  int32_t *__restrict__ alive, int32_t *__restrict__ nn,
                                                  const double *__restrict__ nn_d, int32_t *__restrict__ rec_a,
                                                  int32_t *__restrict__ rec_b, double *__restrict__ rec_d,
                                                  int32_t *__restrict__ rec_n)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= *npairs_dev) return;
    const int a = pairs[r], b = nn[a];
    const int64_t c = N + base + r;
    if (lane < D) S[(size_t)c * D + lane] = S[(size_t)a * D + lane] + S[(size_t)b * D + lane];
    if (lane == 0) {
        const int n = size[a] + size[b];
        size[c] = n;
        alive[a] = 0;
        alive[b] = 0;
        alive[c] = 1;
        nn[c] = -1;
        rec_a[base + r] = a;
        rec_b[base + r] = b;
        rec_d[base + r] = nn_d[a];
        rec_n[base + r] = n;
    }
}

}  // namespace insider
