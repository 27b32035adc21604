// insider_kmeans.hpp — k-means (Lloyd) of embeddings on the device (insider_hip_kmeans; host driver in insider_hip.hip, section
// "k-means").  include/insider_hip.h states the definitions; this file states how the device meets them.
//
// Points.  k_nn_prep (insider_neighbors.hpp, unchanged) brings the points into MFMA operand order once (tiles of 16 points,
// normalised under cosine, dead columns marked); k_km_points rewrites the point-major copy in place with the same expression
// (x = p / |p|), so the grouped sums read D contiguous doubles per member, and stores |x|^2 (index order) for the Euclidean
// distance.  k_km_cprep brings the k centres into operand order once per iteration, padded with zero columns to a whole
// number of staged tiles, with h_j = |c_j|^2 / 2 (Euclidean) or 0 (cosine).
//
// k_km_assign<KS>: a wave owns 16 points (A operand, up to 4 KS doubles per lane for the whole kernel), a block of 4 waves
// streams the centres NT tiles at a time through LDS (a flat copy of operand order, one ds_read_b64 per MFMA).  One chain of
// K4 / 4 v_mfma_f64_16x16x4 gives the 16 x 16 products: lane (g = lane >> 4, t = lane & 15), register r holds (point g + 4 r,
// centre t of the tile); the score is the product minus h_j.  The chain of a pair is the same instruction sequence wherever
// the pair falls.  Each lane keeps the best and the runner-up of the centres it sees (they come in ascending index, so a
// strict > keeps the lower index); at the end a butterfly over the 16 lanes of a point merges the pairs under the total order
// (score descending, index ascending).  The block writes label, second and both distances of its 64 points and one partial of
// the inertia and of the changed labels (its 64 values added in point order by one thread); k_km_reduce adds the partials in
// a fixed order into the iteration's record, the only thing the host reads per iteration.
//
// Update: a stable counting sort of the alive points by label, then a sum per cluster in member order.  The points are cut
// into B <= 256 fixed chunks, one wave each: k_km_hist counts the labels of a chunk in LDS (integer atomics) into row b of a
// B x k table; k_km_colscan turns every column into its exclusive prefix over the chunks and the cluster's size; k_km_scan
// scans the sizes into the clusters' first slots; k_km_scatter walks a chunk again 64 points at a time in ascending index, a
// lane's slot being the cluster's next free slot plus the number of lower lanes with its label (ballots over the label's
// bits: no atomics, so the member list of a cluster ascends).  k_km_sum: a block per cluster, lane = coordinate, wave w adds
// the 64-member groups w, w + 4, ... of the list in order, the four partials are added in wave order, then one division per
// coordinate (by n_j, or by the norm of the sum under cosine).  No floating-point atomics anywhere: every sum has one order.
//
// No kernel waits on another block; the Lloyd loop is the host's, bounded by max_iter.
#pragma once

namespace insider {

constexpr int KM_MAX_K = 4096;      // clusters (an int histogram of k bins fits LDS: 16 KB)
constexpr int KM_NW = 4;            // waves per block of k_km_assign: 64 points per block
constexpr int KM_MAX_CHUNKS = 256;  // chunks of the counting sort

// One thread per point j < n of the point-major matrix X (D x n): under cosine x = p / |p| in place, by the expression of
// k_nn_prep (a dead point stays as it is: nothing reads it); xx[j] = the sum of squares of x in index order.
__global__ void __launch_bounds__(256) k_km_points(double *__restrict__ X, int64_t n, int D, int metric, double *__restrict__ xx)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double *c = X + (size_t)j * D;
    if (metric == 0) {
        double ss = 0.0;
        for (int d = 0; d < D; ++d) ss = fma(c[d], c[d], ss);
        const double nrm = sqrt(ss);
        if (nrm > 0.0)
            for (int d = 0; d < D; ++d) c[d] = c[d] / nrm;
    }
    double s2 = 0.0;
    for (int d = 0; d < D; ++d) s2 = fma(c[d], c[d], s2);
    xx[j] = s2;
}

// Centre j < k of restart r starts from point pick[j]: a copy of D doubles.
__global__ void __launch_bounds__(256) k_km_gather(const double *__restrict__ X, const int32_t *__restrict__ pick, int k, int D,
                                                   double *__restrict__ Cm)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)k * D) return;
    const int j = (int)(e / D), d = (int)(e % D);
    Cm[e] = X[(size_t)pick[j] * D + d];
}

// One thread per centre column j < kpad: operand order (the layout of k_nn_prep), zero beyond k and beyond D, and h.
__global__ void __launch_bounds__(256) k_km_cprep(const double *__restrict__ Cm /*D x k*/, int k, int kpad, int D, int K4,
                                                  int metric, double *__restrict__ Cp, double *__restrict__ h)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= kpad) return;
    double *o = Cp + (size_t)(j >> 4) * 16 * K4 + (j & 15);
    const double *c = Cm + (size_t)j * D;
    double ss = 0.0;
    for (int d = 0; d < K4; ++d) {
        const double v = j < k && d < D ? c[d] : 0.0;
        ss = fma(v, v, ss);
        o[16 * d] = v;
    }
    h[j] = metric == 1 ? 0.5 * ss : 0.0;
}

// a comes before b: score descending, index ascending
__device__ __forceinline__ bool km_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// grid = ceil(n / 64) blocks of 256 threads.  Xp / palive: k_nn_prep's output for the points (padded to 16); Cp / h:
// k_km_cprep's (kpad a multiple of 16 NT).  label is read (the last assignment) and written.  KS = ceil(K4 / 16).
// Dynamic LDS: NT 16 K4 doubles of centres, NT 16 doubles of h.
template <int KS>
__global__ void __launch_bounds__(256) k_km_assign(const double *__restrict__ Xp, const int *__restrict__ palive, int64_t n,
                                                   const double *__restrict__ Cp, const double *__restrict__ h, int k, int kpad,
                                                   int K4, int NT, int metric, const double *__restrict__ xx,
                                                   int32_t *__restrict__ label, int32_t *__restrict__ second,
                                                   double *__restrict__ dist, double *__restrict__ dist2,
                                                   double *__restrict__ part_inertia, int *__restrict__ part_changed)
{
    extern __shared__ double s_km[];
    __shared__ double s_d[16 * KM_NW];
    __shared__ int s_c[16 * KM_NW];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, t = lane & 15;
    double *s_b = s_km, *s_h = s_km + NT * 16 * K4;

    const int64_t q0 = ((int64_t)blockIdx.x * KM_NW + w) * 16;   // this wave's first point
    const bool active = q0 < n;                                   // wave-uniform
    double a[4 * KS];
#pragma unroll
    for (int s = 0; s < 4 * KS; ++s) a[s] = active && 4 * s < K4 ? Xp[(size_t)q0 * K4 + 64 * s + lane] : 0.0;
    double b1[4], b2[4];
    int i1[4], i2[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        b1[r] = b2[r] = -__builtin_inf();
        i1[r] = i2[r] = -1;
    }
    const int nstage = NT * 16 * K4;
#pragma unroll 1
    for (int j0 = 0; j0 < kpad; j0 += 16 * NT) {
        __syncthreads();   // the tiles of the last step are consumed
        const double *src = Cp + (size_t)j0 * K4;
        for (int e = threadIdx.x; e < nstage; e += 256) s_b[e] = src[e];
        if (threadIdx.x < 16 * NT) s_h[threadIdx.x] = h[j0 + threadIdx.x];
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
            const double hj = s_h[tile * 16 + t];
            const bool valid = j < k;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double s = metric == 1 ? acc[r] - hj : acc[r];
                const bool first = valid && s > b1[r], next = valid && !first && s > b2[r];
                b2[r] = first ? b1[r] : (next ? s : b2[r]);
                i2[r] = first ? i1[r] : (next ? j : i2[r]);
                b1[r] = first ? s : b1[r];
                i1[r] = first ? j : i1[r];
            }
        }
    }
    // the 16 lanes of a group hold 16 (best, runner-up) pairs of disjoint centres per point: a butterfly merges them
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const double o1 = __shfl_xor(b1[r], m), o2 = __shfl_xor(b2[r], m);
            const int oi1 = __shfl_xor(i1[r], m), oi2 = __shfl_xor(i2[r], m);
            const bool mine = km_before(b1[r], i1[r], o1, oi1) || oi1 < 0;
            const double ls = mine ? o1 : b1[r], ws = mine ? b2[r] : o2;   // the loser of the firsts, the winner's second
            const int li = mine ? oi1 : i1[r], wi = mine ? i2[r] : oi2;
            const bool lose = li >= 0 && (wi < 0 || km_before(ls, li, ws, wi));
            b1[r] = mine ? b1[r] : o1;
            i1[r] = mine ? i1[r] : oi1;
            b2[r] = lose ? ls : ws;
            i2[r] = lose ? li : wi;
        }
    }
    if (t == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t qi = q0 + g + 4 * r;
            double d1 = 0.0;
            int chg = 0;
            if (qi < n) {
                const bool ok = palive[qi] != 0;
                const double nan = __builtin_nan("");
                double d2 = nan;
                if (ok) {
                    const double x2 = xx[qi];
                    d1 = metric == 1 ? fmax(0.0, x2 - 2.0 * b1[r]) : 1.0 - b1[r];
                    if (i2[r] >= 0) d2 = metric == 1 ? fmax(0.0, x2 - 2.0 * b2[r]) : 1.0 - b2[r];
                    chg = label[qi] != i1[r];
                }
                label[qi] = ok ? i1[r] : -1;
                second[qi] = ok ? i2[r] : -1;
                dist[qi] = ok ? d1 : nan;
                dist2[qi] = d2;
            }
            s_d[16 * w + g + 4 * r] = d1;
            s_c[16 * w + g + 4 * r] = chg;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        int cnt = 0;
        for (int e = 0; e < 16 * KM_NW; ++e) {
            sum += s_d[e];
            cnt += s_c[e];
        }
        part_inertia[blockIdx.x] = sum;
        part_changed[blockIdx.x] = cnt;
    }
}

// One block: rec[0] = the sum of the nb partials of the inertia, rec[1] = the changed labels; thread i adds the partials
// i, i + 256, ... in that order, thread 0 the 256 results in thread order.
__global__ void __launch_bounds__(256) k_km_reduce(const double *__restrict__ part_inertia, const int *__restrict__ part_changed,
                                                   int nb, double *__restrict__ rec)
{
    __shared__ double s_s[256];
    __shared__ long long s_n[256];
    double sum = 0.0;
    long long cnt = 0;
    for (int e = threadIdx.x; e < nb; e += 256) {
        sum += part_inertia[e];
        cnt += part_changed[e];
    }
    s_s[threadIdx.x] = sum;
    s_n[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = 0.0;
        cnt = 0;
        for (int e = 0; e < 256; ++e) {
            sum += s_s[e];
            cnt += s_n[e];
        }
        rec[0] = sum;
        rec[1] = (double)cnt;
    }
}

// grid = B blocks of 64 threads, block b owns the points [b chunk, (b + 1) chunk): table[b][j] = its points with label j.
// Dynamic LDS: k ints.
__global__ void __launch_bounds__(64) k_km_hist(const int32_t *__restrict__ label, int64_t n, int64_t chunk, int k,
                                                int *__restrict__ table)
{
    extern __shared__ int s_hist[];
    for (int j = threadIdx.x; j < k; j += 64) s_hist[j] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 64) {
        const int l = label[i];
        if (l >= 0) atomicAdd(&s_hist[l], 1);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 64) table[(size_t)blockIdx.x * k + j] = s_hist[j];
}

// One thread per cluster j: table[b][j] becomes the exclusive prefix over the chunks b < B, size[j] the total.
__global__ void __launch_bounds__(256) k_km_colscan(int *__restrict__ table, int B, int k, int32_t *__restrict__ size)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    int run = 0;
    for (int b = 0; b < B; ++b) {
        const int c = table[(size_t)b * k + j];
        table[(size_t)b * k + j] = run;
        run += c;
    }
    size[j] = run;
}

// One block: first[j] = size[0] + ... + size[j - 1], j < k <= 4096 (16 consecutive clusters per thread).
__global__ void __launch_bounds__(256) k_km_scan(const int32_t *__restrict__ size, int k, int *__restrict__ first)
{
    __shared__ int s_t[256];
    const int j0 = threadIdx.x * 16;
    int own = 0;
    for (int e = 0; e < 16; ++e) own += j0 + e < k ? size[j0 + e] : 0;
    s_t[threadIdx.x] = own;
    __syncthreads();
    int run = 0;
    for (int e = 0; e < (int)threadIdx.x; ++e) run += s_t[e];
    for (int e = 0; e < 16; ++e) {
        if (j0 + e < k) {
            first[j0 + e] = run;
            run += size[j0 + e];
        }
    }
}

// grid = B blocks of 64 threads, the chunks of k_km_hist.  member[first[j] + table[b][j] + rank] = i for every alive point i
// of the chunk, rank = the chunk's earlier points with label j: 64 points at a time in ascending index, the lanes with one
// label found by ballots over the label's 12 bits.  Dynamic LDS: k ints (the clusters' next free slots).
__global__ void __launch_bounds__(64) k_km_scatter(const int32_t *__restrict__ label, int64_t n, int64_t chunk, int k,
                                                   const int *__restrict__ table, const int *__restrict__ first,
                                                   int32_t *__restrict__ member)
{
    extern __shared__ int s_next[];
    const int lane = threadIdx.x;
    for (int j = lane; j < k; j += 64) s_next[j] = first[j] + table[(size_t)blockIdx.x * k + j];
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const int l = i < hi ? label[i] : -1;
        const bool ok = l >= 0;
        unsigned long long same = __builtin_amdgcn_ballot_w64(ok);
#pragma unroll
        for (int bit = 0; bit < 12; ++bit) {
            const bool set = ((l >> bit) & 1) != 0;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(set);
            same &= set ? m : ~m;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull)), tot = __popcll(same);
        int slot = 0;
        if (ok) slot = s_next[l] + rank;
        wave_sync();   // every lane has read before the last lane of a label moves its slot on
        if (ok) {
            member[slot] = (int32_t)i;
            if (rank == tot - 1) s_next[l] = slot + 1;
        }
        wave_sync();
    }
}

// grid = k blocks of 256 threads: cluster j = blockIdx.x, lane = coordinate d < D (D <= 63), wave w adds the 64-member groups
// w, w + 4, ... of the cluster's list in order; the four partials are added in wave order.  Euclidean: c = sum / n_j; cosine:
// c = sum / |sum|, the norm in index order; an empty cluster, or a sum of norm 0, keeps its centre.
__global__ void __launch_bounds__(256) k_km_sum(const double *__restrict__ X /*D x n*/, const int32_t *__restrict__ member,
                                                const int *__restrict__ first, const int32_t *__restrict__ size, int D,
                                                int metric, double *__restrict__ Cm /*D x k*/)
{
    __shared__ double s_p[4][64];
    const int j = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nj = size[j];
    if (nj == 0) return;   // block-uniform
    const int32_t *mem = member + first[j];
    double acc = 0.0;
    for (int m0 = 64 * w; m0 < nj; m0 += 256) {
        const int cnt = nj - m0 < 64 ? nj - m0 : 64;
        const int mine = lane < cnt ? mem[m0 + lane] : 0;
#pragma unroll 8
        for (int u = 0; u < cnt; ++u) {
            const int i = __shfl(mine, u);
            acc += lane < D ? X[(size_t)i * D + lane] : 0.0;
        }
    }
    s_p[w][lane] = acc;
    __syncthreads();
    if (w != 0) return;
    const double sum = ((s_p[0][lane] + s_p[1][lane]) + s_p[2][lane]) + s_p[3][lane];
    double den = (double)nj;
    if (metric == 0) {
        s_p[0][lane] = sum;
        wave_sync();
        double ss = 0.0;
        for (int d = 0; d < D; ++d) ss = fma(s_p[0][d], s_p[0][d], ss);
        den = sqrt(ss);
        if (!(den > 0.0)) return;   // wave-uniform
    }
    if (lane < D) Cm[(size_t)j * D + lane] = sum / den;
}

}  // namespace insider
