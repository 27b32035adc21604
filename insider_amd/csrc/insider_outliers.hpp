// insider_outliers.hpp — aberrant entries of a fitted model on the resident data set
// (insider_hip_outliers; host driver in insider_hip.hip, section "outlier calls").
//
// With f and r = x - f as in insider_vardecomp.hpp, the standardised residual of entry (i, j) is z = (r - center_j) / scale_j,
// and a selected entry is a call when |z| >= threshold.  The calls come back as a list in ascending gene, then ascending
// sample, with per-gene and per-sample {low, high} counts.  Four stages on the level table T (vd_build_table):
//
// k_ol_flag: the streaming pass of k_vd_stats without its records.  A block of OL_WAVES waves owns GW consecutive genes, its
// waves split the samples (OL_SPL consecutive samples per lane and trip: one 32-byte X load and one 4-byte code load per
// gene; a block covers OL_TRIP samples per trip).  Per entry it forms z (ol_fit, ol_z) and the flag, ORs the four flags of
// the eight lanes that share 32 samples into one word of the BITMAP (one bit per entry, gene-major, ldn / 32 words per
// gene: bit i & 31 of word i >> 5) and counts the low and high calls per lane in integers; a butterfly over the lanes and a
// sum over the waves in LDS give the gene's {low, high}.  Membership is decided here, once.
//
// k_ol_scan: one block; the exclusive scan of the genes' totals in chunks of OL_SCAN_CHUNK with a running carry: int64
// offsets, the grand total at offs[p].
//
// k_ol_fill: one wave per gene walks the gene's bitmap words in sample order (64 words per step, one per lane).  The rank of
// a set bit is the popcount prefix over the lanes plus the bits below it in its own word.  For set bits only the wave
// gathers x and the level-table entries, forms z through the same ol_fit / ol_z, stores (row, col, z) at offset + rank while
// that is below the capacity, and adds to the sample's {low, high} with integer atomics (order-independent).  It never
// re-decides |z| >= threshold: the bitmap's popcount IS the gene's count, so no store leaves the gene's range.
#pragma once

namespace insider {

constexpr int OL_WAVES = 4;                         // waves per block of k_ol_flag and k_ol_fill
constexpr int OL_SPL = 4;                           // consecutive samples per lane and trip
constexpr int OL_TRIP = 64 * OL_WAVES * OL_SPL;     // samples a block of k_ol_flag covers per trip
constexpr int OL_GW = 4;                            // genes per block of k_ol_flag
constexpr int OL_SCAN_THREADS = 256, OL_SCAN_ITEMS = 4;
constexpr int OL_SCAN_CHUNK = OL_SCAN_THREADS * OL_SCAN_ITEMS;   // genes per step of k_ol_scan

// f = g_0 + g_1 + ... in block order for sample i (< n) and G genes; tab(gl, s) = entry s of the level table of gene gl
template <int G, class Tab>
__device__ __forceinline__ void ol_fit(double (&f)[G], const int *__restrict__ lev, const int *__restrict__ lvl_off, int c, int n,
                                       const double *__restrict__ Zc, int m, int SLcat, int i, Tab tab)
{
#pragma unroll
    for (int gl = 0; gl < G; ++gl) f[gl] = 0.0;
    for (int b = 0; b < c; ++b) {
        const int id = lvl_off[b] + lev[(size_t)b * n + i];
#pragma unroll
        for (int gl = 0; gl < G; ++gl) f[gl] += tab(gl, id);
    }
    if (m > 0) {
        double gc[G];
#pragma unroll
        for (int gl = 0; gl < G; ++gl) gc[gl] = 0.0;
        for (int k = 0; k < m; ++k) {
            const double z = Zc[(size_t)k * n + i];
#pragma unroll
            for (int gl = 0; gl < G; ++gl) gc[gl] = fma(z, tab(gl, SLcat + k), gc[gl]);
        }
#pragma unroll
        for (int gl = 0; gl < G; ++gl) f[gl] += gc[gl];
    }
}

// the standardised residual: the one place it is formed
__device__ __forceinline__ double ol_z(double x, double f, double center, double scale)
{
    return ((x - f) - center) / scale;
}

// a scale that can standardise: finite and > 0
__device__ __forceinline__ bool ol_scale_ok(double s) { return s > 0.0 && s < __builtin_inf(); }

// grid = ceil(p / GW) blocks of 64 OL_WAVES threads; dynamic LDS GW SL doubles when STAGED (none otherwise).
// sel_mask: 0 = every entry, else the code bit an entry must carry.  center may be null (0).  bitmap: p x (ldn / 32) words,
// the words below ceil(n / 32) of every gene are written; gcnt: p pairs {low, high}.
template <int GW, bool STAGED>
__global__ void __launch_bounds__(64 * OL_WAVES) k_ol_flag(
    const double *__restrict__ X, const uint8_t *__restrict__ codes, int64_t ldn, int n, int64_t p,
    const int *__restrict__ lev /*c x n, 0-based*/, const int *__restrict__ lvl_off, int c,
    const double *__restrict__ Zc /*m x n*/, int m, int SLcat, const double *__restrict__ T, int SL, int sel_mask,
    const double *__restrict__ center, const double *__restrict__ scale, double threshold, uint32_t *__restrict__ bitmap,
    int *__restrict__ gcnt)
{
    static_assert(OL_SPL == 4, "four samples per lane: one 4-byte code load, eight lanes per bitmap word");
    extern __shared__ double s_tab[];
    __shared__ int s_cnt[OL_WAVES][GW * 2];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t j0 = (int64_t)blockIdx.x * GW;
    const int ng = (int)(p - j0 < GW ? p - j0 : GW);   // genes of this block (>= 1)
    if constexpr (STAGED) {
        for (int t = threadIdx.x; t < ng * SL; t += blockDim.x) s_tab[t] = T[(size_t)j0 * SL + t];
        __syncthreads();
    }
    // table entry s of gene gl (a gene beyond p reads the block's last gene: it is never flagged)
    auto tab = [&](int gl, int s) -> double {
        const int gc = gl < ng ? gl : ng - 1;
        if constexpr (STAGED) return s_tab[gc * SL + s];
        else return T[(size_t)(j0 + gc) * SL + s];
    };
    double ctr[GW], scl[GW];
    bool ok[GW];
    int nlo[GW], nhi[GW];
#pragma unroll
    for (int gl = 0; gl < GW; ++gl) {
        const int64_t j = j0 + (gl < ng ? gl : ng - 1);
        ctr[gl] = center ? center[j] : 0.0;
        scl[gl] = scale[j];
        ok[gl] = gl < ng && ol_scale_ok(scl[gl]);
        nlo[gl] = nhi[gl] = 0;
    }
    const int64_t wpl = ldn >> 5;   // bitmap words per gene
    // the trip count is the wave's: every lane takes part in the shuffles below
    for (int t0 = w * 64 * OL_SPL; t0 < n; t0 += OL_TRIP) {
        const int i0 = t0 + lane * OL_SPL;
        const bool act = i0 < n;   // (then i0 + 3 < ldn: the line holds the four)
        double x[GW][OL_SPL];
        uint32_t cd[GW];
#pragma unroll
        for (int gl = 0; gl < GW; ++gl) {   // every load of the trip in flight before the arithmetic
            cd[gl] = 0;
#pragma unroll
            for (int s = 0; s < OL_SPL; ++s) x[gl][s] = 0.0;
            if (act) {
                const size_t line = (size_t)(j0 + (gl < ng ? gl : ng - 1)) * ldn + i0;
                const double2 lo = *reinterpret_cast<const double2 *>(X + line);
                const double2 hi = *reinterpret_cast<const double2 *>(X + line + 2);
                x[gl][0] = lo.x; x[gl][1] = lo.y; x[gl][2] = hi.x; x[gl][3] = hi.y;
                cd[gl] = *reinterpret_cast<const uint32_t *>(codes + line);
            }
        }
        uint32_t nib[GW];
#pragma unroll
        for (int gl = 0; gl < GW; ++gl) nib[gl] = 0;
#pragma unroll
        for (int s = 0; s < OL_SPL; ++s) {
            const int i = i0 + s;
            const bool in = i < n;   // pad elements carry the train code with x = 0: never called
            double f[GW];
            ol_fit<GW>(f, lev, lvl_off, c, n, Zc, m, SLcat, in ? i : n - 1, tab);
#pragma unroll
            for (int gl = 0; gl < GW; ++gl) {
                const int code = (int)(cd[gl] >> (8 * s)) & 0xff;
                const bool sel = in && ok[gl] && (sel_mask == 0 || (code & sel_mask));
                const double z = ol_z(x[gl][s], f[gl], ctr[gl], scl[gl]);
                const bool call = sel && fabs(z) >= threshold;   // (a NaN z is no call)
                nib[gl] |= (call ? 1u : 0u) << s;
                nlo[gl] += call && z < 0.0 ? 1 : 0;
                nhi[gl] += call && z > 0.0 ? 1 : 0;
            }
        }
        // the eight lanes of 32 consecutive samples form one word
#pragma unroll
        for (int gl = 0; gl < GW; ++gl) {
            uint32_t v = nib[gl] << (4 * (lane & 7));
            v |= __shfl_xor(v, 1);
            v |= __shfl_xor(v, 2);
            v |= __shfl_xor(v, 4);
            if ((lane & 7) == 0 && act && gl < ng) bitmap[(size_t)(j0 + gl) * wpl + (i0 >> 5)] = v;
        }
    }
    // lanes (integer butterfly), then waves
#pragma unroll
    for (int gl = 0; gl < GW; ++gl) {
        int a = nlo[gl], b = nhi[gl];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            a += __shfl_xor(a, o);
            b += __shfl_xor(b, o);
        }
        if (lane == 0) {
            s_cnt[w][2 * gl] = a;
            s_cnt[w][2 * gl + 1] = b;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * ng) {
        int v = 0;
#pragma unroll
        for (int ww = 0; ww < OL_WAVES; ++ww) v += s_cnt[ww][threadIdx.x];
        gcnt[(size_t)j0 * 2 + threadIdx.x] = v;
    }
}

// one block of OL_SCAN_THREADS threads: offs[j] = sum of the totals (low + high) of the genes below j, offs[p] = the grand total
__global__ void __launch_bounds__(OL_SCAN_THREADS) k_ol_scan(const int *__restrict__ gcnt, int64_t p, long long *__restrict__ offs)
{
    constexpr int NW = OL_SCAN_THREADS / 64;
    __shared__ long long s_w[NW];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long carry = 0;
    for (int64_t base = 0; base < p; base += OL_SCAN_CHUNK) {
        const int64_t j = base + (int64_t)threadIdx.x * OL_SCAN_ITEMS;
        long long v[OL_SCAN_ITEMS], mine = 0;
#pragma unroll
        for (int q = 0; q < OL_SCAN_ITEMS; ++q) {
            v[q] = j + q < p ? (long long)gcnt[2 * (j + q)] + gcnt[2 * (j + q) + 1] : 0;
            mine += v[q];
        }
        long long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_w[w] = incl;
        __syncthreads();
        long long before = carry, all = 0;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) {
            if (ww < w) before += s_w[ww];
            all += s_w[ww];
        }
        long long run = before + incl - mine;
#pragma unroll
        for (int q = 0; q < OL_SCAN_ITEMS; ++q) {
            if (j + q < p) offs[j + q] = run;
            run += v[q];
        }
        carry += all;
        __syncthreads();   // the next chunk overwrites s_w
    }
    if (threadIdx.x == 0) offs[p] = carry;
}

// grid = ceil(p / OL_WAVES) blocks of 64 OL_WAVES threads, one wave per gene.  cap: the capacity of rows / cols / zout (they
// may be null when it is 0); scnt: n pairs {low, high}, zeroed before.
__global__ void __launch_bounds__(64 * OL_WAVES) k_ol_fill(
    const double *__restrict__ X, int64_t ldn, int n, int64_t p, const int *__restrict__ lev, const int *__restrict__ lvl_off,
    int c, const double *__restrict__ Zc, int m, int SLcat, const double *__restrict__ T, int SL,
    const double *__restrict__ center, const double *__restrict__ scale, const uint32_t *__restrict__ bitmap,
    const long long *__restrict__ offs, long long cap, int32_t *__restrict__ rows, int32_t *__restrict__ cols,
    double *__restrict__ zout, int *__restrict__ scnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * OL_WAVES + (threadIdx.x >> 6);
    if (j >= p) return;
    const long long o0 = offs[j], o1 = offs[j + 1];
    if (o0 == o1) return;
    const double ctr = center ? center[j] : 0.0, scl = scale[j];
    const double *Tj = T + (size_t)j * SL;
    auto tab = [&](int, int s) -> double { return Tj[s]; };
    const uint32_t *words = bitmap + (size_t)j * (ldn >> 5);
    const int nw = (n + 31) >> 5;
    long long run = o0;
    for (int wb = 0; wb < nw; wb += 64) {   // (uniform: every lane takes part in the shuffles)
        const int wi = wb + lane;
        uint32_t bits = wi < nw ? words[wi] : 0u;
        const int cnt = __popc(bits);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        long long pos = run + (incl - cnt);
        run += __shfl(incl, 63);
        while (bits) {
            const int i = 32 * wi + (__ffs(bits) - 1);
            bits &= bits - 1;
            double f[1];
            ol_fit<1>(f, lev, lvl_off, c, n, Zc, m, SLcat, i, tab);
            const double z = ol_z(X[(size_t)j * ldn + i], f[0], ctr, scl);
            if (pos < cap && pos < o1) {
                rows[pos] = i;
                cols[pos] = (int32_t)j;
                zout[pos] = z;
            }
            atomicAdd(&scnt[2 * (size_t)i + (z > 0.0 ? 1 : 0)], 1);
            ++pos;
        }
    }
}

}  // namespace insider
