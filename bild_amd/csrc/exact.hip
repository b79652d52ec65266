// Exact evidence by enumeration: the kernels (exact.h, exact.cpp).
//
//   * exact_enumerate_kernel: one workgroup per reduction block, one lane per profile.  The local index is split into
//     (trace, combination rank); the rank is unranked in the combinatorial number system (lexicographic rank r of a
//     k-subset of {0 .. n-1} = C(n, k) - 1 - the colex rank of its complement n - 1 - c), a binary search per switch over
//     the binomial table.  Writes the run-length segment rows the likelihood kernels take.
//   * exact_reduce_kernel: one workgroup per block of up to kExactBlock profiles.  Pass 1: the block's largest non-NaN logL
//     m, its NaN count and its MAP profile (lowest index among equal maxima).  Pass 2: sum exp(l - m) and sum l exp(l - m),
//     lane partials in index order, then a fixed tree.  Marginals: every lane OWNS the frames t = lane + 256 f of the
//     block's S x T accumulators in LDS and walks the block's profiles in index order, adding each profile's weight at its
//     own frames -- sums of non-negative terms, no atomics, the order fixed.
//   * exact_fold_kernel: one workgroup per run of blocks of one trajectory; the trajectory's accumulators are carried
//     through its blocks in index order with exp(m_b - M) rescaling (one of the two factors is exactly 1).
// Nothing here depends on the order in which workgroups run: results are bit-identical across calls, chunkings, and the
// other trajectories of the set.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "exact.h"

namespace bild {
namespace {

constexpr int kT = kExactThreads;

__global__ void __launch_bounds__(kT) exact_enumerate_kernel(ExactEnum p)
{
    const ExactBlock blk = p.blocks[blockIdx.x];
    const int k = p.k, K1 = k + 1;
    const int n = p.T[blk.traj] - 1;
    const int64_t C = p.ncomb[blk.traj];
    for (int i = threadIdx.x; i < blk.n; i += kT) {
        const int64_t L = blk.local0 + i;
        const int64_t tr = L / C;
        uint64_t r = (uint64_t)(C - 1 - (L - tr * C));   // colex rank of the complement
        const int64_t row = blk.row0 + i;
        int32_t *ss = p.seg_start + row * K1;
        int32_t *sv = p.seg_state + row * K1;
        const int32_t *th = p.traces + tr * K1;
        ss[0] = 0;
        sv[0] = th[0];
        int hi = n - 1;
        for (int j = 1; j <= k; ++j) {
            const int m = k - j + 1;
            int lo = m - 1;                 // C(m - 1, m) = 0 <= r: lo always qualifies
            int top = hi;
            while (lo < top) {              // largest a in [lo, top] with C(a, m) <= r
                const int mid = (lo + top + 1) >> 1;
                if (p.binom[(int64_t)mid * K1 + m] <= r) lo = mid;
                else top = mid - 1;
            }
            r -= p.binom[(int64_t)lo * K1 + m];
            ss[j] = n - lo;                 // switch frame = c + 1, c = n - 1 - a
            sv[j] = th[j];
            hi = lo - 1;
        }
        p.traj_id[row] = blk.traj;
    }
}

// (value, index) of a MAP candidate: larger value wins, equal values the lower index; idx < 0: none
__device__ __forceinline__ bool map_better(double v, int64_t i, double bv, int64_t bi)
{
    if (i < 0) return false;
    if (bi < 0) return true;
    return v > bv || (v == bv && i < bi);
}

__global__ void __launch_bounds__(kT) exact_reduce_kernel(ExactReduce p)
{
#pragma clang fp contract(off)
    __shared__ double r_m[kT], r_s[kT], r_sl[kT];
    __shared__ int64_t r_i[kT], r_n[kT];
    extern __shared__ double dyn[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const ExactBlock blk = p.blocks[b];
    const double *__restrict__ l = p.logl + blk.row0;
    const double ninf = -__builtin_inf();

    // pass 1: MAP and NaN count; lanes visit their indices in ascending order, so a strict > keeps the lowest index
    double bv = ninf;
    int64_t bi = -1, nn = 0;
    for (int i = tid; i < blk.n; i += kT) {
        const double v = l[i];
        if (isnan(v)) ++nn;
        else if (bi < 0 || v > bv) {
            bv = v;
            bi = i;
        }
    }
    r_m[tid] = bv;
    r_i[tid] = bi;
    r_n[tid] = nn;
    __syncthreads();
    for (int off = kT / 2; off > 0; off >>= 1) {
        if (tid < off && map_better(r_m[tid + off], r_i[tid + off], r_m[tid], r_i[tid])) {
            r_m[tid] = r_m[tid + off];
            r_i[tid] = r_i[tid + off];
        }
        if (tid < off) r_n[tid] += r_n[tid + off];
        __syncthreads();
    }
    const double m = r_i[0] < 0 ? ninf : r_m[0];
    const int64_t map_i = r_i[0], n_nan = r_n[0];
    __syncthreads();

    // pass 2: weights exp(l - m); NaN and -inf candidates weigh 0 and add nothing to either sum
    auto weight = [&](double v) { return (isnan(v) || v == ninf) ? 0.0 : exp(v - m); };
    double s = 0.0, sl = 0.0;
    for (int i = tid; i < blk.n; i += kT) {
        const double v = l[i];
        const double w = weight(v);
        if (w != 0.0) {
            s += w;
            sl += v * w;
        }
    }
    r_s[tid] = s;
    r_sl[tid] = sl;
    __syncthreads();
    for (int off = kT / 2; off > 0; off >>= 1) {
        if (tid < off) {
            r_s[tid] += r_s[tid + off];
            r_sl[tid] += r_sl[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        ExactPart o;
        o.m = m;
        o.s = r_s[0];
        o.sl = r_sl[0];
        o.map_l = map_i < 0 ? __builtin_nan("") : r_m[0];
        o.map_idx = map_i < 0 ? -1 : blk.local0 + map_i;
        o.n_nan = n_nan;
        p.part[b] = o;
    }
    if (!p.marg) return;

    // marginals: LDS [acc: S x T][w: kT][starts: kT x K1][states: kT x K1]
    const int S = p.S, K1 = p.K1, T = p.T[blk.traj];
    double *acc = dyn;
    double *lw = acc + (size_t)S * p.Tm;
    int32_t *lst = reinterpret_cast<int32_t *>(lw + kT);
    int32_t *lsv = lst + kT * K1;
    for (int i = tid; i < S * T; i += kT) acc[i] = 0.0;
    for (int c0 = 0; c0 < blk.n; c0 += kT) {
        const int nc = min(kT, blk.n - c0);
        __syncthreads();
        if (tid < nc) {
            lw[tid] = weight(l[c0 + tid]);
            const int64_t row = blk.row0 + c0 + tid;
            for (int j = 0; j < K1; ++j) {
                lst[tid * K1 + j] = p.seg_start[row * K1 + j];
                lsv[tid * K1 + j] = p.seg_state[row * K1 + j];
            }
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const double wc = lw[c];
            if (wc == 0.0) continue;                // uniform: every lane reads the same word
            const int32_t *st = lst + c * K1;
            const int32_t *sv = lsv + c * K1;
            int j = 0;
            for (int t = tid; t < T; t += kT) {     // j: the interval of frame t (non-decreasing in t)
                while (j + 1 < K1 && st[j + 1] <= t) ++j;
                double *a = acc + (size_t)sv[j] * T + t;
                *a = *a + wc;
            }
        }
    }
    __syncthreads();
    double *out = p.marg + (size_t)b * S * p.Tm;
    for (int s2 = 0; s2 < S; ++s2)
        for (int t = tid; t < T; t += kT) out[(size_t)s2 * p.Tm + t] = acc[(size_t)s2 * T + t];
}

__global__ void __launch_bounds__(kT) exact_fold_kernel(ExactFold p)
{
#pragma clang fp contract(off)
    const ExactRun run = p.runs[blockIdx.x];
    const int j = run.traj;
    const ExactAcc a0 = p.acc[j];
    const ExactPart *__restrict__ part = p.part + run.b0;
    const double ninf = -__builtin_inf();
    if (p.marg) {
        const int T = p.T[j];
        double *am = p.acc_marg + (size_t)j * p.S * p.Tm;
        for (int i = threadIdx.x; i < p.S * T; i += kT) {
            const int s = i / T, t = i - s * T;
            const size_t o = (size_t)s * p.Tm + t;
            double v = am[o], M = a0.M;
            for (int q = 0; q < run.nb; ++q) {
                const double mb = part[q].m;
                if (mb == ninf) continue;           // nothing of weight in the block
                const double x = p.marg[(size_t)(run.b0 + q) * p.S * p.Tm + o];
                if (mb > M) {
                    v = v * exp(M - mb) + x;
                    M = mb;
                } else {
                    v = v + x * exp(mb - M);
                }
            }
            am[o] = v;
        }
    }
    __syncthreads();    // every wave has read the accumulator before it is replaced
    if (threadIdx.x == 0) {
        ExactAcc a = a0;
        for (int q = 0; q < run.nb; ++q) {
            const ExactPart &b = part[q];
            a.n_nan += b.n_nan;
            if (map_better(b.map_l, b.map_idx, a.map_l, a.map_idx)) {
                a.map_l = b.map_l;
                a.map_idx = b.map_idx;
            }
            if (b.m == ninf) continue;
            if (b.m > a.M) {
                const double f = exp(a.M - b.m);
                a.s = a.s * f + b.s;
                a.sl = a.sl * f + b.sl;
                a.M = b.m;
            } else {
                const double f = exp(b.m - a.M);
                a.s = a.s + b.s * f;
                a.sl = a.sl + b.sl * f;
            }
        }
        p.acc[j] = a;
    }
}

} // namespace

size_t exact_reduce_lds(int K1, int S, int Tmax, bool marginals)
{
    if (!marginals) return 0;
    return (size_t)S * Tmax * 8 + (size_t)kT * 8 + (size_t)kT * K1 * 8;
}

int launch_exact_enumerate(const ExactEnum &p, void *stream)
{
    if (p.nblocks <= 0) return 0;
    hipLaunchKernelGGL(exact_enumerate_kernel, dim3(p.nblocks), dim3(kT), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_exact_reduce(const ExactReduce &p, void *stream)
{
    if (p.nblocks <= 0) return 0;
    const size_t lds = exact_reduce_lds(p.K1, p.S, p.Tm, p.marg != nullptr);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void *)exact_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return 1;
    hipLaunchKernelGGL(exact_reduce_kernel, dim3(p.nblocks), dim3(kT), lds, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_exact_fold(const ExactFold &p, void *stream)
{
    if (p.nruns <= 0) return 0;
    hipLaunchKernelGGL(exact_fold_kernel, dim3(p.nruns), dim3(kT), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace bild
