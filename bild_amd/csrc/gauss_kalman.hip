// Per-frame moments of GenericGaussianModel profiles (bild_gauss_kalman_segments, bild_gauss_kalman_mixture:
// gauss_kalman.cpp).
//
// A job is one window of one (trajectory, dimension, state): the data vector y of its valid frames (gauss.hip), its
// covariance C = L L^T and, per missing frame t of the window, the covariance c_t of the missing coordinate with y.  The
// record of a job holds, per entry j, L_jj and z_j = (L^-1 y)_j -- the one-step predictive moments, the innovation and the
// term follow from them and the data -- and, per missing frame, the conditional mean and variance of the coordinate given
// the whole window.  Three kernels, one workgroup per job or per (candidate, interval, dimension):
//   * gauss_kal_factor_kernel: the left-looking column sweep of gauss_sens_factor_kernel over the augmented matrix
//     [C; c_t^T (one row per missing frame); y^T], so that one pass yields L, u_t = L^-1 c_t and z; then one lane per
//     missing frame forms u_t.z and u_t.u_t.  Scratch slot: (n + nmiss + 1) x n doubles.
//   * gauss_kal_solve_kernel: windows whose frames are consecutive, against a leading block of the shared Toeplitz factor
//     of their (state, dimension) (built by gauss_sens_factor_kernel at P = 0): y in LDS, right-looking.
//   * gauss_kal_scatter_kernel: the per-frame outputs of one (candidate, interval, dimension) from its job's record.
// A job's record depends on the job alone and a frame's outputs on the record and the data, so a candidate's outputs do
// not depend on the batch, its order, duplicates or the chunking.  Contraction is off: the sums are written as fma where
// they are meant to be.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_kalman.h"

namespace bild {
namespace {

constexpr int kThreads = 256;
constexpr int kScatterThreads = 64;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// covariance of entries i, j of the data vector (gauss_sens.hip: sens_cov)
__device__ __forceinline__ double kal_cov(const GaussKalSet &p, const int32_t *__restrict__ u, int i, int j)
{
#pragma clang fp contract(off)
    const double *__restrict__ msd = p.msd;
    if (p.order == 0) return 0.5 * (p.msd_inf - msd[abs(u[i] - u[j])]);
    const double a = msd[abs(u[i + 1] - u[j])], b = msd[abs(u[i] - u[j + 1])];
    const double c = msd[abs(u[i + 1] - u[j + 1])], e = msd[abs(u[i] - u[j])];
    return 0.5 * (a + b - c - e);
}

// covariance of entry j with the missing coordinate of frame t: x_t (ss_order 0) or the increment x_t - x_vb from the last
// valid frame vb before t (ss_order 1)
__device__ __forceinline__ double kal_miss_cov(const GaussKalSet &p, const int32_t *__restrict__ u, int t, int vb, int j)
{
#pragma clang fp contract(off)
    const double *__restrict__ msd = p.msd;
    if (p.order == 0) return 0.5 * (p.msd_inf - msd[abs(t - u[j])]);
    const double a = msd[abs(u[j + 1] - vb)], b = msd[abs(u[j] - t)];
    const double c = msd[abs(u[j + 1] - t)], e = msd[abs(u[j] - vb)];
    return 0.5 * (a + b - c - e);
}

// entry j of the data vector (gauss.hip: gauss_rhs)
__device__ __forceinline__ double kal_rhs(const GaussKalSet &p, int rank, bool centred, int j)
{
#pragma clang fp contract(off)
    const double *__restrict__ xv = p.xv + rank;
    if (p.order == 0) return (j == 0 && !centred) ? xv[0] : xv[j] - p.mean;
    return (xv[j + 1] - xv[j]) - p.mean;
}

__global__ void __launch_bounds__(kThreads) gauss_kal_factor_kernel(const GaussKalSet *__restrict__ sets,
                                                                     const GaussKalJob *__restrict__ jobs,
                                                                     double *__restrict__ scratch, double *__restrict__ rec)
{
#pragma clang fp contract(off)
    __shared__ double diag;
    const GaussKalJob job = jobs[blockIdx.x];
    const GaussKalSet &p = sets[job.set];
    const int n = job.n, nm = job.nmiss, R = n + nm;    // rows: n of C, nm missing frames, the data row R
    const int64_t ld = R + 1;
    double *__restrict__ L = scratch + job.fac;
    double *__restrict__ rc = rec + job.rec;
    const int32_t *__restrict__ u = p.vidx + job.rank;
    const int32_t *__restrict__ mt = p.midx + job.miss;
    const bool centred = job.centred;

    for (int j = 0; j < n; ++j) {
        double *__restrict__ colj = L + j * ld;
        for (int i = j + (int)threadIdx.x; i <= R; i += kThreads) {
            double acc;
            if (i < n) {
                acc = kal_cov(p, u, i, j);
            } else if (i < R) {
                const int q = i - n, t = mt[q];
                const int vb = p.order == 0 ? 0 : p.vidx[t - (job.miss + q) - 1];
                acc = kal_miss_cov(p, u, t, vb, j);
            } else {
                acc = kal_rhs(p, job.rank, centred, j);
            }
            const double *__restrict__ ci = L + i;
            const double *__restrict__ cj = L + j;
            for (int k = 0; k < j; ++k) acc = fma(-ci[k * ld], cj[k * ld], acc);
            if (i == j) diag = sqrt(acc);
            else colj[i] = acc;
        }
        __syncthreads();
        const double djj = diag;
        for (int i = j + 1 + (int)threadIdx.x; i <= R; i += kThreads) {
            const double v = colj[i] / djj;
            colj[i] = v;
            if (i == R) {       // the data row: z_j
                rc[2 * j] = djj;
                rc[2 * j + 1] = v;
            }
        }
        if (threadIdx.x == 0) colj[j] = djj;
        __syncthreads();
    }
    // the missing frames: mean u.z and variance C_tt - u.u of the coordinate given the window
    for (int q = threadIdx.x; q < nm; q += kThreads) {
        double s = 0.0, uu = 0.0;
        for (int j = 0; j < n; ++j) {
            const double w = L[j * ld + n + q];
            s = fma(w, L[j * ld + R], s);
            uu = fma(w, w, uu);
        }
        const int t = mt[q];
        double mean, var;
        if (p.order == 0) {
            mean = s + p.mean;
            var = 0.5 * (p.msd_inf - p.msd[0]) - uu;
        } else {
            const int g = t - (job.miss + q);               // valid frames before t; the last of them is vb
            const int vb = p.vidx[g - 1];
            // prior mean of the increment vb -> t: its share of the mean increment to the next valid frame, or the mean
            // increment per frame behind the window's last valid frame
            const double prior = g - job.rank <= n ? p.mean * (double)(t - vb) / (double)(p.vidx[g] - vb) : p.mean * (double)(t - vb);
            mean = p.xv[g - 1] + (prior + s);
            var = p.msd[t - vb] - uu;
        }
        rc[2 * n + 2 * q] = mean;
        rc[2 * n + 2 * q + 1] = var;
    }
}

__global__ void __launch_bounds__(kThreads) gauss_kal_solve_kernel(const GaussKalSet *__restrict__ sets,
                                                                    const GaussKalJob *__restrict__ jobs, double *__restrict__ rec)
{
#pragma clang fp contract(off)
    extern __shared__ double r[];
    const GaussKalJob job = jobs[blockIdx.x];
    const GaussKalSet &p = sets[job.set];
    const int n = job.n;
    const int64_t ld0 = p.fac_ld;
    const double *__restrict__ L0 = p.fac;
    double *__restrict__ rc = rec + job.rec;
    for (int i = threadIdx.x; i < n; i += kThreads) r[i] = kal_rhs(p, job.rank, job.centred, i);
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double *__restrict__ colj = L0 + j * ld0;
        const double djj = colj[j];
        const double z = r[j] / djj;
        if (threadIdx.x == 0) {
            rc[2 * j] = djj;
            rc[2 * j + 1] = z;
        }
        for (int i = j + 1 + (int)threadIdx.x; i < n; i += kThreads) r[i] = fma(-colj[i], z, r[i]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kScatterThreads) gauss_kal_scatter_kernel(const GaussKalScatter p)
{
#pragma clang fp contract(off)
    const GaussKalRef ref = p.refs[blockIdx.x];
    const GaussKalSet &s = p.sets[ref.set];
    const double *__restrict__ rc = p.rec + (ref.rec >= 0 ? ref.rec : 0);
    const double nan = __builtin_nan("");
    const int order = s.order;
    const int64_t base = (ref.cand - p.c0) * p.Tout * p.d + ref.k;
    for (int t = ref.t0 + (int)threadIdx.x; t < ref.t2; t += kScatterThreads) {
        double term = 0.0, pm = nan, pv = nan, sm = nan, sv = nan, in = nan;
        if (t >= ref.t1 || ref.nan) {
            term = nan;
        } else {
            const int g = s.rank[t];
            if (s.rank[t + 1] > g) {                // valid
                const double x = s.xv[g];
                sm = x;
                sv = 0.0;
                const int j = g - ref.rank - order;     // the entry of frame t: v_j (ss_order 0), v_{j+1} (ss_order 1)
                if (j >= ref.skip && j < ref.n) {
                    const double ljj = rc[2 * j], z = rc[2 * j + 1];
                    term = -(log(ljj) + 0.5 * z * z + kHalfLog2Pi);
                    const double shift = order == 0 ? s.mean : s.xv[g - 1] + s.mean;
                    const double y = order == 0 ? x - s.mean : (x - s.xv[g - 1]) - s.mean;
                    pm = (y - ljj * z) + shift;
                    pv = ljj * ljj;
                    in = z;
                }
            } else if (order == 0 || g > ref.rank) {    // missing, with a row in the job
                const int q = (t - g) - ref.miss;
                sm = rc[2 * ref.n + 2 * q];
                sv = rc[2 * ref.n + 2 * q + 1];
            }
        }
        const int64_t o = base + (int64_t)t * p.d;
        if (p.out[0]) p.out[0][o] = term;
        if (p.out[1]) p.out[1][o] = pm;
        if (p.out[2]) p.out[2][o] = pv;
        if (p.out[5]) p.out[5][o] = sm;
        if (p.out[6]) p.out[6][o] = sv;
        if (p.out[7]) p.out[7][o] = in;
    }
}

} // namespace

int launch_gauss_kal_factor(const GaussKalSet *sets, const GaussKalJob *jobs, int njobs, double *scratch, double *rec, void *stream)
{
    if (njobs <= 0) return 0;
    hipLaunchKernelGGL(gauss_kal_factor_kernel, dim3(njobs), dim3(kThreads), 0, (hipStream_t)stream, sets, jobs, scratch, rec);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_kal_solve(const GaussKalSet *sets, const GaussKalJob *jobs, int njobs, int nmax, double *rec, void *stream)
{
    if (njobs <= 0) return 0;
    if (nmax < 1 || nmax > kGaussMaxT) return 1;
    const size_t lds = (size_t)nmax * sizeof(double);
    hipLaunchKernelGGL(gauss_kal_solve_kernel, dim3(njobs), dim3(kThreads), lds, (hipStream_t)stream, sets, jobs, rec);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_kal_scatter(const GaussKalScatter &p, void *stream)
{
    if (p.nrefs <= 0) return 0;
    hipLaunchKernelGGL(gauss_kal_scatter_kernel, dim3(p.nrefs), dim3(kScatterThreads), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace bild
