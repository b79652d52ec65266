// Forward sensitivities of GenericGaussianModel's log-likelihood (bild_gauss_logl_sensitivities: gauss_sens.cpp).
//
// A job is one window of one (trajectory, dimension, state): with the data vector y (gauss.hip), L L^T = C, z = L^-1 y,
// the window's term is minus the sum over the counted entries j (skip <= j < n) of tau_j = log L_jj + z_j^2 / 2 +
// log(2 pi) / 2.  Every parameter p carries a tangent dC_p = covariance(dmsd_p, dmsd_inf_p) and dy_p (-dm_p for a centred
// entry, 0 for the raw conditioning value) through the same factorisation, in forward mode:
//     dacc_ij = dC_ij - sum_k (dL_ik L_jk + L_ik dL_jk),  dL_jj = dacc_jj / (2 L_jj),  dL_ij = (dacc_ij - L_ij dL_jj) / L_jj
//     dz = L^-1 (dy - dL z),  dtau_j = dL_jj / L_jj + z_j dz_j
//     Fisher_pq += dS_p dS_q / (2 S^2) + de_p de_q / S   (S = L_jj^2, e = L_jj z_j)  =  2 a_p a_q + g_p g_q,
//     a_p = dL_jj,p / L_jj,  g_p = a_p z_j + dz_j,p
// Two kernels:
//   * gauss_sens_factor_kernel<P>: the left-looking column sweep of gauss_factor_job with P tangent matrices interleaved
//     with L (the job's scratch slot: element by element, so that a lane reads 1 + P consecutive doubles).  Jobs with a
//     data row are windows with a missing frame (z, dz come out of the sweep as the last row); jobs without one build the shared Toeplitz factor of a (state, dimension) and one tangent of it --
//     one workgroup per (state, dimension, parameter), each recomputing L, so that the P tangents run side by side.
//   * gauss_sens_solve_kernel<P>: windows whose frames are all valid, against leading blocks of the shared factor and
//     its tangents: r = y and the P vectors dr_p = dy_p in LDS ((1 + P) n doubles, dynamic), right-looking.
// The entries of a job are added in order by one lane (factor) or by every lane alike (solve), so a job's sums depend on
// the job alone.  Contraction is off in this file: the base quantities (L, z, tau) take the same instructions in every
// instantiation, which makes logl bit-identical whatever P.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss.h"

namespace bild {
namespace {

constexpr int kThreads = 256;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// covariance of entries i, j of a vector whose times are u (gauss.hip: gauss_cov), from the MSD table msd
__device__ __forceinline__ double sens_cov(const double *__restrict__ msd, double msd_inf, int order, const int32_t *__restrict__ u,
                                           int i, int j)
{
#pragma clang fp contract(off)
    if (order == 0) return 0.5 * (msd_inf - msd[abs(u[i] - u[j])]);
    const double a = msd[abs(u[i + 1] - u[j])], b = msd[abs(u[i] - u[j + 1])];
    const double c = msd[abs(u[i + 1] - u[j + 1])], e = msd[abs(u[i] - u[j])];
    return 0.5 * (a + b - c - e);
}

// entry j of the data vector (gauss.hip: gauss_rhs) and its tangent with respect to the mean (dm = dmean_p)
__device__ __forceinline__ double sens_rhs(const GaussSensSet &p, int rank, bool centred, int j)
{
#pragma clang fp contract(off)
    const double *__restrict__ xv = p.xv + rank;
    if (p.order == 0) return (j == 0 && !centred) ? xv[0] : xv[j] - p.mean;
    return (xv[j + 1] - xv[j]) - p.mean;
}

__device__ __forceinline__ double sens_drhs(int order, bool centred, int j, double dm)
{
    return (order == 0 && j == 0 && !centred) ? 0.0 : -dm;
}

// one counted entry into the job's sums: s[0] += tau, s[1 + p] += dtau_p, s[1 + P + f] += Fisher (upper triangle, row-major)
template <int P>
__device__ __forceinline__ void sens_entry(double *s, double djj, double z, const double *ddjj, const double *dz)
{
#pragma clang fp contract(off)
    s[0] += log(djj) + 0.5 * z * z + kHalfLog2Pi;
    double a[P > 0 ? P : 1], g[P > 0 ? P : 1];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        a[q] = ddjj[q] / djj;
        g[q] = a[q] * z + dz[q];
        s[1 + q] += a[q] + z * dz[q];
    }
    int f = 1 + P;
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int r = q; r < P; ++r, ++f) s[f] += 2.0 * a[q] * a[r] + g[q] * g[r];
}

template <int P>
__global__ void __launch_bounds__(kThreads) gauss_sens_factor_kernel(const GaussSensSet *__restrict__ sets,
                                                                      const GaussSensJob *__restrict__ jobs, double *__restrict__ base,
                                                                      double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double diag, ddiag[P > 0 ? P : 1];
    __shared__ double sums[kGaussSensStride];
    const GaussSensJob job = jobs[blockIdx.x];
    const GaussSensSet &p = sets[job.set];
    const int n = job.n;
    const bool data = job.out >= 0;
    const int rows = data ? n + 1 : n;      // with the data row, or (a shared factor) without
    constexpr int W = 1 + P;                // element (i, k) of L at L[(k ld + i) W], of dL_q at L[(k ld + i) W + 1 + q]
    const int64_t ld = rows;
    double *__restrict__ L = base + job.fac;
    const int32_t *__restrict__ u = p.vidx + job.rank;
    const int order = p.order;
    if (threadIdx.x < kGaussSensStride) sums[threadIdx.x] = 0.0;

    for (int j = 0; j < n; ++j) {
        double *__restrict__ colj = L + j * ld * W;
        for (int i = j + (int)threadIdx.x; i < rows; i += kThreads) {
            double acc, dacc[P > 0 ? P : 1];
            if (i < n) {
                acc = sens_cov(p.msd, p.msd_inf, order, u, i, j);
#pragma unroll
                for (int q = 0; q < P; ++q) dacc[q] = sens_cov(p.dmsd + q * p.dmsd_ld, p.dmsd_inf[q], order, u, i, j);
            } else {
                acc = sens_rhs(p, job.rank, job.centred, j);
#pragma unroll
                for (int q = 0; q < P; ++q) dacc[q] = sens_drhs(order, job.centred, j, p.dmean[q]);
            }
            const double *__restrict__ ck = L + (int64_t)i * W;
            const double *__restrict__ cj = L + (int64_t)j * W;
            for (int k = 0; k < j; ++k, ck += ld * W, cj += ld * W) {
                const double lik = ck[0], ljk = cj[0];
                acc = fma(-lik, ljk, acc);
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    dacc[q] = fma(-ck[1 + q], ljk, dacc[q]);
                    dacc[q] = fma(-lik, cj[1 + q], dacc[q]);
                }
            }
            if (i == j) {
                const double dj = sqrt(acc);
                diag = dj;
#pragma unroll
                for (int q = 0; q < P; ++q) ddiag[q] = dacc[q] / (2.0 * dj);
            } else {
                colj[i * W] = acc;
#pragma unroll
                for (int q = 0; q < P; ++q) colj[i * W + 1 + q] = dacc[q];
            }
        }
        __syncthreads();
        const double djj = diag;
        double ddjj[P > 0 ? P : 1];
#pragma unroll
        for (int q = 0; q < P; ++q) ddjj[q] = ddiag[q];
        for (int i = j + 1 + (int)threadIdx.x; i < rows; i += kThreads) {
            const double v = colj[i * W] / djj;
            colj[i * W] = v;
            double dv[P > 0 ? P : 1];
#pragma unroll
            for (int q = 0; q < P; ++q) {
                dv[q] = (colj[i * W + 1 + q] - v * ddjj[q]) / djj;
                colj[i * W + 1 + q] = dv[q];
            }
            if (i == n && j >= job.skip) sens_entry<P>(sums, djj, v, ddjj, dv);     // the data row: z_j, dz_j
        }
        if (threadIdx.x == 0) {
            colj[j * W] = djj;
#pragma unroll
            for (int q = 0; q < P; ++q) colj[j * W + 1 + q] = ddjj[q];
        }
        __syncthreads();
    }
    if (data && threadIdx.x < kGaussSensStride) out[(int64_t)job.out * kGaussSensStride + threadIdx.x] = sums[threadIdx.x];
}

template <int P>
__global__ void __launch_bounds__(kThreads) gauss_sens_solve_kernel(const GaussSensSet *__restrict__ sets,
                                                                     const GaussSensJob *__restrict__ jobs, int nmax,
                                                                     double *__restrict__ out)
{
#pragma clang fp contract(off)
    extern __shared__ double lds[];     // r, then dr_0 .. dr_{P-1}: nmax doubles each
    const GaussSensJob job = jobs[blockIdx.x];
    const GaussSensSet &p = sets[job.set];
    const int n = job.n, order = p.order;
    const int64_t ld0 = p.fac_ld;
    // the shared factor: P = 0 plain; else P pairs (written by the workgroups of the parameters), pair q interleaving a copy
    // of L with dL_q (element e = j ld0 + i at 2 e and 2 e + 1), 2 ld0^2 doubles each
    constexpr int W = P > 0 ? 2 : 1;
    const int64_t ms = 2 * ld0 * ld0;
    const double *__restrict__ L0 = p.fac;
    double *__restrict__ r = lds;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        r[i] = sens_rhs(p, job.rank, job.centred, i);
#pragma unroll
        for (int q = 0; q < P; ++q) r[(q + 1) * nmax + i] = sens_drhs(order, job.centred, i, p.dmean[q]);
    }
    double s[kGaussSensStride];
#pragma unroll
    for (int e = 0; e < kGaussSensStride; ++e) s[e] = 0.0;
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double *__restrict__ colj = L0 + j * ld0 * W;
        const double djj = colj[j * W];
        const double z = r[j] / djj;
        double ddjj[P > 0 ? P : 1], dz[P > 0 ? P : 1];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            ddjj[q] = colj[q * ms + j * W + 1];
            dz[q] = (r[(q + 1) * nmax + j] - ddjj[q] * z) / djj;
        }
        if (j >= job.skip) sens_entry<P>(s, djj, z, ddjj, dz);
        for (int i = j + 1 + (int)threadIdx.x; i < n; i += kThreads) {
            const double l = colj[i * W];
            r[i] = fma(-l, z, r[i]);
#pragma unroll
            for (int q = 0; q < P; ++q) {
                double w = fma(-colj[q * ms + i * W + 1], z, r[(q + 1) * nmax + i]);
                r[(q + 1) * nmax + i] = fma(-l, dz[q], w);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int e = 0; e < kGaussSensStride; ++e) out[(int64_t)job.out * kGaussSensStride + e] = s[e];
}

template <int P>
int launch_factor(const GaussSensSet *sets, const GaussSensJob *jobs, int njobs, double *base, double *out, void *stream)
{
    hipLaunchKernelGGL(gauss_sens_factor_kernel<P>, dim3(njobs), dim3(kThreads), 0, (hipStream_t)stream, sets, jobs, base, out);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <int P>
int launch_solve(const GaussSensSet *sets, const GaussSensJob *jobs, int njobs, int nmax, double *out, void *stream)
{
    const size_t lds = (size_t)(1 + P) * nmax * sizeof(double);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(gauss_sens_solve_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return 1;
    hipLaunchKernelGGL(gauss_sens_solve_kernel<P>, dim3(njobs), dim3(kThreads), lds, (hipStream_t)stream, sets, jobs, nmax, out);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace

int launch_gauss_sens_factor(const GaussSensSet *sets, const GaussSensJob *jobs, int njobs, int P, double *base, double *out, void *stream)
{
    if (njobs <= 0) return 0;
    switch (P) {
    case 0: return launch_factor<0>(sets, jobs, njobs, base, out, stream);
    case 1: return launch_factor<1>(sets, jobs, njobs, base, out, stream);
    case 2: return launch_factor<2>(sets, jobs, njobs, base, out, stream);
    case 3: return launch_factor<3>(sets, jobs, njobs, base, out, stream);
    case 4: return launch_factor<4>(sets, jobs, njobs, base, out, stream);
    default: return 1;
    }
}

int launch_gauss_sens_solve(const GaussSensSet *sets, const GaussSensJob *jobs, int njobs, int P, int nmax, double *out, void *stream)
{
    if (njobs <= 0) return 0;
    if (nmax < 1 || nmax > kGaussMaxT) return 1;
    switch (P) {
    case 0: return launch_solve<0>(sets, jobs, njobs, nmax, out, stream);
    case 1: return launch_solve<1>(sets, jobs, njobs, nmax, out, stream);
    case 2: return launch_solve<2>(sets, jobs, njobs, nmax, out, stream);
    case 3: return launch_solve<3>(sets, jobs, njobs, nmax, out, stream);
    case 4: return launch_solve<4>(sets, jobs, njobs, nmax, out, stream);
    default: return 1;
    }
}

} // namespace bild
