// Kernels of the evidence gradient (gauss_segsens.h).  Plain fp64 vector code; no atomics, every value
// has one owner and every sum a fixed order.
//
//   * segsens_weight_kernel: Omega(s, a, t) from the tables of the segment recursion.  The terms are those of
//     segdp_cover_kernel -- alpha_j(a, s) exp W[s][a - 1][b] gamma_{k-j}(b, s), scaled by exp(-top_k) so that every
//     exponent is <= 0 -- but the kernel keeps a row's suffix sums instead of collapsing them onto frames.  A wave owns one
//     row a of one (trajectory, s) and walks its tiles of 64 end frames from the right: lane = b - 1 within the tile, so
//     that the row of W is read and the row of Omega written coalesced, and alpha_j(a, s) is the same for the whole wave.
//     A lane adds its terms over k ascending (each k's sum times coef[k]; a k with coef 0 is skipped), then j ascending; a
//     suffix sum across the lanes and the total of the tiles to the right give Omega.  Tiles are aligned to multiples of
//     64 frames, so the order depends on the trajectory alone.
//   * segsens_solve_kernel<P> / segsens_factor_kernel<P>: gauss_sens_solve_kernel / gauss_sens_factor_kernel (gauss_sens.hip)
//     with a weight per counted entry: entry j of a job adds w_j (tau_j, dtau_j, Fisher_j), w_j the sum of Omega(s, a, t_j)
//     over the job's segment starts a (ascending; more than one where window starts on missing frames share the tau row of
//     the next valid one).  An entry of weight 0 adds nothing, so a factor that fails where no profile looks stays harmless.
//     Contraction is off, as in gauss_sens.hip: the sums do not depend on P.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_segsens.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kThreads = 256;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

__device__ __forceinline__ int64_t at(const SegdpParams &p, int traj, int level, int s, int b)
{
    return (int64_t)traj * p.slot + ((int64_t)level * p.S + s) * p.ld + b;
}

__global__ void __launch_bounds__(kThreads) segsens_weight_kernel(SegdpParams p, SegsensWeights w)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, K = p.K;
    const int lane = threadIdx.x & 63;
    const int a = (int)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (a >= T) return;     // the whole wave
    const double *__restrict__ coef = w.coef + (int64_t)traj * K, *__restrict__ top = w.top + (int64_t)traj * K;
    const double *__restrict__ src =
        a == 0 ? td.F + (int64_t)s * (T + 1) : td.W + (int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) - a;    // entry b at src[b]
    double *__restrict__ dst = w.omega + (int64_t)traj * w.om_slot +
                               (a == 0 ? (int64_t)p.S * w.om_tri + (int64_t)s * p.ld - 1 : (int64_t)s * w.om_tri + gauss_wrow(T, a - 1) - a);   // entry t at dst[t + 1]
    double carry = 0.0;
    for (int tile = (T - 1) / kSegdpTile; tile >= a / kSegdpTile; --tile) {
        const int t = tile * kSegdpTile + lane, b = t + 1;
        const bool mine = t < T && t >= a;
        double qv = 0.0;
        const double wv = mine ? src[b] : neg_inf();
        if (mine && wv == wv) {
            for (int k = 0; k < K; ++k) {
                const double ck = coef[k];
                if (!(ck > 0.0)) continue;
                const double tk = top[k];
                double acc = 0.0;
                if (a == 0) {
                    const int64_t g = at(p, traj, k, s, b);
                    const double gz = p.gamma.Z[g];
                    if (gz > 0.0) acc = gz * exp(wv + p.gamma.M[g] - tk);
                } else {
                    const int jmax = min(k, a);
                    for (int j = 1; j <= jmax; ++j) {
                        const int64_t ia = at(p, traj, j, s, a);
                        const double az = p.alpha.Z[ia];
                        if (!(az > 0.0)) continue;
                        const int64_t g = at(p, traj, k - j, s, b);
                        const double gz = p.gamma.Z[g];
                        if (gz > 0.0) acc += az * gz * exp(p.alpha.M[ia] + wv + p.gamma.M[g] - tk);
                    }
                }
                qv += ck * acc;
            }
        }
        qv = wave_scan_down(qv, lane);
        qv += carry;
        if (mine) dst[b] = qv;
        carry = __shfl(qv, 0, 64);
    }
}

// covariance of entries i, j and the data vector: gauss_sens.hip's sens_cov, sens_rhs, sens_drhs
__device__ __forceinline__ double ss_cov(const double *__restrict__ msd, double msd_inf, int order, const int32_t *__restrict__ u, int i,
                                         int j)
{
#pragma clang fp contract(off)
    if (order == 0) return 0.5 * (msd_inf - msd[abs(u[i] - u[j])]);
    const double a = msd[abs(u[i + 1] - u[j])], b = msd[abs(u[i] - u[j + 1])];
    const double c = msd[abs(u[i + 1] - u[j + 1])], e = msd[abs(u[i] - u[j])];
    return 0.5 * (a + b - c - e);
}

__device__ __forceinline__ double ss_rhs(const GaussSensSet &p, int rank, bool centred, int j)
{
#pragma clang fp contract(off)
    const double *__restrict__ xv = p.xv + rank;
    if (p.order == 0) return (j == 0 && !centred) ? xv[0] : xv[j] - p.mean;
    return (xv[j + 1] - xv[j]) - p.mean;
}

__device__ __forceinline__ double ss_drhs(int order, bool centred, int j, double dm)
{
    return (order == 0 && j == 0 && !centred) ? 0.0 : -dm;
}

// the weight of entry j of a job: Omega at the entry's frame, added over the job's segment starts in ascending order
__device__ __forceinline__ double ss_weight(const SegsensJob &job, const double *__restrict__ omega, const int32_t *__restrict__ u, int order,
                                            int j)
{
    const int t = u[order == 0 ? j : j + 1];
    const double *__restrict__ om = omega + job.om;
    if (job.first) return om[t];
    double w = 0.0;
    for (int a = job.a_lo; a <= job.a_hi; ++a) w += om[gauss_wrow(job.T, a - 1) + (t + 1 - a)];
    return w;
}

// one counted entry of weight w into the job's sums: the layout of gauss_sens.hip's sens_entry
template <int P>
__device__ __forceinline__ void ss_entry(double *s, double w, double djj, double z, const double *ddjj, const double *dz)
{
#pragma clang fp contract(off)
    s[0] += w * (log(djj) + 0.5 * z * z + kHalfLog2Pi);
    double a[P > 0 ? P : 1], g[P > 0 ? P : 1];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        a[q] = ddjj[q] / djj;
        g[q] = a[q] * z + dz[q];
        s[1 + q] += w * (a[q] + z * dz[q]);
    }
    int f = 1 + P;
#pragma unroll
    for (int q = 0; q < P; ++q)
#pragma unroll
        for (int r = q; r < P; ++r, ++f) s[f] += w * (2.0 * a[q] * a[r] + g[q] * g[r]);
}

template <int P>
__global__ void __launch_bounds__(kThreads) segsens_factor_kernel(const GaussSensSet *__restrict__ sets, const SegsensJob *__restrict__ jobs,
                                                                   const double *__restrict__ omega, double *__restrict__ base,
                                                                   double *__restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double diag, ddiag[P > 0 ? P : 1];
    __shared__ double sums[kGaussSensStride];
    const SegsensJob sj = jobs[blockIdx.x];
    const GaussSensJob &job = sj.j;
    const GaussSensSet &p = sets[job.set];
    const int n = job.n;
    const int rows = n + 1;                 // with the data row
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
                acc = ss_cov(p.msd, p.msd_inf, order, u, i, j);
#pragma unroll
                for (int q = 0; q < P; ++q) dacc[q] = ss_cov(p.dmsd + q * p.dmsd_ld, p.dmsd_inf[q], order, u, i, j);
            } else {
                acc = ss_rhs(p, job.rank, job.centred, j);
#pragma unroll
                for (int q = 0; q < P; ++q) dacc[q] = ss_drhs(order, job.centred, j, p.dmean[q]);
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
            if (i == n && j >= job.skip) {      // the data row: z_j, dz_j
                const double wj = ss_weight(sj, omega, u, order, j);
                if (wj > 0.0) ss_entry<P>(sums, wj, djj, v, ddjj, dv);
            }
        }
        if (threadIdx.x == 0) {
            colj[j * W] = djj;
#pragma unroll
            for (int q = 0; q < P; ++q) colj[j * W + 1 + q] = ddjj[q];
        }
        __syncthreads();
    }
    if (threadIdx.x < kGaussSensStride) out[(int64_t)job.out * kGaussSensStride + threadIdx.x] = sums[threadIdx.x];
}

template <int P>
__global__ void __launch_bounds__(kThreads) segsens_solve_kernel(const GaussSensSet *__restrict__ sets, const SegsensJob *__restrict__ jobs,
                                                                  int nmax, const double *__restrict__ omega, double *__restrict__ out)
{
#pragma clang fp contract(off)
    extern __shared__ double lds[];     // r, then dr_0 .. dr_{P-1}, then the weights: nmax doubles each
    const SegsensJob sj = jobs[blockIdx.x];
    const GaussSensJob &job = sj.j;
    const GaussSensSet &p = sets[job.set];
    const int n = job.n, order = p.order;
    const int64_t ld0 = p.fac_ld;
    // the shared factor: the layout gauss_sens_solve_kernel reads
    constexpr int W = P > 0 ? 2 : 1;
    const int64_t ms = 2 * ld0 * ld0;
    const double *__restrict__ L0 = p.fac;
    const int32_t *__restrict__ u = p.vidx + job.rank;
    double *__restrict__ r = lds, *__restrict__ wt = lds + (int64_t)(1 + P) * nmax;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        r[i] = ss_rhs(p, job.rank, job.centred, i);
#pragma unroll
        for (int q = 0; q < P; ++q) r[(q + 1) * nmax + i] = ss_drhs(order, job.centred, i, p.dmean[q]);
        wt[i] = i >= job.skip ? ss_weight(sj, omega, u, order, i) : 0.0;
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
        const double wj = wt[j];
        if (wj > 0.0) ss_entry<P>(s, wj, djj, z, ddjj, dz);
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
int launch_factor(const GaussSensSet *sets, const SegsensJob *jobs, int njobs, const double *omega, double *base, double *out, void *stream)
{
    hipLaunchKernelGGL(segsens_factor_kernel<P>, dim3(njobs), dim3(kThreads), 0, (hipStream_t)stream, sets, jobs, omega, base, out);
    return launched();
}

template <int P>
int launch_solve(const GaussSensSet *sets, const SegsensJob *jobs, int njobs, int nmax, const double *omega, double *out, void *stream)
{
    const size_t lds = (size_t)(2 + P) * nmax * sizeof(double);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(segsens_solve_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess)
        return 1;
    hipLaunchKernelGGL(segsens_solve_kernel<P>, dim3(njobs), dim3(kThreads), lds, (hipStream_t)stream, sets, jobs, nmax, omega, out);
    return launched();
}

} // namespace

int launch_segsens_weight(const SegdpParams &p, const SegsensWeights &w, void *stream)
{
    const int waves = kThreads / 64;
    const dim3 grid((unsigned)((p.Tm + waves - 1) / waves), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(segsens_weight_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p, w);
    return launched();
}

int launch_segsens_factor(const GaussSensSet *sets, const SegsensJob *jobs, int njobs, int P, const double *omega, double *base, double *out,
                          void *stream)
{
    if (njobs <= 0) return 0;
    switch (P) {
    case 0: return launch_factor<0>(sets, jobs, njobs, omega, base, out, stream);
    case 1: return launch_factor<1>(sets, jobs, njobs, omega, base, out, stream);
    case 2: return launch_factor<2>(sets, jobs, njobs, omega, base, out, stream);
    case 3: return launch_factor<3>(sets, jobs, njobs, omega, base, out, stream);
    case 4: return launch_factor<4>(sets, jobs, njobs, omega, base, out, stream);
    default: return 1;
    }
}

int launch_segsens_solve(const GaussSensSet *sets, const SegsensJob *jobs, int njobs, int P, int nmax, const double *omega, double *out,
                         void *stream)
{
    if (njobs <= 0) return 0;
    if (nmax < 1 || nmax > kGaussMaxT) return 1;
    switch (P) {
    case 0: return launch_solve<0>(sets, jobs, njobs, nmax, omega, out, stream);
    case 1: return launch_solve<1>(sets, jobs, njobs, nmax, omega, out, stream);
    case 2: return launch_solve<2>(sets, jobs, njobs, nmax, omega, out, stream);
    case 3: return launch_solve<3>(sets, jobs, njobs, nmax, omega, out, stream);
    case 4: return launch_solve<4>(sets, jobs, njobs, nmax, omega, out, stream);
    default: return 1;
    }
}

} // namespace bild
