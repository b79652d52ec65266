// GenericGaussianModel (reference bild/models.py:536-728) on gfx950: the interval tables and the walk over them.
//
// A profile's logL is a sum over its intervals, and the term of an interval depends on (window start, window end,
// state) only ("GenericGaussianModel").  Per trajectory, state n and dimension, take a window start a and the
// valid frames u_0 < u_1 < ... from a on.  With the data vector y (ss_order 0: x_{u_0} raw, then x_{u_j} - m; the first
// interval centres x_{u_0} too; ss_order 1: the increments x_{u_{j+1}} - x_{u_j} - m), L = chol(C) and z = L^-1 y,
//   tau_j = log L_jj + z_j^2 / 2 + log(2 pi) / 2,
// and the interval's term over window [a, b) is minus the sum of tau_j over the entries j whose frames lie before b.
// Three kernels build that:
//   * gauss_factor_kernel: one workgroup per window start factors C of that start (entries generated from the MSD table,
//     nothing stored but the factor) with y appended as one more row, so that the forward solve comes out of the same
//     left-looking column sweep: the last row of the factor of [C y; y^T .] is z.  Used for the one shared Toeplitz factor
//     of a (state, dimension) -- then without the extra row -- and for every start that has a missing frame after it.
//   * gauss_solve_kernel: one workgroup per start whose frames are all valid from the start on: those use leading blocks
//     of the shared factor, so only z = L^-1 y is left (right-looking, y in LDS).
//   * gauss_accumulate_kernel: one lane per (state, start) turns a dimension's tau rows into window sums and adds them to
//     the table, dimensions in index order.
// The walk (gauss_walk_kernel) takes one candidate per lane: run-length segments or the sampler's (s, theta) row, cleaned
// into the reference's intervals (runs of equal state), then k + 1 table reads.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "gauss.h"
#include "philox.h"

namespace bild {
namespace {

constexpr int kThreads = 256;
constexpr double kHalfLog2Pi = 0.91893853320467274178;

// covariance of entries i, j of a start's vector (times: the start's valid frames)
__device__ __forceinline__ double gauss_cov(const GaussJobSet &p, const int32_t *__restrict__ u, int i, int j)
{
    const double *__restrict__ msd = p.msd;
    if (p.order == 0) {
        const int lag = abs(u[i] - u[j]);
        return 0.5 * (p.msd_inf - msd[lag]);
    }
    // increments between consecutive valid frames: 1/2 (msd(u_{i+1} - u_j) + msd(u_i - u_{j+1}) - msd(u_{i+1} - u_{j+1}) - msd(u_i - u_j))
    const double a = msd[abs(u[i + 1] - u[j])], b = msd[abs(u[i] - u[j + 1])];
    const double c = msd[abs(u[i + 1] - u[j + 1])], e = msd[abs(u[i] - u[j])];
    return 0.5 * (a + b - c - e);
}

// entry j of a start's data vector (xv: the dimension's valid values, compacted; p: the start's rank among them)
__device__ __forceinline__ double gauss_rhs(const GaussJobSet &p, int rank, bool centred, int j)
{
    const double *__restrict__ xv = p.xv + rank;
    if (p.order == 0) return (j == 0 && !centred) ? xv[0] : xv[j] - p.mean;
    return (xv[j + 1] - xv[j]) - p.mean;
}

// The left-looking column sweep of one job by one workgroup (the likelihood's factorisations and the generator's factors)
__device__ __forceinline__ void gauss_factor_job(const GaussJobSet &p, const GaussJob &job, double *__restrict__ L)
{
    __shared__ double diag;
    const int n = job.n;
    const int rows = job.tau_row >= 0 ? n + 1 : n;      // with the data row, or (the shared factor) without
    const int ld = rows;
    const int32_t *__restrict__ u = p.vidx + job.rank;
    double *__restrict__ tau = job.tau_row >= 0 ? p.tau + (int64_t)job.tau_row * p.tau_ld : nullptr;

    for (int j = 0; j < n; ++j) {
        double *__restrict__ colj = L + (int64_t)j * ld;
        for (int i = j + (int)threadIdx.x; i < rows; i += kThreads) {
            double acc = i < n ? gauss_cov(p, u, i, j) : gauss_rhs(p, job.rank, job.centred, j);
            const double *__restrict__ ck = L + i;
            const double *__restrict__ cj = L + j;
            for (int k = 0; k < j; ++k) acc = fma(-ck[(int64_t)k * ld], cj[(int64_t)k * ld], acc);
            if (i == j) diag = sqrt(acc);
            else colj[i] = acc;
        }
        __syncthreads();
        const double djj = diag;
        for (int i = j + 1 + (int)threadIdx.x; i < rows; i += kThreads) {
            const double v = colj[i] / djj;
            colj[i] = v;
            if (i == n) tau[j] = log(djj) + 0.5 * v * v + kHalfLog2Pi;
        }
        if (threadIdx.x == 0) colj[j] = djj;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads) gauss_factor_kernel(GaussJobSet p, const GaussJob *__restrict__ jobs, double *__restrict__ scratch,
                                                                 int64_t slot_doubles)
{
    const GaussJob job = jobs[blockIdx.x];
    gauss_factor_job(p, job, job.factor_out ? p.factor : scratch + (int64_t)blockIdx.x * slot_doubles);
}

// one job per set, each written to its set's factor (the generator's S x d Toeplitz factors in one launch)
__global__ void __launch_bounds__(kThreads) gauss_factor_sets_kernel(const GaussJobSet *__restrict__ sets, const GaussJob *__restrict__ jobs)
{
    const GaussJobSet p = sets[blockIdx.x];
    const GaussJob job = jobs[blockIdx.x];
    gauss_factor_job(p, job, p.factor);
}

__global__ void __launch_bounds__(kThreads) gauss_solve_kernel(GaussJobSet p, const GaussJob *__restrict__ jobs, int ld0)
{
    __shared__ double r[kGaussMaxT];
    const GaussJob job = jobs[blockIdx.x];
    const int n = job.n;
    const double *__restrict__ L0 = p.factor;
    double *__restrict__ tau = p.tau + (int64_t)job.tau_row * p.tau_ld;
    for (int i = threadIdx.x; i < n; i += kThreads) r[i] = gauss_rhs(p, job.rank, job.centred, i);
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double djj = L0[(int64_t)j * ld0 + j];
        const double z = r[j] / djj;
        if (threadIdx.x == 0) tau[j] = log(djj) + 0.5 * z * z + kHalfLog2Pi;
        const double *__restrict__ colj = L0 + (int64_t)j * ld0;
        for (int i = j + 1 + (int)threadIdx.x; i < n; i += kThreads) r[i] = fma(-colj[i], z, r[i]);
        __syncthreads();
    }
}

// One lane per (state, start a); a == T is the first-interval row F.  Adds this dimension's window sums to the table
// (first dimension: stores them).
__global__ void __launch_bounds__(kThreads) gauss_accumulate_kernel(GaussAccum p)
{
    const int64_t lane = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int T = p.T;
    if (lane >= (int64_t)p.S * (T + 1)) return;
    const int s = (int)(lane / (T + 1));
    const int a = (int)(lane - (int64_t)s * (T + 1));
    const int order = p.order[s];
    const bool first = a == T;
    const int V = p.V;
    const int rank = first ? 0 : p.rank_of[a];
    // the F row of an ss_order-0 state has its own tau row (centred first value); everything else is the start's row
    const double *__restrict__ tau = p.tau + ((int64_t)s * (V + 1) + (first && order == 0 ? V : rank)) * p.tau_ld;
    double *__restrict__ out = first ? p.F + (int64_t)s * (T + 1) : p.W + (int64_t)s * p.w_per_state + gauss_wrow(T, a);
    const int a0 = first ? 0 : a;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double acc = 0.0;
    int cnt = 0;
    for (int b = a0 + 1; b <= T; ++b) {
        while (rank + cnt < V && p.vidx[rank + cnt] < b) {
            if (order == 0) {
                if (first || cnt >= 1) acc += tau[cnt];
            } else if (cnt >= 1) {
                acc += tau[cnt - 1];
            }
            ++cnt;
        }
        // ss_order 0, later interval, no valid frame in the window: the reference raises IndexError; here NaN
        const double v = (order == 0 && !first && cnt == 0) ? nan : -acc;
        double *o = first ? out + b : out + (b - a - 1);
        *o = p.dim == 0 ? v : *o + v;
    }
}

template <bool ST>
__global__ void __launch_bounds__(kThreads) gauss_walk_kernel(GaussWalk p)
{
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= p.n) return;
    const int K1 = p.K1;
    const int tj = p.traj_id ? p.traj_id[r] : 0;
    const GaussTraj td = p.trajs[tj];
    const int T = td.T;
    const int S = p.S;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    double acc = 0.0, cum = 0.0;
    const double Tm1 = (double)(T - 1);
    int t0 = 0, cur = 0, prev_idx = 0;
    bool first = true, ok = true;
    // segment i covers [start_i, start_{i+1}); the next start is read one step ahead
    int start_next = 0, state_next = 0;
    auto read = [&](int i, int &st, int &sv) {
        if constexpr (ST) {
            const int64_t th = p.thetas[r * K1 + i];
            ok = ok && th >= 0 && th < S;
            sv = (int)th;
            if (i == 0) {
                st = 0;
            } else {
                cum = __dadd_rn(cum, p.ss[r * K1 + i - 1]);     // np.cumsum: sequential
                const double pos = __dmul_rn(cum, Tm1);        // one multiplication, not fused with the sum
                const bool in_range = pos >= 0.0 && pos < 2147483646.0;
                const int idx = in_range ? (int)pos + 1 : INT_MAX;   // floor + 1 (truncation for 0 <= pos)
                ok = ok && in_range && idx >= prev_idx;
                prev_idx = idx;
                st = idx;
            }
        } else {
            st = p.seg_start[r * K1 + i];
            sv = p.seg_state[r * K1 + i];
        }
    };
    read(0, start_next, state_next);
    cur = state_next;
    for (int i = 0; i < K1; ++i) {
        const int st = min(start_next, T), sv = state_next;
        int en = T;
        if (i + 1 < K1) {
            read(i + 1, start_next, state_next);
            en = min(start_next, T);
        }
        if (!ok) break;
        if (en <= st || sv == cur) continue;           // empty segment, or a boundary that switches nothing
        // close [t0, st) in state cur
        acc += first ? td.F[(int64_t)cur * (T + 1) + st] : td.W[(int64_t)cur * td.w_per_state + gauss_wrow(T, t0 - 1) + (st - t0)];
        first = false;
        t0 = st;
        cur = sv;
    }
    if (!ok) {
        if (p.status && atomicCAS(p.status, 0, 1) == 0) p.status[1] = (int)(r < INT_MAX ? r : INT_MAX);
        p.out[r] = nan;
        return;
    }
    acc += first ? td.F[(int64_t)cur * (T + 1) + T] : td.W[(int64_t)cur * td.w_per_state + gauss_wrow(T, t0 - 1) + (T - t0)];
    p.out[r] = acc;
}


// ---------------------------------------------------------------- the generator (bild_gauss_simulate, gauss_sim.cpp)
// Per (state, dimension) one lower Cholesky factor L of the Toeplitz covariance of the longest window (gauss_factor_sets_kernel);
// a column (trajectory, interval, dimension) is the product of its leading block with the interval's normals, and a
// sequential pass per trajectory adds the means, the conditioning column and the ss_order-1 prefix sums.  DESIGN.md
// section 12.

// Device mode: the normal of (trajectory i of the call, frame t, dimension k) is one of the Box-Muller pair of the
// Philox-4x32-10 block with key = seed, counter (i, t / 2, k, 1): even t the cosine, odd t the sine.  Written to Z in the
// replay layout (column after column), so that the product reads both modes alike.  One wave per column.
__global__ void __launch_bounds__(64) gauss_sim_normals_kernel(GaussSimProduct p)
{
    const GaussSimCol c = p.cols[blockIdx.x];
    const int f_lo = c.frame0 + c.skip0, f_hi = c.frame0 + c.len;     // frames [f_lo, f_hi)
    for (int q = (f_lo >> 1) + (int)threadIdx.x; 2 * q < f_hi; q += 64) {
        uint32_t r[4];
        philox4x32_10((uint32_t)c.traj, (uint32_t)q, (uint32_t)c.k, 1u, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), r);
        double n0, n1;
        philox_normal_pair(r, &n0, &n1);
        const int t = 2 * q;
        if (t >= f_lo) p.z[c.z + (t - c.frame0)] = n0;
        if (t + 1 >= f_lo && t + 1 < f_hi) p.z[c.z + (t + 1 - c.frame0)] = n1;
    }
}

// One workgroup per task: a tile of kGaussSimTM rows x the block's columns.  Lane (tx, ty): row r0 + tx, columns
// 8 ty .. 8 ty + 7.  The factor tile (j <= row only; zeros above the diagonal, whose memory is never written) and the
// normals tile go through LDS, kGaussSimKC entries of j at a time; every output sums over j in ascending order, so a
// column's values do not depend on its block, its tile or the batch.
constexpr int kGaussSimKC = 32;
constexpr int kGaussSimCPL = kGaussSimTN / (kThreads / kGaussSimTM);     // columns per lane (8)

__global__ void __launch_bounds__(kThreads) gauss_sim_product_kernel(GaussSimProduct p)
{
    __shared__ double Ls[kGaussSimKC][kGaussSimTM];
    __shared__ double Zs[kGaussSimKC][kGaussSimTN];
    __shared__ GaussSimCol cs[kGaussSimTN];
    const GaussSimTask task = p.tasks[blockIdx.x];
    const GaussSimBlock b = p.blocks[task.block];
    const int tid = threadIdx.x, tx = tid % kGaussSimTM, ty = tid / kGaussSimTM;
    const int r0 = task.r0, r = r0 + tx;
    if (tid < b.nc) cs[tid] = p.cols[b.c0 + tid];
    __syncthreads();

    double acc[kGaussSimCPL];
#pragma unroll
    for (int q = 0; q < kGaussSimCPL; ++q) acc[q] = 0.0;
    const int jend = min(r0 + kGaussSimTM, b.nmax);
    const double *__restrict__ L = b.L;
    for (int j0 = 0; j0 < jend; j0 += kGaussSimKC) {
        for (int e = tid; e < kGaussSimKC * kGaussSimTM; e += kThreads) {
            const int jj = e / kGaussSimTM, ii = e % kGaussSimTM, j = j0 + jj, rr = r0 + ii;
            Ls[jj][ii] = (j <= rr && rr < b.nmax) ? L[(int64_t)j * b.ld + rr] : 0.0;
        }
        for (int e = tid; e < kGaussSimKC * kGaussSimTN; e += kThreads) {
            const int jj = e / kGaussSimTN, cc = e % kGaussSimTN, j = j0 + jj;
            double v = 0.0;
            if (cc < b.nc) {
                const GaussSimCol &c = cs[cc];
                if (j >= c.skip0 && j < c.len) v = p.z[c.z + j];
            }
            Zs[jj][cc] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int jj = 0; jj < kGaussSimKC; ++jj) {
            const double a = Ls[jj][tx];
#pragma unroll
            for (int q = 0; q < kGaussSimCPL; ++q) acc[q] = fma(a, Zs[jj][ty * kGaussSimCPL + q], acc[q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kGaussSimCPL; ++q) {
        const int cc = ty * kGaussSimCPL + q;
        if (cc >= b.nc) break;
        const GaussSimCol &c = cs[cc];
        if (r >= c.skip0 && r < c.len) p.out[(c.row + r) * p.d + b.k] = acc[q];
    }
}

// inclusive prefix sum over the workgroup (kThreads lanes); every lane calls it
__device__ __forceinline__ double gauss_block_scan(double v, double *wsum)
{
    const int lane = threadIdx.x % warpSize, w = threadIdx.x / warpSize;
    for (int o = 1; o < warpSize; o *= 2) {
        const double u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    if (lane == warpSize - 1) wsum[w] = v;
    __syncthreads();
    double before = 0.0;
    for (int q = 0; q < w; ++q) before += wsum[q];
    __syncthreads();
    return before + v;
}

// One workgroup per (trajectory, group of kGaussSimDG dimensions), lanes over frames, the intervals in order, kThreads
// frames at a time.  out holds the product y (entry 0 of an ss_order-1 first interval has none); per dimension:
//   ss_order 0, first interval:  x_t = m + y_t
//   ss_order 0, later interval:  x_t = m + y_t + a L[t - t0 + 1, 0],  a = (x_{t0-1} - m) / L[0, 0]
//   ss_order 1:                  x_t = x_{t0-1} + sum_{t0 <= u <= t} (y_u + m)   (first interval: x_0 = 0, the sum from 1)
// The frames of a pass are staged in LDS and written as whole rows of the group, NaN where missing.
__global__ void __launch_bounds__(kThreads) gauss_sim_assemble_kernel(GaussSimAssemble p)
{
    __shared__ double buf[kThreads * kGaussSimDG];
    __shared__ double carry[kGaussSimDG], start[kGaussSimDG], wsum[kThreads / 64];
    const int i = blockIdx.x, d = p.d;
    const int k0 = blockIdx.y * kGaussSimDG, dd = min(kGaussSimDG, d - k0);
    const int tid = threadIdx.x;
    const int64_t row0 = p.frame_off[i];
    double *__restrict__ out = p.out;
    if (tid < kGaussSimDG) carry[tid] = 0.0;
    __syncthreads();
    for (int v = p.iv_off[i]; v < p.iv_off[i + 1]; ++v) {
        const int t0 = p.iv[3 * v], t1 = p.iv[3 * v + 1], s = p.iv[3 * v + 2];
        if (tid < kGaussSimDG) start[tid] = carry[tid];     // x_{t0-1} (0 before the first interval)
        __syncthreads();
        for (int c0 = t0; c0 < t1; c0 += kThreads) {
            const int nf = min(kThreads, t1 - c0), t = c0 + tid;
            const bool in = tid < nf;
            for (int kk = 0; kk < dd; ++kk) {
                const int k = k0 + kk, sk = s * d + k;
                const double m = p.mean[sk];
                const double y = in && !(t == 0 && p.order[sk] == 1) ? out[(row0 + t) * d + k] : 0.0;
                double x;
                if (p.order[sk] == 0) {
                    x = m + y;
                    if (t0 > 0 && in) {
                        const double *__restrict__ L = p.L[sk];
                        x = fma((start[kk] - m) / L[0], L[t - t0 + 1], x);
                    }
                } else {
                    const double base = carry[kk];
                    x = base + gauss_block_scan(in && t > 0 ? y + m : 0.0, wsum);
                }
                if (in) buf[tid * kGaussSimDG + kk] = x;
                if (tid == nf - 1) carry[kk] = x;
                __syncthreads();
            }
            for (int e = tid; e < nf * dd; e += kThreads) {
                const int f = e / dd, kk = e - f * dd;
                const int64_t rr = row0 + c0 + f;
                out[rr * d + k0 + kk] = p.missing[rr] ? __longlong_as_double(0x7ff8000000000000ll) : buf[f * kGaussSimDG + kk];
            }
            __syncthreads();
        }
    }
}

} // namespace

int launch_gauss_factor_sets(const GaussJobSet *d_sets, const GaussJob *d_jobs, int nsets, void *stream)
{
    if (nsets <= 0) return 0;
    hipLaunchKernelGGL(gauss_factor_sets_kernel, dim3(nsets), dim3(kThreads), 0, (hipStream_t)stream, d_sets, d_jobs);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_sim_normals(const GaussSimProduct &p, void *stream)
{
    if (p.ncols <= 0) return 0;
    hipLaunchKernelGGL(gauss_sim_normals_kernel, dim3(p.ncols), dim3(64), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_sim_product(const GaussSimProduct &p, void *stream)
{
    if (p.ntasks <= 0) return 0;
    hipLaunchKernelGGL(gauss_sim_product_kernel, dim3(p.ntasks), dim3(kThreads), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_sim_assemble(const GaussSimAssemble &p, void *stream)
{
    if (p.n <= 0) return 0;
    const dim3 grid((unsigned)p.n, (unsigned)((p.d + kGaussSimDG - 1) / kGaussSimDG));
    hipLaunchKernelGGL(gauss_sim_assemble_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_factor(const GaussJobSet &p, const GaussJob *d_jobs, int njobs, double *scratch, int64_t slot_doubles, void *stream)
{
    if (njobs <= 0) return 0;
    hipLaunchKernelGGL(gauss_factor_kernel, dim3(njobs), dim3(kThreads), 0, (hipStream_t)stream, p, d_jobs, scratch, slot_doubles);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_solve(const GaussJobSet &p, const GaussJob *d_jobs, int njobs, int ld0, void *stream)
{
    if (njobs <= 0) return 0;
    hipLaunchKernelGGL(gauss_solve_kernel, dim3(njobs), dim3(kThreads), 0, (hipStream_t)stream, p, d_jobs, ld0);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_accumulate(const GaussAccum &p, void *stream)
{
    const int64_t lanes = (int64_t)p.S * (p.T + 1);
    hipLaunchKernelGGL(gauss_accumulate_kernel, dim3((unsigned)((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gauss_walk(const GaussWalk &p, bool st, void *stream)
{
    if (p.n <= 0) return 0;
    const dim3 grid((unsigned)((p.n + kThreads - 1) / kThreads));
    if (st) hipLaunchKernelGGL(gauss_walk_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(gauss_walk_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace bild
