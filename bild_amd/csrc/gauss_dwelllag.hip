// The kernels of exact fixed-lag smoothing under a dwell-time prior (gauss_dwelllag.h).  Plain fp64 vector
// code; no atomics, every value has one owner and every sum a fixed order that depends on the trajectory and on `lag` alone.
//
//   * dwell_lag_base_kernel: Hbase and Kbase, the starts a <= b - 1 - lag of every end frame b.  As dwell_filter_kernel: one
//     workgroup of kDwellWaves waves per (trajectory, tile of 64 ends b), lane = b, the states walked inside the workgroup, the
//     waves taking the starts a = 1 + q, 1 + q + 8, .. (wave 0 the first segment as well); row a - 1 of W and the runs of
//     log_dwell and log_surv are read coalesced across the lanes, alpha(a, s) and alphaArg are the same for the whole wave, and
//     the loads of kDwellLagAhead starts are issued before their arithmetic.  One head + w feeds both sums.  The waves' pairs meet
//     in LDS and wave 0 merges them in wave order.  alpha is complete behind the forward pass, so no term waits for another.
//   * dwell_lag_window_kernel<S>: one wave per (trajectory, cut u), lane = b - lo - 1 for the ends b = lo + 1 .. u of the window,
//     lo = max(u - 1 - lag, 0): at most lag + 1 <= 64 lanes.
//       the chain, a = u - 1 down to lo + 1, as part 2 of dwell_backward_kernel: lane b keeps gamma_u(b, .) in registers, one
//       butterfly (max, then sum) per state and step gives beta_u(a, .), from which lane a takes its gamma_u(a, .).  Row a - 1 of
//       W is contiguous across the lanes; the entries of step a - 1 are loaded before the arithmetic of step a.
//       the frames, a ascending from max(lo + 1 - lag, 0) (lag 0: from lo): lane b keeps H(t, b, .) (lane u: K(t, u, .)) as (m, z), started from
//       its base, and adds the start a where b - lag <= a < b.  From a = lo on, a is a frame t of the window: the lanes b > t give
//       (m + gamma_u(b, s), z), one butterfly (max, then sum) makes J_u(t, s), and lane t - lo keeps it.  The loads of start
//       a + 1 are issued before the arithmetic of start a.
//       E(u) comes from lane u - 1 - lo, and lane t - lo writes J_u(t, .) - E(u) at column u - 1 - t; the wave of cut T fills
//       the columns behind it as well.
//     The states of a chain step depend on one another through log_jump, so the kernel is instantiated per S like the forward
//     and backward passes, with gamma, the sums and log_jump in registers; S is a run-time value of the call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwelllag.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kWaves = kDwellWaves;
constexpr int kDwellLagAhead = 2;   // starts of one wave whose loads are in flight together

__global__ void __launch_bounds__(kWaves * 64) dwell_lag_base_kernel(DwellParams p, DwellLag o)
{
    __shared__ double sh_m[2][kWaves][64], sh_z[2][kWaves][64];
    const int traj = blockIdx.x, b0 = (int)blockIdx.y * kDwellTile;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld, S = p.S, lag = o.lag;
    if (b0 >= T) return;    // the whole workgroup
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int b = b0 + 1 + lane;
    const bool mine = b <= T;
    const int a_end = min(b0 + kDwellTile, T) - lag;    // the starts a < a_end are left of the window of an end of the tile
    const int64_t base = (int64_t)traj * p.slot;
    const double *__restrict__ al = p.alpha + base;
    const int32_t *__restrict__ alArg = p.alphaArg + base;

    for (int s = 0; s < S; ++s) {
        const double *__restrict__ Ws = td.W + (int64_t)s * td.w_per_state;
        const double *__restrict__ surv = p.log_surv + (int64_t)s * p.L;
        const double *__restrict__ dwell = p.log_dwell + (int64_t)s * p.L;
        double md = neg_inf(), zd = 0.0, ms = neg_inf(), zs = 0.0;
        // the first segment [0, b)
        if (q == 0 && mine && b - 1 - lag >= 0 && p.log_init[s] > neg_inf()) {
            const double f = td.F[(int64_t)s * (T + 1) + b];
            if (f == f) {
                lse_add(md, zd, p.log_init[s] + f + dwell[b - 1]);
                lse_add(ms, zs, p.log_init[s] + f + surv[b - 1]);
            }
        }
        // the starts a = 1 .. b - 1 - lag
        for (int a0 = 1 + q; a0 < a_end; a0 += kDwellLagAhead * kWaves) {
            double hv[kDwellLagAhead], dv[kDwellLagAhead], sv[kDwellLagAhead], wv[kDwellLagAhead];
#pragma unroll
            for (int i = 0; i < kDwellLagAhead; ++i) {
                const int a = a0 + i * kWaves;
                const bool use = a < a_end && mine && a <= b - 1 - lag && alArg[s * ld + a] >= 0;
                hv[i] = use ? al[s * ld + a] : neg_inf();
                dv[i] = use ? dwell[b - a - 1] : neg_inf();
                sv[i] = use ? surv[b - a - 1] : neg_inf();
                wv[i] = use ? Ws[gauss_wrow(T, a - 1) + (b - a)] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < kDwellLagAhead; ++i) {
                if (wv[i] != wv[i]) continue;   // a NaN window enters no sum
                const double c = hv[i] + wv[i];
                lse_add(md, zd, c + dv[i]);
                lse_add(ms, zs, c + sv[i]);
            }
        }
        sh_m[0][q][lane] = md, sh_z[0][q][lane] = zd;
        sh_m[1][q][lane] = ms, sh_z[1][q][lane] = zs;
        __syncthreads();
        if (q < 2) {    // wave 0 merges the log_dwell sums, wave 1 the log_surv sums, both in wave order
            double top = neg_inf();
            for (int w = 0; w < kWaves; ++w)
                if (sh_z[q][w][lane] > 0.0) top = fmax(top, sh_m[q][w][lane]);
            double z = 0.0;
            for (int w = 0; w < kWaves; ++w) {
                const double wz = sh_z[q][w][lane];
                if (wz > 0.0) z += wz * exp(sh_m[q][w][lane] - top);
            }
            if (mine) (q == 0 ? o.Hbase : o.Kbase)[base + (int64_t)s * ld + b] = lse_value(top, z);
        }
        __syncthreads();
    }
}

// log prior weight of a segment [a, b) in state s under the cut u: the segment that ends at u is censored
__device__ __forceinline__ double omega_cut(const DwellParams &p, int s, int a, int b, int u)
{
    return b == u ? p.log_surv[(int64_t)s * p.L + (u - a - 1)] : p.log_dwell[(int64_t)s * p.L + (b - a - 1)];
}

template <int S> __global__ void __launch_bounds__(kDwellLagCuts * 64) dwell_lag_window_kernel(DwellParams p, DwellLag o)
{
    const int traj = blockIdx.x, lane = threadIdx.x & 63;
    const int u = (int)blockIdx.y * kDwellLagCuts + (threadIdx.x >> 6) + 1;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld, lag = o.lag;
    if (u > T) return;      // the whole wave
    const int lo = max(u - 1 - lag, 0), n = u - lo;     // n <= lag + 1 <= 64 ends and as many frames
    const int b = lo + 1 + lane;
    const bool mine = lane < n;
    const int64_t base = (int64_t)traj * p.slot;
    const double *__restrict__ al = p.alpha + base;
    const int32_t *__restrict__ alArg = p.alphaArg + base;
    double jm[S][S];
    for (int r = 0; r < S; ++r)
        for (int s = 0; s < S; ++s) jm[r][s] = p.log_jump[r * S + s];

    // the chain: gamma_u(b, .) of the window's ends
    double g[S];
    for (int s = 0; s < S; ++s) g[s] = b == u ? 0.0 : neg_inf();
    {
        double wn[S], on[S];
        for (int s = 0; s < S; ++s) {
            const int a = u - 1;
            const bool use = mine && b > a && a > lo;
            wn[s] = use ? td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) + (b - a)] : 0.0;
            on[s] = use ? omega_cut(p, s, a, b, u) : neg_inf();
        }
        for (int a = u - 1; a > lo; --a) {
            double bc[S];
            for (int s = 0; s < S; ++s) {
                const double wc = wn[s], oc = on[s];
                const bool use = mine && b > a - 1 && a - 1 > lo;
                wn[s] = use ? td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, a - 2) + (b - a + 1)] : 0.0;
                on[s] = use ? omega_cut(p, s, a - 1, b, u) : neg_inf();
                double t = neg_inf();
                if (mine && b > a && g[s] > neg_inf() && oc > neg_inf() && wc == wc) t = oc + wc + g[s];
                const double m = wave_max(t);
                const double z = wave_sum(t > neg_inf() ? exp(t - m) : 0.0);
                bc[s] = lse_value(m, z);
            }
            for (int s = 0; s < S; ++s) {
                double top = neg_inf(), zz = 0.0;
                for (int r = 0; r < S; ++r) top = fmax(top, jm[s][r] + bc[r]);
                if (top > neg_inf())
                    for (int r = 0; r < S; ++r) {
                        const double t = jm[s][r] + bc[r];
                        if (t > neg_inf()) zz += exp(t - top);
                    }
                if (b == a) g[s] = lse_value(top, zz);
            }
        }
    }

    // the frames: H(t, b, .) of lane b (K(t, u, .) of lane u) grows with the starts a, and every a >= lo is a frame t
    double m[S], z[S], J[S];
    for (int s = 0; s < S; ++s) {
        const double bv = mine ? (b == u ? o.Kbase : o.Hbase)[base + (int64_t)s * ld + b] : neg_inf();
        m[s] = bv, z[s] = bv > neg_inf() ? 1.0 : 0.0, J[s] = neg_inf();
    }
    const int a_first = max(min(lo + 1 - lag, lo), 0);      // (lag 0: no start inside the window, the one frame t = lo)
    double hn[S], wn[S], on[S];
    auto fetch = [&](int a) {
        const bool use = a < u && mine && a < b && a >= b - lag;
        for (int s = 0; s < S; ++s) {
            if (a == 0) {
                hn[s] = p.log_init[s];
                wn[s] = use ? td.F[(int64_t)s * (T + 1) + b] : 0.0;
            } else {
                hn[s] = a < u && alArg[s * ld + a] >= 0 ? al[s * ld + a] : neg_inf();
                wn[s] = use ? td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) + (b - a)] : 0.0;
            }
            on[s] = use ? omega_cut(p, s, a, b, u) : neg_inf();
        }
    };
    fetch(a_first);
    for (int a = a_first; a < u; ++a) {
        double hc[S], wc[S], oc[S];
        for (int s = 0; s < S; ++s) hc[s] = hn[s], wc[s] = wn[s], oc[s] = on[s];
        fetch(a + 1);
        for (int s = 0; s < S; ++s)
            if (wc[s] == wc[s]) lse_add(m[s], z[s], hc[s] + oc[s] + wc[s]);     // (oc is -inf outside the lane's starts)
        if (a < lo) continue;   // the whole wave
        for (int s = 0; s < S; ++s) {
            const double v = mine && b > a && z[s] > 0.0 && g[s] > neg_inf() ? m[s] + g[s] : neg_inf();
            const double top = wave_max(v);
            const double sum = wave_sum(v > neg_inf() ? z[s] * exp(v - top) : 0.0);
            if (lane == a - lo) J[s] = lse_value(top, sum);
        }
    }

    // E(u) from the last frame of the cut; lane t - lo writes frame t
    double top = neg_inf(), zz = 0.0, last[S];
    for (int s = 0; s < S; ++s) {
        last[s] = __shfl(J[s], n - 1, 64);
        top = fmax(top, last[s]);
    }
    if (top > neg_inf())
        for (int s = 0; s < S; ++s)
            if (last[s] > neg_inf()) zz += exp(last[s] - top);
    const double E = lse_value(top, zz);
    if (!mine) return;
    const int t = lo + lane, l0 = u - 1 - t, l1 = u == T ? lag : l0;    // cut T is every later column's as well
    for (int s = 0; s < S; ++s) {
        const double v = E > neg_inf() ? J[s] - E : quiet_nan();
        double *__restrict__ row = o.lagged + (((int64_t)traj * S + s) * p.Tm + t) * (lag + 1);
        for (int l = l0; l <= l1; ++l) row[l] = v;
    }
}

} // namespace

int launch_dwell_lag_bases(const DwellParams &p, const DwellLag &o, void *stream)
{
    const dim3 grid((unsigned)p.n_traj, (unsigned)p.ntile);
    hipLaunchKernelGGL(dwell_lag_base_kernel, grid, dim3(kWaves * 64), 0, (hipStream_t)stream, p, o);
    return launched();
}

int launch_dwell_lag_windows(const DwellParams &p, const DwellLag &o, void *stream)
{
    if (o.lag < 0 || o.lag > kDwellLagMax) return 1;    // a window is one wavefront
    const dim3 grid((unsigned)p.n_traj, (unsigned)((p.Tm + kDwellLagCuts - 1) / kDwellLagCuts)), block(kDwellLagCuts * 64);
    switch (p.S) {
    case 1: hipLaunchKernelGGL(dwell_lag_window_kernel<1>, grid, block, 0, (hipStream_t)stream, p, o); break;
    case 2: hipLaunchKernelGGL(dwell_lag_window_kernel<2>, grid, block, 0, (hipStream_t)stream, p, o); break;
    case 3: hipLaunchKernelGGL(dwell_lag_window_kernel<3>, grid, block, 0, (hipStream_t)stream, p, o); break;
    case 4: hipLaunchKernelGGL(dwell_lag_window_kernel<4>, grid, block, 0, (hipStream_t)stream, p, o); break;
    default: return 1;
    }
    return launched();
}

} // namespace bild
