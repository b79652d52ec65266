// The weight kernel of the evidence gradient under a dwell-time prior (gauss_dwellsens.h).  Plain fp64
// vector code; no atomics, every value has one owner and every sum a fixed order that depends on the trajectory alone.
//
//   * dwellsens_weight_kernel: Omega(s, a, t) from the tables of the dwell-time recursion.  The terms are those of
//     dwell_cover_kernel -- exp(alpha(a, s) + omega + W[s][a - 1][b] + gamma(b, s) - logev), the exponent clamped at 0 -- but
//     the kernel keeps a row's suffix sums instead of collapsing them onto frames: segsens_weight_kernel (gauss_segsens.hip)
//     without its loops over k and j.  A wave owns one row a of one (trajectory, s) and walks its tiles of 64 end frames from
//     the right: lane = b - 1 within the tile, so that the row of W, the run of log_dwell and gamma(., s) are read and the row
//     of Omega written coalesced; alpha(a, s) and logev are the same for the whole wave.  One exp per (a, b, s).  A suffix
//     sum across the lanes and the total of the tiles to the right give Omega.  Tiles are aligned to multiples of 64 frames.
//     S is a run-time value: nothing per state stays in registers across frames.  A row whose start no profile reaches, and
//     every row of a trajectory without a profile of positive weight, is written as zeros: a job may read it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwellsens.h"
#include "wave.h"

namespace bild {
namespace {

__global__ void __launch_bounds__(kDwellThreads) dwellsens_weight_kernel(DwellParams p, DwellsensWeights w)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    const int lane = threadIdx.x & 63;
    const int a = (int)blockIdx.x * (kDwellThreads / 64) + (threadIdx.x >> 6);
    if (a >= T) return;     // the whole wave
    const int64_t base = (int64_t)traj * p.slot + (int64_t)s * p.ld;
    const double logev = p.fin[2 * traj];
    const double head = a == 0 ? p.log_init[s] : p.alpha[base + a];
    const bool live = logev > neg_inf() && head > neg_inf();
    const double *__restrict__ src =
        a == 0 ? td.F + (int64_t)s * (T + 1) : td.W + (int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) - a;    // entry b at src[b]
    const double *__restrict__ gam = p.gamma + base;
    const double *__restrict__ dwell = p.log_dwell + (int64_t)s * p.L - a - 1;      // length b - a at dwell[b]
    const double surv = p.log_surv[(int64_t)s * p.L + (T - a - 1)];
    double *__restrict__ dst = w.omega + (int64_t)traj * w.om_slot +
                               (a == 0 ? (int64_t)p.S * w.om_tri + (int64_t)s * p.ld - 1 : (int64_t)s * w.om_tri + gauss_wrow(T, a - 1) - a);   // entry t at dst[t + 1]
    double carry = 0.0;
    for (int tile = (T - 1) / kDwellTile; tile >= a / kDwellTile; --tile) {
        const int t = tile * kDwellTile + lane, b = t + 1;
        const bool mine = t < T && t >= a;
        double qv = 0.0;
        if (mine && live) {
            const double g = gam[b], om = b == T ? surv : dwell[b], wv = src[b];
            if (g > neg_inf() && om > neg_inf() && wv == wv) qv = exp(fmin(head + om + wv + g - logev, 0.0));
        }
        qv = wave_scan_down(qv, lane);
        qv += carry;
        if (mine) dst[b] = qv;
        carry = __shfl(qv, 0, 64);
    }
}

} // namespace

int launch_dwellsens_weight(const DwellParams &p, const DwellsensWeights &w, void *stream)
{
    const int waves = kDwellThreads / 64;
    const dim3 grid((unsigned)((p.Tm + waves - 1) / waves), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(dwellsens_weight_kernel, grid, dim3(kDwellThreads), 0, (hipStream_t)stream, p, w);
    return launched();
}

} // namespace bild
