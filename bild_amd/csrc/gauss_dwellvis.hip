// Kernel of the posterior of the number of visits to a set G of states under a dwell-time prior (gauss_dwellvis.h, DESIGN.md
// section 30): plain fp64 vector code on the tables W and F of a GenericGaussianModel trajectory set and on the prior tables of
// the dwell-time recursion (gauss_dwell.h).  Everything is kept in logs, sums are (m, z) pairs of wave.h, no atomics: every
// value has one owner and every sum a fixed order that depends on the trajectory alone.
//
//   * dwell_visits_kernel: end frame b of the forward recursion resolved by the number n of visits begun, one launch per end
//       frame, as dwell_occupancy_kernel (gauss_dwellocc.hip): b needs alpha of every earlier c, and the launch boundary is
//       the only synchronisation between end frames.  A segment keeps n, so the sum over c reads alpha(c, s, n) at the lane's
//       own n; the jump mix reads A(b, r, n - 1) for a jump from r outside G into G.  A workgroup therefore owns 63 values of
//       n of one trajectory, lanes 1 .. 63, and lane 0 carries the row below them: it is summed as every other lane is and
//       never written, and the mix takes row n - 1 from the lane below (one shuffle).  The rows at end frame b are n = 0 ..
//       min(n_top, ceil(b / 2) + 1), so the second tile opens at b = 123.  The eight waves stride the switch frame c from the
//       first c that can reach the tile (alpha(c, ., n) exists for c >= 2 n - 3); omega_s(c, b) and W[s][c - 1][b] are one
//       address for the wave, and a c whose omega is -inf or whose window is NaN adds nothing for the whole wave; the run
//       alpha(c, s, .) is read coalesced.  The loads of four switch frames of a wave are issued together, the terms added in
//       ascending c.  A lane keeps a running (m, z); the waves' pairs meet in LDS and wave 0 merges them in wave order.  Wave
//       0 then holds A(b, ., n) of its n in registers, forms alpha(b, ., n) from it (the jump mix, fused) and writes it; at
//       b = T it writes A(T, ., n) instead.  No entry of alpha is read that no launch wrote: row n of switch frame c is read
//       for n <= min(n_top, ceil(c / 2) + 1) alone, which is what end frame c wrote.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwellvis.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kWaves = kDwellVisWaves;
constexpr int kAhead = 4;       // switch frames of a wave whose loads are in flight together

template <int S> __global__ void __launch_bounds__(kWaves * 64) dwell_visits_kernel(DwellParams p, DwellVisits o, int b)
{
    __shared__ double sh_m[kWaves][64], sh_z[kWaves][64];
    const int cap = dwell_visits_cap(b, o.n_top);       // the last row of the launch
    const int tiles = cap / kDwellVisTile + 1;          // blockIdx.x = trajectory x tile of n = 0 .. cap
    const int traj = (int)blockIdx.x / tiles;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ldn = o.ldn;
    if (T < b) return;          // the whole workgroup
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int n0 = ((int)blockIdx.x % tiles) * kDwellVisTile, n = n0 - 1 + lane;    // lane 0: the row below the tile's own
    const bool row = n >= 0 && n <= cap;
    double *__restrict__ alpha = o.alpha + (int64_t)traj * o.stride;

    double An[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool in = (o.target >> s & 1u) != 0;
        const double *__restrict__ dw = p.log_dwell + (int64_t)s * p.L, *__restrict__ sv = p.log_surv + (int64_t)s * p.L;
        double m = neg_inf(), z = 0.0;
        if (q == 0 && row && n == (in ? 1 : 0)) {       // the first segment: the first visit has begun, or none
            const double f = td.F[(int64_t)s * (T + 1) + b];
            if (f == f) lse_add(m, z, p.log_init[s] + (b == T ? sv[T - 1] : dw[b - 1]) + f);
        }
        const double *__restrict__ Ws = td.W + (int64_t)s * td.w_per_state;
        const int c_lo = max(1, 2 * max(n0 - 1, 0) - 3);        // no earlier c wrote a row of the tile
        const double *__restrict__ omega = b == T ? sv + (T - 1) : dw + (b - 1);     // omega_s(c, b) at omega[-c]
        int c = c_lo + q;
        // four switch frames at a time: their loads do not wait for one another (a row that end frame c did not write is
        // read at the nearest written one and dropped); the terms are added in the order of the plain loop below
        for (; c + (kAhead - 1) * kWaves < b; c += kAhead * kWaves) {
            double om[kAhead], w[kAhead], a[kAhead];
            bool use[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
                const int ck = c + k * kWaves, top = dwell_visits_cap(ck, o.n_top);
                om[k] = omega[-ck];
                w[k] = Ws[gauss_wrow(T, ck - 1) + (b - ck)];
                use[k] = row && n <= top;
                a[k] = alpha[((int64_t)ck * S + s) * ldn + min(max(n, 0), top)];
            }
#pragma unroll
            for (int k = 0; k < kAhead; ++k)
                if (use[k] && om[k] > neg_inf() && w[k] == w[k]) lse_add(m, z, a[k] + om[k] + w[k]);
        }
        for (; c < b; c += kWaves) {
            const double om = omega[-c];
            if (!(om > neg_inf())) continue;    // the whole wave
            const double w = Ws[gauss_wrow(T, c - 1) + (b - c)];
            if (w != w) continue;               // the whole wave
            if (!row || n > dwell_visits_cap(c, o.n_top)) continue;     // end frame c wrote no row n
            lse_add(m, z, alpha[((int64_t)c * S + s) * ldn + n] + om + w);
        }
        sh_m[q][lane] = m;
        sh_z[q][lane] = z;
        __syncthreads();
        if (q == 0) {
            for (int r = 1; r < kWaves; ++r) lse_merge(m, z, sh_m[r][lane], sh_z[r][lane]);
            An[s] = lse_value(m, z);            // -inf in a lane without a row
        }
        __syncthreads();
    }
    if (q != 0) return;
    if (b == T) {
        if (row && lane > 0)
            for (int s = 0; s < S; ++s) o.last[((int64_t)traj * ldn + n) * S + s] = An[s];
        return;
    }
    // the jump mix: a jump from outside G into G begins a visit, so it takes row n - 1, which the lane below holds (row 0
    // takes the -inf of the lane without a row below it)
    double below[S];
#pragma unroll
    for (int r = 0; r < S; ++r) below[r] = __shfl_up(An[r], 1, 64);
    if (!row || lane == 0) return;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const bool in = (o.target >> s & 1u) != 0;
        double m = neg_inf(), z = 0.0;
#pragma unroll
        for (int r = 0; r < S; ++r) lse_add(m, z, (in && !(o.target >> r & 1u) ? below[r] : An[r]) + p.log_jump[r * S + s]);
        alpha[((int64_t)b * S + s) * ldn + n] = lse_value(m, z);
    }
}

} // namespace

int launch_dwell_visits(const DwellParams &p, const DwellVisits &o, int b, void *stream)
{
    if (b < 1 || b > p.Tm || p.n_traj < 1 || o.n_top < 0 || o.ldn != o.n_top + 1) return 1;
    const dim3 grid((unsigned)(dwell_visits_cap(b, o.n_top) / kDwellVisTile + 1) * (unsigned)p.n_traj), block(kWaves * 64);
    switch (p.S) {
    case 2: hipLaunchKernelGGL(dwell_visits_kernel<2>, grid, block, 0, (hipStream_t)stream, p, o, b); break;
    case 3: hipLaunchKernelGGL(dwell_visits_kernel<3>, grid, block, 0, (hipStream_t)stream, p, o, b); break;
    case 4: hipLaunchKernelGGL(dwell_visits_kernel<4>, grid, block, 0, (hipStream_t)stream, p, o, b); break;
    default: return 1;      // one state has no proper subset
    }
    return launched();
}

} // namespace bild
