// Kernel of the posterior of the number of frames in a set G of states under a dwell-time prior (gauss_dwellocc.h, DESIGN.md
// section 28): plain fp64 vector code on the tables W and F of a GenericGaussianModel trajectory set and on the prior tables of
// the dwell-time recursion (gauss_dwell.h).  Everything is kept in logs, sums are (m, z) pairs of wave.h, no atomics: every
// value has one owner and every sum a fixed order that depends on the trajectory alone.
//
//   * dwell_occupancy_kernel: end frame b of the forward recursion resolved by the number n of frames in G, one launch per end
//       frame: a segment in G that starts at c reads alpha(c, s, n - (b - c)), so b needs every n of every earlier c, and the
//       launch boundary is the only synchronisation between end frames.  A workgroup owns 64 values of n of one trajectory
//       (lane = n; n = 0 .. b, so the second tile opens at b = 64) and takes the states in turn.  The eight waves stride the
//       switch frame c from the first c that can reach the tile (c >= n outside G, c >= b - n inside); omega_s(c, b) and
//       W[s][c - 1][b] are one address for the wave, and a c whose omega is -inf or whose window is NaN adds nothing for the
//       whole wave; the run alpha(c, s, .) is read coalesced.  The loads of four switch frames of a wave are issued together,
//       the terms added in ascending c.  A lane keeps a running (m, z); the waves' pairs meet in LDS and wave 0
//       merges them in wave order.  Wave 0 then holds A(b, ., n) of its n in registers, forms alpha(b, ., n) from it (the
//       jump mix, fused) and writes it; at b = T it writes A(T, ., n) instead.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwellocc.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kWaves = kDwellOccWaves;
constexpr int kAhead = 4;       // switch frames of a wave whose loads are in flight together

template <int S> __global__ void __launch_bounds__(kWaves * 64) dwell_occupancy_kernel(DwellParams p, DwellOccupancy o, int b)
{
    __shared__ double sh_m[kWaves][64], sh_z[kWaves][64];
    const int tiles = b / kDwellTile + 1;       // of the launch: blockIdx.x = trajectory x tile of n = 0 .. b
    const int traj = (int)blockIdx.x / tiles;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld;
    if (T < b) return;          // the whole workgroup
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int n0 = ((int)blockIdx.x % tiles) * kDwellTile, n = n0 + lane;
    double *__restrict__ alpha = o.alpha + (int64_t)traj * o.stride;

    double An[S];
    for (int s = 0; s < S; ++s) {
        const bool in = (o.target >> s & 1u) != 0;
        const double *__restrict__ dw = p.log_dwell + (int64_t)s * p.L, *__restrict__ sv = p.log_surv + (int64_t)s * p.L;
        double m = neg_inf(), z = 0.0;
        if (q == 0 && n == (in ? b : 0)) {      // the first segment: all of its b frames are in G, or none
            const double f = td.F[(int64_t)s * (T + 1) + b];
            if (f == f) lse_add(m, z, p.log_init[s] + (b == T ? sv[T - 1] : dw[b - 1]) + f);
        }
        const double *__restrict__ Ws = td.W + (int64_t)s * td.w_per_state;
        const int c_lo = max(1, in ? b - n0 - (kDwellTile - 1) : n0);       // no earlier c reaches an n of the tile
        const double *__restrict__ omega = b == T ? sv + (T - 1) : dw + (b - 1);     // omega_s(c, b) at omega[-c]
        int c = c_lo + q;
        // four switch frames at a time: their loads do not wait for one another (an entry outside 0 .. c is read at the
        // nearest end of the run and dropped); the terms are added in the order of the plain loop below
        for (; c + (kAhead - 1) * kWaves < b; c += kAhead * kWaves) {
            double om[kAhead], w[kAhead], a[kAhead];
            bool use[kAhead];
#pragma unroll
            for (int k = 0; k < kAhead; ++k) {
                const int ck = c + k * kWaves, from = in ? n - (b - ck) : n;
                om[k] = omega[-ck];
                w[k] = Ws[gauss_wrow(T, ck - 1) + (b - ck)];
                use[k] = from >= 0 && from <= ck;
                a[k] = alpha[((int64_t)ck * S + s) * ld + min(max(from, 0), ck)];
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
            const int from = in ? n - (b - c) : n;
            if (from < 0 || from > c) continue; // alpha(c, ., from) is empty (and n > b has no owner)
            lse_add(m, z, alpha[((int64_t)c * S + s) * ld + from] + om + w);
        }
        sh_m[q][lane] = m;
        sh_z[q][lane] = z;
        __syncthreads();
        if (q == 0) {
            for (int r = 1; r < kWaves; ++r) lse_merge(m, z, sh_m[r][lane], sh_z[r][lane]);
            An[s] = lse_value(m, z);
        }
        __syncthreads();
    }
    if (q != 0 || n > b) return;
    if (b == T) {
        for (int s = 0; s < S; ++s) o.last[((int64_t)traj * ld + n) * S + s] = An[s];
        return;
    }
    for (int s = 0; s < S; ++s) {
        double m = neg_inf(), z = 0.0;
        for (int r = 0; r < S; ++r) lse_add(m, z, An[r] + p.log_jump[r * S + s]);
        alpha[((int64_t)b * S + s) * ld + n] = lse_value(m, z);
    }
}

} // namespace

int launch_dwell_occupancy(const DwellParams &p, const DwellOccupancy &o, int b, void *stream)
{
    if (b < 1 || b > p.Tm || p.n_traj < 1) return 1;
    const dim3 grid((unsigned)(b / kDwellTile + 1) * (unsigned)p.n_traj), block(kWaves * 64);
    switch (p.S) {
    case 2: hipLaunchKernelGGL(dwell_occupancy_kernel<2>, grid, block, 0, (hipStream_t)stream, p, o, b); break;
    case 3: hipLaunchKernelGGL(dwell_occupancy_kernel<3>, grid, block, 0, (hipStream_t)stream, p, o, b); break;
    case 4: hipLaunchKernelGGL(dwell_occupancy_kernel<4>, grid, block, 0, (hipStream_t)stream, p, o, b); break;
    default: return 1;      // one state has no proper subset
    }
    return launched();
}

} // namespace bild
