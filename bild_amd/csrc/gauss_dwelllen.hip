// The kernels of the expected segment-length counts under a dwell-time prior (gauss_dwelllen.h).  Plain
// fp64 vector code; no atomics and no LDS, every value has one owner and every sum a fixed order that depends on the
// trajectory alone.
//
//   * dwell_length_kernel: D[s][l], the sums of the segment weight Q(a, a + l, s) along the diagonals of the (a, b) triangle.
//     The terms are those of dwellsens_weight_kernel (gauss_dwellsens.hip), one exp per (a, l, s).  A wave owns one tile of 64
//     lengths of one (trajectory, s), lane = l, and one block of kDwellLenBlock start frames a, which it walks in ascending
//     order: at step a the lanes read row a - 1 of W at b = a + l (F for a = 0) and gamma(b, s), both contiguous across the
//     lanes; log_dwell[s][l] sits in a register, alpha(a, s) and logev are the same for the whole wave, and every lane adds
//     into its own accumulator.  No step depends on the one before, so the loads of the next kDwellLenAhead steps are issued
//     before the arithmetic of the current ones.  Tiles and blocks are aligned to multiples of 64 and kDwellLenBlock frames of
//     the trajectory; a block's share goes to `part`.
//   * dwell_length_close_kernel: one wave per tile of 64 lengths adds the blocks' shares in block order, writes
//     C[s][l] = Q(T - l, T, s) from log_surv, and the wave of the first tile sums I[s] = sum_b Q(0, b, s) over the tiles of b
//     in ascending order.
//   S is a run-time value.  A row whose start no profile reaches, and every row of a trajectory without a profile of positive
//   weight, adds zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwelllen.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kDwellLenAhead = 4;   // steps whose loads are in flight while the steps before them are summed

// the weight of one segment; a NaN window, a -inf head or a -inf tail weighs 0
__device__ __forceinline__ double segment_weight(double head, double om, double wv, double g, double logev)
{
    return head > neg_inf() && g > neg_inf() && wv == wv ? exp(fmin(head + om + wv + g - logev, 0.0)) : 0.0;
}

__global__ void __launch_bounds__(kDwellThreads) dwell_length_kernel(DwellParams p, DwellLengths o)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    const int lane = threadIdx.x & 63;
    const int w = (int)blockIdx.x * (kDwellThreads / 64) + (threadIdx.x >> 6);
    const int tile = w / o.nblk, blk = w % o.nblk;
    const int l = tile * kDwellTile + 1 + lane;                 // this lane's length
    const int a0 = blk * kDwellLenBlock;
    const int a1 = min(a0 + kDwellLenBlock, T - (l - lane));    // the tile's shortest length ends inside the trajectory for a < a1
    if (a0 >= a1) return;   // the whole wave
    const int64_t base = (int64_t)traj * p.slot + (int64_t)s * p.ld;
    const double logev = p.fin[2 * traj];
    const double init = p.log_init[s];
    const double dw = l < T ? p.log_dwell[(int64_t)s * p.L + (l - 1)] : neg_inf();
    const bool use = logev > neg_inf() && dw > neg_inf();
    const double *__restrict__ Ws = td.W + (int64_t)s * td.w_per_state + l;    // entry (a - 1, a + l) at Ws[gauss_wrow(T, a - 1)]
    const double *__restrict__ F = td.F + (int64_t)s * (T + 1) + l;
    const double *__restrict__ gam = p.gamma + base + l;                        // gamma(a + l, s) at gam[a]
    const double *__restrict__ al = p.alpha + base;

    double hn[kDwellLenAhead], wn[kDwellLenAhead], gn[kDwellLenAhead];
#pragma unroll
    for (int i = 0; i < kDwellLenAhead; ++i) {
        const int a = a0 + i;
        const bool mine = use && a < a1 && a + l < T;
        hn[i] = a >= a1 ? neg_inf() : a == 0 ? init : al[a];
        wn[i] = mine ? (a == 0 ? F[0] : Ws[gauss_wrow(T, a - 1)]) : 0.0;
        gn[i] = mine ? gam[a] : neg_inf();
    }
    double acc = 0.0;
    for (int ab = a0; ab < a1; ab += kDwellLenAhead) {
        double hc[kDwellLenAhead], wc[kDwellLenAhead], gc[kDwellLenAhead];
#pragma unroll
        for (int i = 0; i < kDwellLenAhead; ++i) {
            hc[i] = hn[i], wc[i] = wn[i], gc[i] = gn[i];
            const int a = ab + kDwellLenAhead + i;      // (>= 1)
            const bool mine = use && a < a1 && a + l < T;
            hn[i] = a >= a1 ? neg_inf() : al[a];
            wn[i] = mine ? Ws[gauss_wrow(T, a - 1)] : 0.0;
            gn[i] = mine ? gam[a] : neg_inf();
        }
#pragma unroll
        for (int i = 0; i < kDwellLenAhead; ++i) acc += segment_weight(hc[i], dw, wc[i], gc[i], logev);
    }
    if (a0 + l < T) o.part[(((int64_t)traj * p.S + s) * o.nblk + blk) * p.Tm + (l - 1)] = acc;
}

__global__ void __launch_bounds__(kDwellThreads) dwell_length_close_kernel(DwellParams p, DwellLengths o)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * (kDwellThreads / 64) + (threadIdx.x >> 6);
    if (tile * kDwellTile >= T) return;     // the whole wave
    const int l = tile * kDwellTile + 1 + lane;
    const int64_t base = (int64_t)traj * p.slot + (int64_t)s * p.ld;
    const double logev = p.fin[2 * traj];
    const bool live = logev > neg_inf();
    const double init = p.log_init[s];
    const double *__restrict__ F = td.F + (int64_t)s * (T + 1);
    const double *__restrict__ gam = p.gamma + base;
    if (l <= T) {
        const double *__restrict__ part = o.part + ((int64_t)traj * p.S + s) * o.nblk * p.Tm + (l - 1);
        double d = 0.0;
        for (int blk = 0; blk * kDwellLenBlock + l < T; ++blk) d += part[(int64_t)blk * p.Tm];
        o.dwell[base + l - 1] = d;
        // the last segment [a, T), a = T - l
        const int a = T - l;
        double c = 0.0;
        if (live) {
            const double head = a == 0 ? init : p.alpha[base + a];
            const double wv = a == 0 ? F[T] : td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) + l];
            c = segment_weight(head, p.log_surv[(int64_t)s * p.L + (l - 1)], wv, gam[T], logev);
        }
        o.cens[base + l - 1] = c;
    }
    if (tile != 0) return;
    // the first segment [0, b): tiles of b in ascending order, lane = b - 1 within the tile
    double acc = 0.0;
    if (live && init > neg_inf())
        for (int b0 = 0; b0 < T; b0 += kDwellTile) {
            const int b = b0 + 1 + lane;
            if (b > T) continue;
            const double om = b == T ? p.log_surv[(int64_t)s * p.L + (T - 1)] : p.log_dwell[(int64_t)s * p.L + (b - 1)];
            if (om > neg_inf()) acc += segment_weight(init, om, F[b], gam[b], logev);
        }
    acc = wave_sum(acc);
    if (lane == 0) o.init[(int64_t)traj * p.S + s] = acc;
}

} // namespace

int launch_dwell_lengths(const DwellParams &p, const DwellLengths &o, void *stream)
{
    const int waves = kDwellThreads / 64;
    const dim3 grid((unsigned)((p.ntile * o.nblk + waves - 1) / waves), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(dwell_length_kernel, grid, dim3(kDwellThreads), 0, (hipStream_t)stream, p, o);
    if (launched()) return 1;
    const dim3 grid2((unsigned)((p.ntile + waves - 1) / waves), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(dwell_length_close_kernel, grid2, dim3(kDwellThreads), 0, (hipStream_t)stream, p, o);
    return launched();
}

} // namespace bild
