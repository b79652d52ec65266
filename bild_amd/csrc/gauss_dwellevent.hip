// Kernels of the switch counts and the first-contact times under a dwell-time prior (gauss_dwellevent.h, DESIGN.md section
// 27): plain fp64 vector code on the tables W and F of a GenericGaussianModel trajectory set and on the tables of the
// dwell-time recursion (gauss_dwell.h).  Everything is kept in logs, sums are (m, z) pairs of wave.h, no atomics: every value
// has one owner and every sum a fixed order that depends on the trajectory alone.
//
//   * dwell_level_kernel: level n of the forward recursion resolved by the number of switches, one launch per level.  A
//       workgroup owns 64 end frames b of one trajectory (lane = b) and takes the states in turn.  The eight waves stride the
//       switch frame c = n + q, n + q + 8, ..: row c - 1 of W and the run of log_dwell are read coalesced (the lane of b = T
//       reads log_surv), alpha_{n-1}(c, s) is one address for the wave.  A lane keeps a running (m, z); the waves' pairs meet
//       in LDS and wave 0 merges them in wave order.  Wave 0 then holds A_n(b, .) of its frame in registers, forms
//       alpha_n(b, .) from it (the jump mix, fused) and writes it to the row that level n + 1 reads; the lane of b = T
//       writes A_n(T, .).  Level n has nothing at b <= n: the launch starts at the tile of b = n + 1.
//   * dwell_contact_kernel: one wave per trajectory.  Lanes stride b for h(s), butterfly merges; then lanes stride t for
//       first(t), the states in ascending order, s' outside.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwellevent.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kWaves = kDwellEventWaves;

template <int S> __global__ void __launch_bounds__(kWaves * 64) dwell_level_kernel(DwellParams p, DwellLevels o, int n, int tile0)
{
    __shared__ double sh_m[kWaves][64], sh_z[kWaves][64];
    const int tiles = p.ntile - tile0;      // of the launch: blockIdx.x = trajectory x tile
    const int traj = (int)blockIdx.x / tiles;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int b0 = (tile0 + (int)blockIdx.x % tiles) * kDwellTile;
    if (b0 >= T) return;        // the whole workgroup
    const int b = b0 + 1 + lane;
    const bool mine = b <= T && b > n;
    const int c_end = min(b0 + kDwellTile, T);      // switches c < c_end can reach an end frame of the tile
    const double *__restrict__ prev = o.lev + ((int64_t)traj * 2 + ((n + 1) & 1)) * p.slot;
    double *__restrict__ next = o.lev + ((int64_t)traj * 2 + (n & 1)) * p.slot;

    double An[S];
    for (int s = 0; s < S; ++s) {
        double m = neg_inf(), z = 0.0;
        if (n == 0) {
            if (q == 0 && mine) {
                const double om = b == T ? p.log_surv[(int64_t)s * p.L + (T - 1)] : p.log_dwell[(int64_t)s * p.L + (b - 1)];
                const double f = td.F[(int64_t)s * (T + 1) + b];
                if (f == f) lse_add(m, z, p.log_init[s] + om + f);
            }
        } else if (mine) {
            const double *__restrict__ Ws = td.W + (int64_t)s * td.w_per_state;
            const double *__restrict__ dw = p.log_dwell + (int64_t)s * p.L, *__restrict__ sv = p.log_surv + (int64_t)s * p.L;
            const double *__restrict__ al = prev + (int64_t)s * ld;
            for (int c = n + q; c < c_end; c += kWaves) {
                const double a = al[c];
                if (!(a > neg_inf())) continue;     // the whole wave
                if (b <= c) continue;
                const double om = b == T ? sv[T - c - 1] : dw[b - c - 1];
                const double w = Ws[gauss_wrow(T, c - 1) + (b - c)];
                if (w != w) continue;
                lse_add(m, z, a + om + w);
            }
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
    if (q != 0 || b > T) return;
    if (b == T) {
        for (int s = 0; s < S; ++s) o.last[((int64_t)traj * (o.k_max + 1) + n) * S + s] = An[s];
        return;
    }
    for (int s = 0; s < S; ++s) {
        double m = neg_inf(), z = 0.0;
        for (int r = 0; r < S; ++r) lse_add(m, z, An[r] + p.log_jump[r * S + s]);
        next[(int64_t)s * ld + b] = lse_value(m, z);
    }
}

__global__ void __launch_bounds__(kDwellThreads) dwell_contact_kernel(DwellParams p, DwellContact o)
{
    const int lane = threadIdx.x & 63;
    const int traj = (int)blockIdx.x * (kDwellThreads / 64) + (threadIdx.x >> 6);
    if (traj >= p.n_traj) return;       // the whole wave
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, S = p.S, ld = p.ld;
    double *__restrict__ first = o.first + (int64_t)traj * ld;
    if (T < 1) {
        if (lane == 0) first[p.Tm] = neg_inf();
        return;
    }
    const int64_t base = (int64_t)traj * p.slot;
    const double *__restrict__ Ax = o.Ax + base, *__restrict__ beta = p.beta + base, *__restrict__ gamma = p.gamma + base;

    // first(0): the first segment is in G
    double fm = neg_inf(), fz = 0.0;
    for (int s = 0; s < S; ++s) {
        if (!(o.target >> s & 1u)) continue;
        const double init = p.log_init[s];
        if (!(init > neg_inf())) continue;
        const double *__restrict__ F = td.F + (int64_t)s * (T + 1);
        const double *__restrict__ dw = p.log_dwell + (int64_t)s * p.L;      // length b at dw[b - 1]
        const double surv = p.log_surv[(int64_t)s * p.L + (T - 1)];
        double m = neg_inf(), z = 0.0;
        for (int b = 1 + lane; b <= T; b += 64) {
            const double f = F[b];
            if (f == f) lse_add(m, z, (b < T ? dw[b - 1] : surv) + f + gamma[(int64_t)s * ld + b]);
        }
        for (int off = 32; off >= 1; off >>= 1) lse_merge(m, z, __shfl_xor(m, off, 64), __shfl_xor(z, off, 64));
        lse_merge(fm, fz, init + m, z);
    }
    if (lane == 0) first[0] = lse_value(fm, fz);

    // first(t): a jump at t from outside G into G
    for (int t = 1 + lane; t < T; t += 64) {
        double m = neg_inf(), z = 0.0;
        for (int r = 0; r < S; ++r) {
            if (o.target >> r & 1u) continue;
            const double a = Ax[(int64_t)r * ld + t];
            for (int s = 0; s < S; ++s)
                if (o.target >> s & 1u) lse_add(m, z, a + p.log_jump[r * S + s] + beta[(int64_t)s * ld + t]);
        }
        first[t] = lse_value(m, z);
    }
    if (lane == 0) {
        double m = neg_inf(), z = 0.0;
        for (int r = 0; r < S; ++r)
            if (!(o.target >> r & 1u)) lse_add(m, z, Ax[(int64_t)r * ld + T]);
        first[p.Tm] = lse_value(m, z);
    }
}

} // namespace

int launch_dwell_level(const DwellParams &p, const DwellLevels &o, int n, void *stream)
{
    const int tile0 = n / kDwellTile;       // the tile of b = n + 1
    if (n < 0 || n > o.k_max || tile0 >= p.ntile) return 1;
    const dim3 grid((unsigned)(p.ntile - tile0) * (unsigned)p.n_traj), block(kWaves * 64);
    switch (p.S) {
    case 1: hipLaunchKernelGGL(dwell_level_kernel<1>, grid, block, 0, (hipStream_t)stream, p, o, n, tile0); break;
    case 2: hipLaunchKernelGGL(dwell_level_kernel<2>, grid, block, 0, (hipStream_t)stream, p, o, n, tile0); break;
    case 3: hipLaunchKernelGGL(dwell_level_kernel<3>, grid, block, 0, (hipStream_t)stream, p, o, n, tile0); break;
    case 4: hipLaunchKernelGGL(dwell_level_kernel<4>, grid, block, 0, (hipStream_t)stream, p, o, n, tile0); break;
    default: return 1;
    }
    return launched();
}

int launch_dwell_contact(const DwellParams &p, const DwellContact &o, void *stream)
{
    const int waves = kDwellThreads / 64;
    hipLaunchKernelGGL(dwell_contact_kernel, dim3((unsigned)((p.n_traj + waves - 1) / waves)), dim3(kDwellThreads), 0, (hipStream_t)stream,
                       p, o);
    return launched();
}

} // namespace bild
