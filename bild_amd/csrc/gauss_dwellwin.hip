// Kernel of the exact window support under a dwell-time prior (gauss_dwellwin.h): plain fp64 vector
// code on the tables W and F of a GenericGaussianModel trajectory set and on alpha and gamma of the dwell-time recursion
// (gauss_dwell.h).  Everything is kept in logs, sums are (m, z) pairs of wave.h, no atomics: every value has one owner and every
// sum a fixed order that depends on the trajectory and the query alone.
//
//   * dwell_window_kernel: one workgroup of eight waves per query (u, v, G); the states outside G are skipped by the mask.
//       The window chain, tiles of 64 end frames b = b0 + 1 + lane from b0 = u, b < v:
//         part 1, starts c <= b0: the waves take c = q, q + 8, ..; row c - 1 of W (F for c = 0) is read coalesced along b, the
//         head is one address for the wave: log_init for c = 0, alpha(c, .) for c <= u, kappa(c, .) from the query's scratch
//         row behind it.  A lane keeps a running (m, z); the waves' pairs meet in LDS and wave 0 merges them in wave order.
//         part 2, the tile's triangle, wave 0 alone, as dwell_forward_kernel's: at step c lane c's C(c, .) is complete and goes
//         to every lane by a shuffle, every lane forms kappa(c, .) over the states of G from it, lane c writes it to the
//         scratch row, and the lanes b > c add their term.  The W and prior entries of step c + 1 are loaded before the
//         arithmetic of step c.
//       The closure: the waves take the rows c = q, q + 8, .. < v, the lanes stride b = v + lane, v + lane + 64, .. <= T with
//         gamma(b, s); states ascending outside, rows inside, one (m, z) a lane; a butterfly of pair merges, the waves' pairs
//         in LDS, thread 0 merges them in wave order and stores num.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwellwin.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kWaves = kDwellWinWaves;

// log prior weight of a segment [a, b) in state s: the last segment is censored
__device__ __forceinline__ double omega(const DwellParams &p, int s, int a, int b, int T)
{
    return b == T ? p.log_surv[(int64_t)s * p.L + (T - a - 1)] : p.log_dwell[(int64_t)s * p.L + (b - a - 1)];
}

template <int S> __global__ void __launch_bounds__(kWaves * 64) dwell_window_kernel(DwellParams p, DwellWindows o)
{
    __shared__ double sh_m[kWaves][64], sh_z[kWaves][64];
    const DwellWinQuery qd = o.queries[blockIdx.x];
    const GaussTraj td = p.trajs[qd.traj];
    const int T = td.T, ld = p.ld, u = qd.u, v = qd.v;
    const int n = v - u - 1;        // frames of the chain: c = u + 1 .. v - 1
    const unsigned G = qd.target;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const double *__restrict__ al = p.alpha + (int64_t)qd.traj * p.slot;
    const double *__restrict__ gamma = p.gamma + (int64_t)qd.traj * p.slot;
    double *kap = o.kappa + qd.kappa;

    // the head of a segment that starts at c (the whole wave), and its table entry at end frame b > c
    auto head = [&](int c, int s) { return c == 0 ? p.log_init[s] : c <= u ? al[(int64_t)s * ld + c] : kap[(int64_t)s * n + (c - u - 1)]; };
    auto entry = [&](int c, int b, int s) {
        return c == 0 ? td.F[(int64_t)s * (T + 1) + b] : td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, c - 1) + (b - c)];
    };

    double jm[S][S];
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) jm[a][b] = p.log_jump[a * S + b];

    for (int b0 = u; b0 < v - 1; b0 += kDwellTile) {
        const int b = b0 + 1 + lane;
        const bool mine = b < v;
        double Sm[S], Sz[S];
        // part 1: the starts c <= b0
        for (int s = 0; s < S; ++s) {
            double m = neg_inf(), z = 0.0;
            if ((G >> s & 1u) && mine) {
                for (int c = q; c <= b0; c += kWaves) {
                    const double h = head(c, s);
                    if (!(h > neg_inf())) continue;     // the whole wave
                    const double om = omega(p, s, c, b, T);
                    const double w = entry(c, b, s);
                    if (w != w) continue;
                    lse_add(m, z, h + om + w);
                }
            }
            sh_m[q][lane] = m;
            sh_z[q][lane] = z;
            __syncthreads();
            if (q == 0) {
                for (int r = 1; r < kWaves; ++r) lse_merge(m, z, sh_m[r][lane], sh_z[r][lane]);
                Sm[s] = m, Sz[s] = z;
            }
            __syncthreads();
        }
        // part 2: the tile's own starts, c = b0 + 1 + lc < v
        if (q == 0) {
            const int nstep = min(kDwellTile, v - 1 - b0);
            double wn[S], on[S];
            for (int s = 0; s < S; ++s) {
                const int c = b0 + 1;
                const bool use = (G >> s & 1u) && mine && b > c;
                wn[s] = use ? entry(c, b, s) : 0.0;
                on[s] = use ? omega(p, s, c, b, T) : neg_inf();
            }
            for (int lc = 0; lc < nstep; ++lc) {
                const int c = b0 + 1 + lc;
                double wc[S], oc[S];
                for (int s = 0; s < S; ++s) {
                    wc[s] = wn[s], oc[s] = on[s];
                    const bool use = (G >> s & 1u) && mine && b > c + 1 && lc + 1 < nstep;
                    wn[s] = use ? entry(c + 1, b, s) : 0.0;
                    on[s] = use ? omega(p, s, c + 1, b, T) : neg_inf();
                }
                double Cc[S];
                for (int s = 0; s < S; ++s) Cc[s] = (G >> s & 1u) ? lse_value(__shfl(Sm[s], lc, 64), __shfl(Sz[s], lc, 64)) : neg_inf();
                for (int s = 0; s < S; ++s) {
                    if (!(G >> s & 1u)) continue;
                    double m = neg_inf(), z = 0.0;
                    for (int r = 0; r < S; ++r)
                        if (G >> r & 1u) lse_add(m, z, Cc[r] + jm[r][s]);
                    const double ks = lse_value(m, z);
                    if (lane == lc) kap[(int64_t)s * n + (c - u - 1)] = ks;
                    if (!(mine && b > c && ks > neg_inf() && oc[s] > neg_inf())) continue;
                    if (wc[s] != wc[s]) continue;
                    lse_add(Sm[s], Sz[s], ks + oc[s] + wc[s]);
                }
            }
        }
        __syncthreads();    // the tile's kappa is in memory before the next tile and the closure read it
    }

    // the closure: rows c < v against the end frames b >= v
    double m = neg_inf(), z = 0.0;
    for (int s = 0; s < S; ++s) {
        if (!(G >> s & 1u)) continue;
        for (int c = q; c < v; c += kWaves) {
            const double h = head(c, s);
            if (!(h > neg_inf())) continue;     // the whole wave
            for (int b = v + lane; b <= T; b += 64) {
                const double g = gamma[(int64_t)s * ld + b];
                if (!(g > neg_inf())) continue;
                const double om = omega(p, s, c, b, T);
                if (!(om > neg_inf())) continue;
                const double w = entry(c, b, s);
                if (w != w) continue;
                lse_add(m, z, h + om + w + g);
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) lse_merge(m, z, __shfl_xor(m, off, 64), __shfl_xor(z, off, 64));
    if (lane == 0) sh_m[q][0] = m, sh_z[q][0] = z;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int r = 1; r < kWaves; ++r) lse_merge(m, z, sh_m[r][0], sh_z[r][0]);
    o.num[blockIdx.x] = lse_value(m, z);
}

} // namespace

int launch_dwell_windows(const DwellParams &p, const DwellWindows &o, void *stream)
{
    if (o.n < 1) return 1;
    const dim3 grid((unsigned)o.n), block(kWaves * 64);
    switch (p.S) {
    case 2: hipLaunchKernelGGL(dwell_window_kernel<2>, grid, block, 0, (hipStream_t)stream, p, o); break;
    case 3: hipLaunchKernelGGL(dwell_window_kernel<3>, grid, block, 0, (hipStream_t)stream, p, o); break;
    case 4: hipLaunchKernelGGL(dwell_window_kernel<4>, grid, block, 0, (hipStream_t)stream, p, o); break;
    default: return 1;      // (one state has no proper subset: the call refuses it)
    }
    return launched();
}

} // namespace bild
