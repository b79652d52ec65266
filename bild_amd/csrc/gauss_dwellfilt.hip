// The kernel of the exact online filter under a dwell-time prior (gauss_dwellfilt.h).  Plain fp64 vector
// code; no atomics, every value has one owner and every sum a fixed order that depends on the trajectory alone.
//
//   * dwell_filter_kernel: one workgroup of kDwellWaves waves per (trajectory, tile of 64 prefix ends b), lane = b, tiles cut
//     from frame 0 of the trajectory: part 1 of dwell_forward_kernel with log_surv in place of log_dwell.  alpha is complete,
//     so the tile's own triangle is the lane predicate c < b.  The states are walked inside the workgroup.  The waves take the
//     switches c = 1 + q, 1 + q + 8, ..; row c - 1 of W and the run of log_surv are read coalesced across the lanes (log_dwell
//     only where a window is NaN, for its count), alpha(c, s) and alphaArg are the same for the whole wave; the loads of kDwellFiltAhead switches are issued before
//     their arithmetic.  A lane keeps (m, z, r) per state: (m, z) as lse_add keeps them, r = sum (b - c) exp(term - m) on the
//     same scale.  The waves' triples and the two counts of skipped NaN windows meet in LDS and wave 0 merges them in wave
//     order.  Behind the states wave 0 forms E(b), log_filtered and run_mean.
//     With log_run asked for, a second sweep of the same workgroup writes term - E(b) for the run lengths r = 1 .. min(R, b):
//     a wave per end frame b of the tile, lane = r, so that a row of the output is written coalesced; alpha and log_surv are
//     contiguous across the lanes, the entries W[s][b - r - 1][b] are a gather down a column.
//   S is a run-time value.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwellfilt.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kWaves = kDwellWaves;
constexpr int kDwellFiltAhead = 2;  // switches of one wave whose loads are in flight together: 4 cost 151 VGPRs and a workgroup a CU

__global__ void __launch_bounds__(kWaves * 64) dwell_filter_kernel(DwellParams p, DwellFilter o)
{
    __shared__ double sh_m[kWaves][64], sh_z[kWaves][64], sh_r[kWaves][64];
    __shared__ double sh_G[kDwellMaxS][64], sh_len[kDwellMaxS][64], sh_E[64];
    __shared__ int sh_ns[kWaves][64], sh_nd[kWaves][64];
    const int traj = blockIdx.x, b0 = (int)blockIdx.y * kDwellTile;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld, S = p.S, Tm = p.Tm;
    if (b0 >= T) return;    // the whole workgroup
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int b = b0 + 1 + lane;
    const bool mine = b <= T;
    const int c_end = min(b0 + kDwellTile, T);      // the switches c < c_end start a window that ends inside the tile
    const int64_t base = (int64_t)traj * p.slot;
    const double *__restrict__ al = p.alpha + base;
    const int32_t *__restrict__ alArg = p.alphaArg + base;

    int n_surv = 0, n_dwell = 0;
    for (int s = 0; s < S; ++s) {
        const double *__restrict__ Ws = td.W + (int64_t)s * td.w_per_state;
        const double *__restrict__ surv = p.log_surv + (int64_t)s * p.L;
        const double *__restrict__ dwell = p.log_dwell + (int64_t)s * p.L;
        double m = neg_inf(), z = 0.0, r = 0.0;
        // the first segment [0, b)
        if (q == 0 && mine && p.log_init[s] > neg_inf()) {
            const double f = td.F[(int64_t)s * (T + 1) + b];
            if (f != f) {
                n_surv += surv[b - 1] > neg_inf();
                n_dwell += dwell[b - 1] > neg_inf();
            } else {
                lse_add_len(m, z, r, p.log_init[s] + surv[b - 1] + f, (double)b);
            }
        }
        // the switches c = 1 .. b - 1
        for (int c0 = 1 + q; c0 < c_end; c0 += kDwellFiltAhead * kWaves) {
            double hv[kDwellFiltAhead], sv[kDwellFiltAhead], wv[kDwellFiltAhead];
#pragma unroll
            for (int i = 0; i < kDwellFiltAhead; ++i) {
                const int c = c0 + i * kWaves;
                const bool use = c < c_end && mine && c < b && alArg[s * ld + c] >= 0;
                hv[i] = use ? al[s * ld + c] : neg_inf();
                sv[i] = use ? surv[b - c - 1] : neg_inf();
                wv[i] = use ? Ws[gauss_wrow(T, c - 1) + (b - c)] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < kDwellFiltAhead; ++i) {
                const int c = c0 + i * kWaves;
                if (wv[i] != wv[i]) {   // (rare: log_dwell is read for the count alone)
                    n_surv += sv[i] > neg_inf();
                    n_dwell += dwell[b - c - 1] > neg_inf();
                } else {
                    lse_add_len(m, z, r, hv[i] + sv[i] + wv[i], (double)(b - c));
                }
            }
        }
        sh_m[q][lane] = m;
        sh_z[q][lane] = z;
        sh_r[q][lane] = r;
        __syncthreads();
        if (q == 0) {
            double top = neg_inf();
            for (int w = 0; w < kWaves; ++w)
                if (sh_z[w][lane] > 0.0) top = fmax(top, sh_m[w][lane]);
            z = 0.0, r = 0.0;
            for (int w = 0; w < kWaves; ++w) {
                const double wz = sh_z[w][lane];
                if (wz > 0.0) {
                    const double e = exp(sh_m[w][lane] - top);
                    z += wz * e;
                    r += sh_r[w][lane] * e;
                }
            }
            sh_G[s][lane] = lse_value(top, z);
            sh_len[s][lane] = z > 0.0 ? r / z : 0.0;    // the mean length of the current segment given theta_t = s
        }
        __syncthreads();
    }
    sh_ns[q][lane] = n_surv;
    sh_nd[q][lane] = n_dwell;
    __syncthreads();
    if (q == 0) {
        double m = neg_inf(), z = 0.0;
        for (int s = 0; s < S; ++s) lse_add(m, z, sh_G[s][lane]);
        const double E = lse_value(m, z);
        const bool live = E > neg_inf();
        sh_E[lane] = E;
        if (mine) {
            const int64_t row = (int64_t)traj * Tm + (b - 1);
            double mean = 0.0;
            for (int s = 0; s < S; ++s) {
                const double g = sh_G[s][lane];
                o.filt[((int64_t)traj * S + s) * Tm + (b - 1)] = live ? g - E : quiet_nan();
                if (live && g > neg_inf()) mean += exp(g - E) * sh_len[s][lane];
            }
            int ns = 0, nd = 0;
            for (int w = 0; w < kWaves; ++w) ns += sh_ns[w][lane], nd += sh_nd[w][lane];
            o.prefix[row] = E;
            o.run_mean[row] = live ? mean : quiet_nan();
            o.n_surv[row] = ns;
            o.n_dwell[row] = nd;
        }
    }
    if (!o.log_run) return;     // the whole grid
    __syncthreads();

    // the run lengths: a wave per end frame of the tile, lane = r
    const int R = o.R;
    for (int lb = q; lb < kDwellTile && b0 + 1 + lb <= T; lb += kWaves) {
        const int be = b0 + 1 + lb;
        const double E = sh_E[lb];
        const bool live = E > neg_inf();
        for (int s = 0; s < S; ++s) {
            const double *__restrict__ Ws = td.W + (int64_t)s * td.w_per_state;
            const double *__restrict__ surv = p.log_surv + (int64_t)s * p.L;
            double *__restrict__ out = o.log_run + (((int64_t)traj * S + s) * Tm + (be - 1)) * R;
            for (int r0 = 0; r0 < R; r0 += 64) {
                const int len = r0 + 1 + lane;
                if (len > R) continue;
                double v = live ? neg_inf() : quiet_nan();
                if (live && len <= be) {
                    const int c = be - len;
                    double head, w;
                    if (c == 0) {
                        head = p.log_init[s];
                        w = td.F[(int64_t)s * (T + 1) + be];
                    } else {
                        head = alArg[s * ld + c] >= 0 ? al[s * ld + c] : neg_inf();
                        w = Ws[gauss_wrow(T, c - 1) + len];
                    }
                    const double term = head + surv[len - 1] + w;
                    if (w == w && term > neg_inf()) v = term - E;
                }
                out[len - 1] = v;
            }
        }
    }
}

} // namespace

int launch_dwell_filter(const DwellParams &p, const DwellFilter &o, void *stream)
{
    const dim3 grid((unsigned)p.n_traj, (unsigned)p.ntile);
    hipLaunchKernelGGL(dwell_filter_kernel, grid, dim3(kWaves * 64), 0, (hipStream_t)stream, p, o);
    return launched();
}

} // namespace bild
