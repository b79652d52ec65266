// Kernels of the exact posterior draws (gauss_segdraw.h): plain fp64 vector code on the tables W and
// F of a GenericGaussianModel trajectory set and the backward tables of the segment recursion.  No atomics.
//
//   * segdraw_head_kernel: one wave per (trajectory, k) finds the scale M and the total Z of the list of the first pick,
//     exp F[s][b] gamma_k(b, s) over (s, b): they belong to the trajectory, not to a draw.
//   * segdraw_kernel: one wave per draw.  A pick over end frames b walks blocks of 64 ascending b, lane = b, so that row
//     t_i - 1 of W and the row of gamma are read coalesced; every lane forms Z_gamma exp(W + M_gamma - M) <= 1, an inclusive
//     scan across the lanes continues the running total, and a ballot finds the first lane of positive weight whose total
//     exceeds u times the list's total.  The wave stops at the first block that reaches it.  The total is the table's own
//     value (beta_m(t_i, s_i), or the head's Z), summed in another order than the scan: where rounding carries the target
//     past the scan's end, the last entry of positive weight is taken.  A lane of weight 0 never qualifies.  The picks of a
//     state run over S values and are done by every lane alike.  The walk of a pick over the blocks is wave.h's wave_pick,
//     as in gauss_dwelldraw.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_segdraw.h"
#include "philox.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kThreads = kSegdrawThreads;

__device__ __forceinline__ int64_t at(const SegdrawParams &p, int traj, int level, int s, int b)
{
    return (int64_t)traj * p.slot + ((int64_t)level * p.S + s) * p.ld + b;
}

__global__ void __launch_bounds__(kThreads) segdraw_head_kernel(SegdrawParams p)
{
    const int traj = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (k >= p.K) return;       // the whole wave
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, hi = T - k;     // gamma_k(b, .) is empty behind T - k
    double best = neg_inf(), z = 0.0;
    for (int s = 0; s < p.S; ++s) {
        const int64_t base = at(p, traj, k, s, 0);
        const double *__restrict__ gM = p.gamma.M + base, *__restrict__ gZ = p.gamma.Z + base;
        const double *__restrict__ F = td.F + (int64_t)s * (T + 1);
        for (int b = 1 + lane; b <= hi; b += 64) {
            if (!(gZ[b] > 0.0)) continue;
            const double t = gM[b] + F[b];      // NaN compares false
            if (t > best) best = t;
        }
    }
    best = wave_max(best);
    if (best > neg_inf()) {
        for (int s = 0; s < p.S; ++s) {
            const int64_t base = at(p, traj, k, s, 0);
            const double *__restrict__ gM = p.gamma.M + base, *__restrict__ gZ = p.gamma.Z + base;
            const double *__restrict__ F = td.F + (int64_t)s * (T + 1);
            for (int b = 1 + lane; b <= hi; b += 64) {
                const double gz = gZ[b], f = F[b];
                if (!(gz > 0.0) || f != f) continue;
                z += gz * exp(gM[b] + f - best);
            }
        }
        z = wave_sum(z);
    }
    if (lane == 0) {
        p.head[((int64_t)traj * p.K + k) * 2] = best;
        p.head[((int64_t)traj * p.K + k) * 2 + 1] = z;
    }
}

// The wave's pick among the end frames b = lo .. hi of the list with weights gZ[b] exp(row[b] + gM[b] - M): the first b of
// positive weight whose running total, continued from `base`, exceeds `target`; 0 if the list ends before.  `base` and
// `last` (the last b of positive weight) are carried on.
__device__ __forceinline__ int segdraw_pick(const double *__restrict__ row, const double *__restrict__ gM, const double *__restrict__ gZ, int lo,
                                            int hi, double M, double target, int lane, double &base, int &last)
{
    return wave_pick(lo, hi, target, lane, base, last, [&](int b) {
        const double gz = gZ[b], w = row[b];
        return gz > 0.0 && w == w ? gz * exp(gM[b] + w - M) : 0.0;
    });
}

// (The parameter block is read from device memory where a value is needed: passed as kernel arguments, all of it is held in
// scalar registers from the first instruction on, and the compiler spills 55 of them.)
__global__ void __launch_bounds__(kThreads) segdraw_kernel(const SegdrawParams *pp)
{
    const SegdrawParams &p = *pp;
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * (kThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= p.n_draws) return;     // the whole wave
    const int r = p.order[i], traj = p.slot_of[i], k = p.draw_k[r];
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, S = p.S, K = p.K, U = p.U;
    const int64_t seg0 = (int64_t)r * K, u0 = (int64_t)r * U;      // the draw's rows of segments and of uniforms
    // the uniforms of Philox(seed, 0, r) in the order of its uniform(): words 2, 3 of a block, then words 0, 1
    uint32_t pend0 = 0, pend1 = 0;
    int nu = 0;
    auto uniform = [&]() {      // every lane alike
        double u;
        if (p.uniforms) {
            u = p.uniforms[u0 + nu];
        } else if (nu & 1) {
            u = philox_uniform(pend0, pend1);
        } else {
            uint32_t o[4];
            philox4x32_10((uint32_t)r, 0u, 0u, (uint32_t)(nu >> 1), (uint32_t)p.seed, (uint32_t)(p.seed >> 32), o);
            u = philox_uniform(o[2], o[3]);
            pend0 = o[0], pend1 = o[1];
        }
        if (p.uniforms_out && lane == 0) p.uniforms_out[u0 + nu] = u;
        ++nu;
        return u;
    };

    const double *__restrict__ head = p.head + ((int64_t)traj * K + k) * 2;     // M and Z of the first list
    bool ok = head[1] > 0.0;
    int s = 0, t = 0;       // the state of the open segment and its start
    double acc = 0.0;
    for (int j = 0; ok && j <= k; ++j) {
        const int m = k - j;    // switches still to come behind the segment that is open
        double M = head[0], total = head[1];
        int s_lo = 0, s_hi = S - 1;     // j = 0: (s_0, t_1) over every state in turn, the running total carried on
        if (j > 0) {
            // s_j among the allowed q, ascending, against beta_m(t, q)
            // (their scale and total are gamma_{m+1}(t, s), which segdp_bmix_kernel summed over the same q in the same order)
            const int64_t gs = at(p, traj, m + 1, s, t);
            const double best = p.gamma.M[gs], tot = p.gamma.Z[gs];
            const double target = uniform() * tot;
            double cum = 0.0;
            int sn = -1, last = -1;
            for (int q = 0; q < S && sn < 0; ++q) {
                if (!p.tr[s * S + q]) continue;
                const int64_t g = at(p, traj, m, q, t);
                const double zq = p.beta.Z[g];
                const double e = zq > 0.0 ? zq * exp(p.beta.M[g] - best) : 0.0;
                cum += e;
                if (e > 0.0) {
                    last = q;
                    if (cum > target) sn = q;
                }
            }
            if (sn < 0) sn = last;
            ok = sn >= 0;
            if (!ok) break;
            s = sn;
            if (lane == 0) p.seg_start[seg0 + j] = t, p.seg_state[seg0 + j] = s;
            if (m == 0) {       // the last segment ends at T
                acc += td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, t - 1) + (T - t)];
                break;
            }
            // t_{j+1} among b = t + 1 .. T - m against exp W[s][t - 1][b] gamma_m(b, s): the total is beta_m(t, s)
            const int64_t g = at(p, traj, m, s, t);
            M = p.beta.M[g], total = p.beta.Z[g];
            s_lo = s_hi = s;
        }
        const double target = uniform() * total;
        const int64_t woff = j > 0 ? gauss_wrow(T, t - 1) - t : 0;      // entry b of a state's row at row[b]
        double base = 0.0;
        int last_s = -1, last_b = 0, b = 0, sq = s_lo;
        for (; sq <= s_hi; ++sq) {
            const double *__restrict__ row = j > 0 ? td.W + (int64_t)sq * td.w_per_state + woff : td.F + (int64_t)sq * (T + 1);
            const int64_t g = at(p, traj, m, sq, 0);
            int last = 0;
            b = segdraw_pick(row, p.gamma.M + g, p.gamma.Z + g, t + 1, T - m, M, target, lane, base, last);
            if (last) last_s = sq, last_b = last;
            if (b) break;
        }
        if (!b) sq = last_s, b = last_b;
        ok = b > 0;
        if (!ok) break;
        s = sq;
        if (j == 0 && lane == 0) p.seg_start[seg0] = 0, p.seg_state[seg0] = s;
        acc += j > 0 ? td.W[(int64_t)s * td.w_per_state + woff + b] : td.F[(int64_t)s * (T + 1) + b];
        t = b;
    }
    if (lane != 0) return;
    if (ok) {
        for (int j = k + 1; j < K; ++j) p.seg_start[seg0 + j] = T, p.seg_state[seg0 + j] = 0;
        p.logl[r] = acc;
    } else {
        for (int j = 0; j < K; ++j) p.seg_start[seg0 + j] = -1, p.seg_state[seg0 + j] = -1;
        p.logl[r] = quiet_nan();
        for (int j = 0; p.uniforms_out && j < U; ++j) p.uniforms_out[u0 + j] = 0.0;
    }
}

} // namespace

int launch_segdraw_head(const SegdrawParams &p, void *stream)
{
    const int waves = kThreads / 64;
    const dim3 grid((unsigned)((p.K + waves - 1) / waves), (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdraw_head_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    return launched();
}

int launch_segdraw(const SegdrawParams &p, const SegdrawParams *d_p, void *stream)
{
    const int waves = kThreads / 64;
    hipLaunchKernelGGL(segdraw_kernel, dim3((unsigned)((p.n_draws + waves - 1) / waves)), dim3(kThreads), 0, (hipStream_t)stream, d_p);
    return launched();
}

} // namespace bild
