// Kernels of the exact posterior draws under a dwell-time prior (gauss_dwelldraw.h): plain fp64 vector
// code on the tables W and F of a GenericGaussianModel trajectory set and the tables beta and gamma of the dwell-time
// recursion's backward pass.  Every table holds logs.  No atomics.
//
//   * dwelldraw_head_kernel: one wave per trajectory finds the scale M (the largest term) and the total Z of the list of the
//     first pick, exp(log_init[s] + omega_s(0, b) + F[s][b] + gamma(b, s) - M) over (s, b): they belong to the trajectory, not
//     to a draw.
//   * dwelldraw_kernel: one wave per draw.  A pick over end frames b walks blocks of 64 ascending b, lane = b, so that the
//     row of W (or F), the run of log_dwell and the row of gamma are read coalesced; every lane forms exp(term - total) <= 1,
//     an inclusive scan across the lanes continues the running total, and a ballot finds the first lane of positive weight
//     whose total exceeds u times the list's total.  The wave stops at the first block that reaches it.  The total is the
//     table's own value (beta(t_i, s_i), gamma(t_i, s_{i-1}) for a state pick, or the head's pair), summed in another order
//     than the scan: where rounding carries the target past the scan's end, the last entry of positive weight is taken.  A
//     lane of weight 0 never qualifies.  The picks of a state run over S values and are done by every lane alike.  The bytes
//     of a segment are written by the lanes together as soon as its end is picked, byte x always by lane x mod 64.  The walk
//     of a pick over the blocks is wave.h's wave_pick, as in gauss_segdraw.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwelldraw.h"
#include "philox.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kThreads = kDwelldrawThreads;

// log weight of the entry b of a list: prior term + table entry + what can still follow; a NaN window weighs 0
__device__ __forceinline__ double entry(double prior, double w, double g) { return w == w ? prior + w + g : neg_inf(); }

__global__ void __launch_bounds__(kThreads) dwelldraw_head_kernel(DwelldrawParams p)
{
    const int lane = threadIdx.x & 63;
    const int traj = (int)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (traj >= p.n_traj) return;       // the whole wave
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    double best = neg_inf(), z = 0.0;
    for (int pass = 0; pass < 2 && T >= 1; ++pass) {
        for (int s = 0; s < p.S; ++s) {
            const double init = p.log_init[s], surv = p.log_surv[(int64_t)s * p.L + (T - 1)];
            if (!(init > neg_inf())) continue;
            const double *__restrict__ F = td.F + (int64_t)s * (T + 1);
            const double *__restrict__ dw = p.log_dwell + (int64_t)s * p.L;      // length b at dw[b - 1]
            const double *__restrict__ gam = p.gamma + (int64_t)traj * p.slot + (int64_t)s * p.ld;
            for (int b = 1 + lane; b <= T; b += 64) {
                const double t = entry(init + (b < T ? dw[b - 1] : surv), F[b], gam[b]);
                if (pass == 0)
                    best = fmax(best, t);
                else if (t > neg_inf())
                    z += exp(t - best);
            }
        }
        if (pass == 0) {
            // (wave_max, written out: through the helper the compiler keeps 8 more VGPRs here, a wave less per SIMD)
            for (int off = 32; off >= 1; off >>= 1) best = fmax(best, __shfl_xor(best, off, 64));
            if (!(best > neg_inf())) break;
        } else {
            z = wave_sum(z);
        }
    }
    if (lane == 0) {
        p.head[(int64_t)traj * 2] = best;
        p.head[(int64_t)traj * 2 + 1] = z;
    }
}

// The wave's pick among the end frames b = lo .. T of the list with weights exp(add + omega(b) + row[b] + gam[b] - shift),
// omega(b) = dw[b] for b < T and surv for b = T: the first b of positive weight whose running total, continued from `base`,
// exceeds `target`; 0 if the list ends before.  `base` and `last` (the last b of positive weight) are carried on.
__device__ __forceinline__ int dwelldraw_pick(const double *__restrict__ row, const double *__restrict__ dw, double surv, double add,
                                              const double *__restrict__ gam, int lo, int T, double shift, double target, int lane,
                                              double &base, int &last)
{
    return wave_pick(lo, T, target, lane, base, last, [&](int b) {
        const double t = entry(add + (b < T ? dw[b] : surv), row[b], gam[b]);
        return t > neg_inf() ? exp(t - shift) : 0.0;
    });
}

// frames [a, b) of a draw's row get state s: byte x by lane x mod 64, 64 consecutive bytes a store
__device__ __forceinline__ void put_states(uint8_t *row, int a, int b, int s, int lane)
{
    if (!row) return;
    for (int x = (a & ~63) + lane; x < b; x += 64)
        if (x >= a) row[x] = (uint8_t)s;
}

// (The parameter block is read from device memory where a value is needed, as in segdraw_kernel: passed as kernel arguments,
// all of it is held in scalar registers from the first instruction on.)
__global__ void __launch_bounds__(kThreads) dwelldraw_kernel(const DwelldrawParams *pp)
{
    const DwelldrawParams &p = *pp;
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * (kThreads / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= p.n_draws) return;     // the whole wave
    const int r = p.order[i], traj = p.slot_of[i];
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, S = p.S, L = p.L, U = p.U, ld = p.ld;
    const int64_t u0 = (int64_t)r * U;
    const int64_t sidx = p.stream ? p.stream[r] : (int64_t)r;
    uint8_t *row = p.states ? p.states + (int64_t)r * p.T_max : nullptr;
    const double *__restrict__ beta = p.beta + (int64_t)traj * p.slot, *__restrict__ gamma = p.gamma + (int64_t)traj * p.slot;
    // the uniforms of Philox(seed, 0, sidx) in the order of its uniform(): words 2, 3 of a block, then words 0, 1
    uint32_t pend0 = 0, pend1 = 0;
    int nu = 0;
    auto uniform = [&](double &u) {     // every lane alike; false: the replay row is used up
        if (p.uniforms) {
            if (nu >= U) return false;
            u = p.uniforms[u0 + nu];
        } else if (nu & 1) {
            u = philox_uniform(pend0, pend1);
        } else {
            uint32_t o[4];
            philox4x32_10((uint32_t)sidx, (uint32_t)((uint64_t)sidx >> 32), 0u, (uint32_t)(nu >> 1), (uint32_t)p.seed,
                          (uint32_t)(p.seed >> 32), o);
            u = philox_uniform(o[2], o[3]);
            pend0 = o[0], pend1 = o[1];
        }
        if (p.uniforms_out && nu < U && lane == 0) p.uniforms_out[u0 + nu] = u;
        ++nu;
        return true;
    };

    const double headM = p.head[(int64_t)traj * 2], headZ = p.head[(int64_t)traj * 2 + 1];
    bool ok = headZ > 0.0, short_row = false;
    int s = 0, t = 0, b = 0, k = 0;     // the state of the open segment, its start and its end; the switches so far
    double acc = 0.0, lp = 0.0, u = 0.0;
    if (ok && !uniform(u)) ok = false, short_row = true;
    if (ok) {
        // (s_0, t_1) over every state in turn, the running total carried on
        const double target = u * headZ;
        double base = 0.0;
        int last_s = -1, last_b = 0, sq = 0;
        for (; sq < S; ++sq) {
            const double init = p.log_init[sq];
            if (!(init > neg_inf())) continue;
            int last = 0;
            b = dwelldraw_pick(td.F + (int64_t)sq * (T + 1), p.log_dwell + (int64_t)sq * L - 1, p.log_surv[(int64_t)sq * L + (T - 1)], init,
                               gamma + (int64_t)sq * ld, 1, T, headM, target, lane, base, last);
            if (last) last_s = sq, last_b = last;
            if (b) break;
        }
        if (!b) sq = last_s, b = last_b;
        ok = b > 0;
        if (ok) {
            s = sq;
            acc += td.F[(int64_t)s * (T + 1) + b];
            lp = p.log_init[s];
            put_states(row, 0, b, s, lane);
        }
    }
    while (ok && b < T) {
        lp = lp + p.log_dwell[(int64_t)s * L + (b - t - 1)];
        t = b;
        // s_i among q ascending against log_jump[s][q] + beta(t, q): the total is gamma(t, s)
        if (!uniform(u)) {
            ok = false, short_row = true;
            break;
        }
        const double gt = gamma[(int64_t)s * ld + t];
        double cum = 0.0;
        int sn = -1, last_q = -1;
        for (int q = 0; q < S && sn < 0; ++q) {
            const double lw = p.log_jump[s * S + q] + beta[(int64_t)q * ld + t];
            const double e = lw > neg_inf() ? exp(lw - gt) : 0.0;
            cum += e;
            if (e > 0.0) {
                last_q = q;
                if (cum > u) sn = q;
            }
        }
        if (sn < 0) sn = last_q;
        ok = sn >= 0;
        if (!ok) break;
        lp = lp + p.log_jump[s * S + sn];
        s = __builtin_amdgcn_readfirstlane(sn);
        ++k;
        // t_{i+1} among b = t + 1 .. T against omega_s(t, b) + W[s][t - 1][b] + gamma(b, s): the total is beta(t, s)
        if (!uniform(u)) {
            ok = false, short_row = true;
            break;
        }
        const double *__restrict__ wrow = td.W + (int64_t)s * td.w_per_state + gauss_wrow(T, t - 1) - t;     // entry b at wrow[b]
        double base = 0.0;
        int last = 0;
        b = dwelldraw_pick(wrow, p.log_dwell + (int64_t)s * L - t - 1, p.log_surv[(int64_t)s * L + (T - t - 1)], 0.0, gamma + (int64_t)s * ld,
                           t + 1, T, beta[(int64_t)s * ld + t], u, lane, base, last);
        if (!b) b = last;
        ok = b > 0;
        if (!ok) break;
        acc += wrow[b];
        put_states(row, t, b, s, lane);
    }
    if (ok) lp = lp + p.log_surv[(int64_t)s * L + (T - t - 1)];

    // behind T, and a draw without a profile: 255 (byte x by lane x mod 64 here as well)
    if (row)
        for (int x = (ok ? (T & ~63) : 0) + lane; x < p.T_max; x += 64)
            if (!ok || x >= T) row[x] = 255;
    if (lane != 0) return;
    p.n_switches[r] = ok ? k : -1;
    p.logl[r] = ok ? acc : quiet_nan();
    p.log_prior[r] = ok ? lp : quiet_nan();
    p.n_uniforms[r] = short_row ? -1 : (ok ? nu : 0);
    if (!ok)
        for (int j = 0; p.uniforms_out && j < U; ++j) p.uniforms_out[u0 + j] = 0.0;
}

} // namespace

int launch_dwelldraw_head(const DwelldrawParams &p, void *stream)
{
    const int waves = kThreads / 64;
    hipLaunchKernelGGL(dwelldraw_head_kernel, dim3((unsigned)((p.n_traj + waves - 1) / waves)), dim3(kThreads), 0, (hipStream_t)stream, p);
    return launched();
}

int launch_dwelldraw(const DwelldrawParams &p, const DwelldrawParams *d_p, void *stream)
{
    const int waves = kThreads / 64;
    hipLaunchKernelGGL(dwelldraw_kernel, dim3((unsigned)((p.n_draws + waves - 1) / waves)), dim3(kThreads), 0, (hipStream_t)stream, d_p);
    return launched();
}

} // namespace bild
