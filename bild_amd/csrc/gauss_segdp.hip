// Kernels of the segment recursion (gauss_segdp.h): plain fp64 vector code on the tables W and F of a
// GenericGaussianModel trajectory set.  No atomics: every value has one owner, and every sum a fixed order.
//
//   * segdp_init_kernel: A_0 = F and gamma_0 = [b == T].
//   * segdp_mix_kernel / segdp_bmix_kernel: one lane per (frame, state) sums the previous level over the allowed states.
//   * segdp_level_kernel: A_j(b, s) = sum_c alpha_j(c, s) exp W[s][c - 1][b].  A workgroup owns 64 end frames b of one
//     (trajectory, s); lane = b, so that row c - 1 of W is read coalesced while c advances, and alpha_j(c, s) is the same
//     for the whole wave.  The sixteen waves take c = j + q, j + q + 16, ...; pass 1 finds the maximum and its c, the waves'
//     results meet in LDS (ties: the smaller c), pass 2 sums exp(term - maximum) <= 1 and the waves' sums are added in
//     wave order.
//   * segdp_blevel_kernel: beta_m(a, s) = sum_b exp W[s][a - 1][b] gamma_m(b, s), one wave per row a, lanes stride b,
//     butterfly reductions.
//   * segdp_backtrack_kernel: one lane per (trajectory, k) follows the back-pointers.
//   * segdp_cover_kernel / segdp_carry_kernel: the marginals.  The weight of a segment [a, b) in state s within the
//     profiles of k switches is Q = sum_j alpha_j(a, s) exp W[s][a - 1][b] gamma_{k-j}(b, s); frame t collects Q of every
//     a <= t < b.  A wave owns 64 frames t = b - 1 of one (trajectory, k, s) and walks the rows a: a suffix sum across the
//     lanes gives each t the row's terms with b > t inside the tile, and the row's total goes to row_tot.  The carry kernel
//     adds, per t, the totals of the tiles to the right over the rows a <= t.  Sums of non-negative terms only.
// The reductions and scans across a wave and the carry's body are those of wave.h, which gauss_dwell.hip uses too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_segdp.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kThreads = kSegdpThreads;

__device__ __forceinline__ int64_t at(const SegdpParams &p, int traj, int level, int s, int b)
{
    return (int64_t)traj * p.slot + ((int64_t)level * p.S + s) * p.ld + b;
}

__global__ void __launch_bounds__(kThreads) segdp_init_kernel(SegdpParams p, int backward)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const int b = (int)(blockIdx.x * kThreads + threadIdx.x);
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    if (b > T) return;
    const int64_t i = at(p, traj, 0, s, b);
    if (backward) {
        p.gamma.M[i] = b == T ? 0.0 : neg_inf();
        p.gamma.Z[i] = b == T ? 1.0 : 0.0;
        return;
    }
    const double f = b >= 1 ? td.F[(int64_t)s * (T + 1) + b] : 0.0;
    const bool nan = f != f, none = b < 1;
    const bool live = !none && !nan && f > neg_inf();
    p.A.M[i] = none || nan ? neg_inf() : f;
    p.A.Z[i] = live ? 1.0 : 0.0;
    p.A.R[i] = live ? f : 0.0;
    p.A.ok[i] = none || nan ? 0.0 : 1.0;
    p.A.bad[i] = !none && nan ? 1.0 : 0.0;
    p.A.arg[i] = none || nan ? -1 : 0;
}

// alpha_j(c, s) from A_{j-1}(c, s') over the s' with transitions[s'][s]; ties of the maximum: the smallest s'
__global__ void __launch_bounds__(kThreads) segdp_mix_kernel(SegdpParams p, int j)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const int c = (int)(blockIdx.x * kThreads + threadIdx.x);
    const int T = p.trajs[traj].T;
    if (c > T) return;
    const int S = p.S;
    double best = neg_inf(), ok = 0.0, bad = 0.0;
    int arg = -1;
    for (int q = 0; q < S; ++q) {
        if (!p.tr[q * S + s]) continue;
        const int64_t i = at(p, traj, j - 1, q, c);
        const double okq = p.A.ok[i];
        ok += okq;
        bad += p.A.bad[i];
        const double m = p.A.M[i];
        if (okq > 0.0 && (arg < 0 || m > best)) {
            best = m;
            arg = q;
        }
    }
    double z = 0.0, u = 0.0;
    if (arg >= 0 && best > neg_inf()) {
        for (int q = 0; q < S; ++q) {
            if (!p.tr[q * S + s]) continue;
            const int64_t i = at(p, traj, j - 1, q, c);
            const double zq = p.A.Z[i];
            if (!(zq > 0.0)) continue;
            const double w = zq * exp(p.A.M[i] - best);
            z += w;
            if (w > 0.0) u += w * p.A.R[i];
        }
    }
    const int64_t o = at(p, traj, j, s, c);
    p.alpha.M[o] = best;
    p.alpha.Z[o] = z;
    p.alpha.R[o] = z > 0.0 ? u / z : 0.0;
    p.alpha.ok[o] = ok;
    p.alpha.bad[o] = bad;
    p.alpha.arg[o] = arg;
}

__global__ void __launch_bounds__(kSegdpSlices * 64) segdp_level_kernel(SegdpParams p, int j)
{
    __shared__ double sh_best[kSegdpSlices][kSegdpTile], sh_ok[kSegdpSlices][kSegdpTile], sh_bad[kSegdpSlices][kSegdpTile];
    __shared__ int sh_arg[kSegdpSlices][kSegdpTile];
    const int traj = blockIdx.z, s = blockIdx.y;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int b0 = (int)blockIdx.x * kSegdpTile;
    if (b0 > T) return;     // the whole workgroup
    const int b = b0 + lane;
    const bool mine = b <= T;
    const int c_end = min(b0 + kSegdpTile - 1, T);      // switches c < c_end can reach an end frame of the tile
    const double *__restrict__ W = td.W + (int64_t)s * td.w_per_state;
    const int64_t base = at(p, traj, j, s, 0);
    const double *__restrict__ aM = p.alpha.M + base, *__restrict__ aZ = p.alpha.Z + base, *__restrict__ aR = p.alpha.R + base;
    const double *__restrict__ aok = p.alpha.ok + base, *__restrict__ abad = p.alpha.bad + base;

    // pass 1: the maximum, its switch frame, and the counts
    double best = neg_inf(), ok = 0.0, bad = 0.0;
    int arg = -1;
    for (int c = j + q; c < c_end; c += kSegdpSlices) {
        const double cok = aok[c], cbad = abad[c];
        if (cok + cbad == 0.0) continue;    // no trace reaches (j, s) by frame c: nothing to add, a NaN window included
        if (!(mine && b > c)) continue;
        const double w = W[gauss_wrow(T, c - 1) + (b - c)];
        if (w != w) {
            bad += cok + cbad;
            continue;
        }
        ok += cok;
        bad += cbad;
        const double t = aM[c] + w;
        if (cok > 0.0 && (arg < 0 || t > best)) {
            best = t;
            arg = c;
        }
    }
    sh_best[q][lane] = best;
    sh_arg[q][lane] = arg;
    sh_ok[q][lane] = ok;
    sh_bad[q][lane] = bad;
    __syncthreads();
    best = neg_inf(), arg = -1, ok = 0.0, bad = 0.0;
    for (int r = 0; r < kSegdpSlices; ++r) {
        const double v = sh_best[r][lane];
        const int a = sh_arg[r][lane];
        if (a >= 0 && (arg < 0 || v > best || (v == best && a < arg))) {
            best = v;
            arg = a;
        }
        ok += sh_ok[r][lane];
        bad += sh_bad[r][lane];
    }
    __syncthreads();

    // pass 2: sum exp(term - best) and the weighted log-likelihoods
    double z = 0.0, u = 0.0;
    if (arg >= 0 && best > neg_inf()) {
        for (int c = j + q; c < c_end; c += kSegdpSlices) {
            const double cz = aZ[c];
            if (!(cz > 0.0)) continue;
            if (!(mine && b > c)) continue;
            const double w = W[gauss_wrow(T, c - 1) + (b - c)];
            if (w != w) continue;
            const double e = cz * exp(aM[c] + w - best);
            z += e;
            if (e > 0.0) u += e * (aR[c] + w);
        }
    }
    sh_best[q][lane] = z;
    sh_ok[q][lane] = u;
    __syncthreads();
    if (q != 0 || !mine) return;
    z = 0.0, u = 0.0;
    for (int r = 0; r < kSegdpSlices; ++r) {
        z += sh_best[r][lane];
        u += sh_ok[r][lane];
    }
    const int64_t o = base + b;
    p.A.M[o] = best;
    p.A.Z[o] = z;
    p.A.R[o] = z > 0.0 ? u / z : 0.0;
    p.A.ok[o] = ok;
    p.A.bad[o] = bad;
    p.A.arg[o] = arg;
}

// beta_m(a, s): one wave per row a (a = 0 has no window and stays empty)
__global__ void __launch_bounds__(kThreads) segdp_blevel_kernel(SegdpParams p, int m)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    const int lane = threadIdx.x & 63;
    const int a = (int)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (a > T) return;
    const int64_t base = at(p, traj, m, s, 0);
    const double *__restrict__ gM = p.gamma.M + base, *__restrict__ gZ = p.gamma.Z + base;
    double best = neg_inf(), z = 0.0;
    if (a >= 1 && a < T) {
        const double *__restrict__ W = td.W + (int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) - a;   // entry b at W[b]
        for (int b = a + 1 + lane; b <= T; b += 64) {
            if (!(gZ[b] > 0.0)) continue;
            const double t = gM[b] + W[b];      // NaN compares false
            if (t > best) best = t;
        }
        best = wave_max(best);
        if (best > neg_inf()) {
            for (int b = a + 1 + lane; b <= T; b += 64) {
                const double gz = gZ[b];
                if (!(gz > 0.0)) continue;
                const double w = W[b];
                if (w != w) continue;
                z += gz * exp(gM[b] + w - best);
            }
            z = wave_sum(z);
        }
    }
    if (lane == 0) {
        p.beta.M[base + a] = best;
        p.beta.Z[base + a] = z;
    }
}

// gamma_m(b, s) from beta_{m-1}(b, s'') over the s'' with transitions[s][s'']
__global__ void __launch_bounds__(kThreads) segdp_bmix_kernel(SegdpParams p, int m)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const int b = (int)(blockIdx.x * kThreads + threadIdx.x);
    const int T = p.trajs[traj].T;
    if (b > T) return;
    const int S = p.S;
    double best = neg_inf();
    for (int q = 0; q < S; ++q) {
        if (!p.tr[s * S + q]) continue;
        const int64_t i = at(p, traj, m - 1, q, b);
        if (p.beta.Z[i] > 0.0) best = fmax(best, p.beta.M[i]);
    }
    double z = 0.0;
    if (best > neg_inf()) {
        for (int q = 0; q < S; ++q) {
            if (!p.tr[s * S + q]) continue;
            const int64_t i = at(p, traj, m - 1, q, b);
            const double zq = p.beta.Z[i];
            if (zq > 0.0) z += zq * exp(p.beta.M[i] - best);
        }
    }
    const int64_t o = at(p, traj, m, s, b);
    p.gamma.M[o] = best;
    p.gamma.Z[o] = z;
}

// the MAP profile of every k: from the smallest final state of the largest A_k(T, .) back along the pointers
__global__ void __launch_bounds__(kThreads) segdp_backtrack_kernel(SegdpParams p)
{
    const int r = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (r >= p.n_traj * p.K) return;
    const int traj = r / p.K, k = r - traj * p.K;
    const int T = p.trajs[traj].T, S = p.S, K = p.K;
    int32_t *__restrict__ ss = p.map_seg_start + (int64_t)r * K, *__restrict__ sv = p.map_seg_state + (int64_t)r * K;
    int s = -1;
    double best = neg_inf();
    for (int q = 0; q < S; ++q) {
        const int64_t i = at(p, traj, k, q, T);
        double *__restrict__ fin = p.fin + ((int64_t)r * S + q) * 5;
        fin[0] = p.A.M[i], fin[1] = p.A.Z[i], fin[2] = p.A.R[i], fin[3] = p.A.ok[i], fin[4] = p.A.bad[i];
        if (p.A.arg[i] < 0) continue;
        if (s < 0 || p.A.M[i] > best) {
            best = p.A.M[i];
            s = q;
        }
    }
    if (s < 0) {
        for (int i = 0; i < K; ++i) ss[i] = -1, sv[i] = -1;
        return;
    }
    for (int i = k + 1; i < K; ++i) ss[i] = T, sv[i] = 0;
    int b = T;
    for (int j = k; j >= 1; --j) {
        const int c = p.A.arg[at(p, traj, j, s, b)];
        ss[j] = c;
        sv[j] = s;
        s = p.alpha.arg[at(p, traj, j, s, c)];
        b = c;
    }
    ss[0] = 0;
    sv[0] = s;
}

// the largest log-likelihood of the profiles of k switches: the scale of the marginals
__device__ __forceinline__ double segdp_top(const SegdpParams &p, int traj, int k, int T)
{
    double top = neg_inf();
    for (int q = 0; q < p.S; ++q) {
        const int64_t i = at(p, traj, k, q, T);
        if (p.A.Z[i] > 0.0) top = fmax(top, p.A.M[i]);
    }
    return top;
}

__global__ void __launch_bounds__(kThreads) segdp_cover_kernel(SegdpParams p)
{
    const int traj = blockIdx.z;
    const int k = (int)blockIdx.y / p.S, s = (int)blockIdx.y - k * p.S;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const int t = tile * kSegdpTile + lane, b = t + 1;
    if (tile * kSegdpTile >= T) return;     // the whole wave
    const double top = segdp_top(p, traj, k, T);
    const double nan = quiet_nan();
    const bool mine = b <= T;
    const double *__restrict__ W = td.W + (int64_t)s * td.w_per_state;
    double *__restrict__ row_tot = p.row_tot + ((((int64_t)traj * p.K + k) * p.S + s) * p.ntile + tile) * p.Tm;
    double acc = 0.0;
    const int a_end = min(tile * kSegdpTile + kSegdpTile, T);   // rows a < a_end cover a frame of the tile
    if (top > neg_inf()) {
        for (int a = 0; a < a_end; ++a) {
            double qv = 0.0;
            if (a == 0) {
                if (mine) {
                    const int64_t g = at(p, traj, k, s, b);
                    const double f = td.F[(int64_t)s * (T + 1) + b], gz = p.gamma.Z[g];
                    if (f == f && gz > 0.0) qv = gz * exp(f + p.gamma.M[g] - top);
                }
            } else {
                const double w = mine && b > a ? W[gauss_wrow(T, a - 1) + (b - a)] : nan;
                const int jmax = min(k, a);
                for (int j = 1; j <= jmax; ++j) {
                    const int64_t ia = at(p, traj, j, s, a);
                    const double az = p.alpha.Z[ia];
                    if (!(az > 0.0)) continue;
                    const double am = p.alpha.M[ia];
                    if (w == w) {
                        const int64_t g = at(p, traj, k - j, s, b);
                        const double gz = p.gamma.Z[g];
                        if (gz > 0.0) qv += az * gz * exp(am + w + p.gamma.M[g] - top);
                    }
                }
            }
            qv = wave_scan_down(qv, lane);
            if (t >= a) acc += qv;
            if (lane == 0) row_tot[a] = qv;
        }
    }
    if (mine) p.cover[at(p, traj, k, s, t)] = acc;
}

// post from cover and the row totals (wave_carry): one wave per (k, s, tile)
__global__ void __launch_bounds__(kThreads) segdp_carry_kernel(SegdpParams p)
{
    const int traj = blockIdx.z;
    const int k = (int)blockIdx.y / p.S, s = (int)blockIdx.y - k * p.S;
    const int T = p.trajs[traj].T;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (tile * kSegdpTile >= T) return;
    const double *__restrict__ row_tot = p.row_tot + (((int64_t)traj * p.K + k) * p.S + s) * p.ntile * p.Tm;
    const int64_t row = at(p, traj, k, s, 0);
    wave_carry(row_tot, p.cover + row, p.post + row, T, p.Tm, tile, segdp_top(p, traj, k, T) > neg_inf(), lane);
}

} // namespace

int launch_segdp_init(const SegdpParams &p, bool backward, void *stream)
{
    const dim3 grid((unsigned)((p.ld + kThreads - 1) / kThreads), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdp_init_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p, backward ? 1 : 0);
    return launched();
}

int launch_segdp_mix(const SegdpParams &p, int j, void *stream)
{
    const dim3 grid((unsigned)((p.ld + kThreads - 1) / kThreads), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdp_mix_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p, j);
    return launched();
}

int launch_segdp_level(const SegdpParams &p, int j, void *stream)
{
    const dim3 grid((unsigned)((p.ld + kSegdpTile - 1) / kSegdpTile), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdp_level_kernel, grid, dim3(kSegdpSlices * 64), 0, (hipStream_t)stream, p, j);
    return launched();
}

int launch_segdp_blevel(const SegdpParams &p, int m, void *stream)
{
    const int rows = kThreads / 64;
    const dim3 grid((unsigned)((p.ld + rows - 1) / rows), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdp_blevel_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p, m);
    return launched();
}

int launch_segdp_bmix(const SegdpParams &p, int m, void *stream)
{
    const dim3 grid((unsigned)((p.ld + kThreads - 1) / kThreads), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdp_bmix_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p, m);
    return launched();
}

int launch_segdp_backtrack(const SegdpParams &p, void *stream)
{
    const int n = p.n_traj * p.K;
    hipLaunchKernelGGL(segdp_backtrack_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, p);
    return launched();
}

int launch_segdp_cover(const SegdpParams &p, void *stream)
{
    const int waves = kThreads / 64;
    const dim3 grid((unsigned)((p.ntile + waves - 1) / waves), (unsigned)(p.K * p.S), (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdp_cover_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    return launched();
}

int launch_segdp_carry(const SegdpParams &p, void *stream)
{
    const int waves = kThreads / 64;
    const dim3 grid((unsigned)((p.ntile + waves - 1) / waves), (unsigned)(p.K * p.S), (unsigned)p.n_traj);
    hipLaunchKernelGGL(segdp_carry_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    return launched();
}

} // namespace bild
