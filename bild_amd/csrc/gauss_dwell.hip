// Kernels of the dwell-time recursion (gauss_dwell.h): plain fp64 vector code on the tables W and F of
// a GenericGaussianModel trajectory set.  Everything is kept in logs, every exponent is non-positive, no atomics: every value
// has one owner and every sum a fixed order that depends on the trajectory alone.
//
//   * dwell_forward_kernel: one workgroup per trajectory, all states, tiles of 64 end frames b (lane = b).
//       part 1, switches c at or left of the tile's start: the waves take c = 1 + q, 1 + q + 8, ...; row c - 1 of W is read
//       coalesced, alpha(c, s) is the same for the whole wave.  A lane keeps a running (m, z) and rescales when a larger
//       term arrives; the waves' pairs meet in LDS and wave 0 merges them in wave order.
//       part 2, the tile's triangle, wave 0 alone: at step c lane c's A(c, .) is complete and goes to every lane by a
//       shuffle, every lane forms alpha(c, .) from it, and the lanes b > c add their term.  The W and prior entries of step
//       c + 1 are loaded before the arithmetic of step c, so the dependent chain waits for no load.
//       The same walk in (max, +) with back-pointers gives the MAP profile, which thread 0 expands at the end.
//   * dwell_backward_kernel: the same tiles, descending.  Part 1: one wave per row a of the tile against gamma(b) right of the
//       tile, lanes stride b, butterfly merges.  Part 2, wave 0: rows a descending, lane = b holds gamma(b, .) in registers,
//       a butterfly over the tile's lanes gives beta(a, .), from which lane a gets its gamma(a, .).
//   * dwell_cover_kernel / dwell_carry_kernel: the statistics, section 18's pattern (the scans and the carry: wave.h) with
//       one exp per (a, b, s).  The weight of a segment [a, b) in state s is Q = exp(alpha(a, s) + omega + W + gamma(b, s) -
//       log evidence); frame t collects Q of every a <= t < b, and Q (b - a - 1) adds up to the expected stays.  Sums of
//       non-negative terms only.
//   * dwell_counts_kernel: the expected jumps, O(S^2 T), and the tiles' stays added in tile order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gauss_dwell.h"
#include "wave.h"

namespace bild {
namespace {

constexpr int kWaves = kDwellWaves;

// (lse_add, lse_merge, lse_value: wave.h)
// log prior weight of a segment [a, b) in state s: the last segment is censored
__device__ __forceinline__ double omega(const DwellParams &p, int s, int a, int b, int T)
{
    return b == T ? p.log_surv[(int64_t)s * p.L + (T - a - 1)] : p.log_dwell[(int64_t)s * p.L + (b - a - 1)];
}

template <int S> __global__ void __launch_bounds__(kWaves * 64) dwell_forward_kernel(DwellParams p)
{
    __shared__ double sh_m[kWaves][64], sh_z[kWaves][64], sh_v[kWaves][64];
    __shared__ int sh_arg[kWaves][64];
    __shared__ int sh_cnt[kWaves];
    const int traj = blockIdx.x;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t base = (int64_t)traj * p.slot;
    double *A = p.A + base, *AV = p.AV + base, *al = p.alpha + base, *alV = p.alphaV + base;
    int32_t *Aarg = p.Aarg + base, *alArg = p.alphaArg + base;
    uint8_t *states = p.map_states + (int64_t)traj * p.Tm;
    for (int t = threadIdx.x; t < p.Tm; t += kWaves * 64) states[t] = 255;

    double jm[S][S];
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) jm[a][b] = p.log_jump[a * S + b];
    int cnt = 0;

    for (int b0 = 0; b0 < T; b0 += kDwellTile) {
        const int b = b0 + 1 + lane;
        const bool mine = b <= T;
        double Sm[S], Sz[S], Sv[S];
        int Sa[S];
        // part 1: the first segment and the switches c <= b0
        for (int s = 0; s < S; ++s) {
            const double *Ws = td.W + (int64_t)s * td.w_per_state;
            double m = neg_inf(), z = 0.0, v = neg_inf();
            int arg = -1;
            if (q == 0 && mine) {
                const double pr = p.log_init[s] + omega(p, s, 0, b, T);
                if (pr > neg_inf()) {
                    const double f = td.F[(int64_t)s * (T + 1) + b];
                    if (f != f) {
                        ++cnt;
                    } else {
                        arg = 0;
                        v = pr + f;
                        lse_add(m, z, v);
                    }
                }
            }
            if (mine) {
                for (int c = 1 + q; c <= b0; c += kWaves) {
                    if (alArg[s * ld + c] < 0) continue;        // the whole wave
                    const double om = omega(p, s, c, b, T);
                    if (!(om > neg_inf())) continue;
                    const double w = Ws[gauss_wrow(T, c - 1) + (b - c)];
                    if (w != w) {
                        ++cnt;
                        continue;
                    }
                    const double o = om + w;
                    lse_add(m, z, al[s * ld + c] + o);
                    const double tv = alV[s * ld + c] + o;
                    if (arg < 0 || tv > v) {
                        v = tv;
                        arg = c;
                    }
                }
            }
            sh_m[q][lane] = m;
            sh_z[q][lane] = z;
            sh_v[q][lane] = v;
            sh_arg[q][lane] = arg;
            __syncthreads();
            if (q == 0) {
                double top = neg_inf();
                v = neg_inf(), arg = -1;
                for (int r = 0; r < kWaves; ++r) {
                    if (sh_z[r][lane] > 0.0) top = fmax(top, sh_m[r][lane]);
                    const double rv = sh_v[r][lane];
                    const int ra = sh_arg[r][lane];
                    if (ra >= 0 && (arg < 0 || rv > v || (rv == v && ra < arg))) {
                        v = rv;
                        arg = ra;
                    }
                }
                z = 0.0;
                for (int r = 0; r < kWaves; ++r) {
                    const double rz = sh_z[r][lane];
                    if (rz > 0.0) z += rz * exp(sh_m[r][lane] - top);
                }
                Sm[s] = top, Sz[s] = z, Sv[s] = v, Sa[s] = arg;
            }
            __syncthreads();
        }
        // part 2: the tile's own switches, c = b0 + 1 + lc
        if (q == 0) {
            const int nstep = min(kDwellTile, T - 1 - b0);      // switches c < T only
            double wn[S], on[S];
            for (int s = 0; s < S; ++s) {
                const int c = b0 + 1;
                const bool use = mine && b > c && nstep > 0;
                wn[s] = use ? td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, c - 1) + (b - c)] : 0.0;
                on[s] = use ? omega(p, s, c, b, T) : neg_inf();
            }
            for (int lc = 0; lc < nstep; ++lc) {
                const int c = b0 + 1 + lc;
                double wc[S], oc[S];
                for (int s = 0; s < S; ++s) {
                    wc[s] = wn[s], oc[s] = on[s];
                    const bool use = mine && b > c + 1 && lc + 1 < nstep;
                    wn[s] = use ? td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, c) + (b - c - 1)] : 0.0;
                    on[s] = use ? omega(p, s, c + 1, b, T) : neg_inf();
                }
                double Ac[S], Vc[S];
                bool Rc[S];
                for (int s = 0; s < S; ++s) {
                    Ac[s] = lse_value(__shfl(Sm[s], lc, 64), __shfl(Sz[s], lc, 64));
                    Vc[s] = __shfl(Sv[s], lc, 64);
                    Rc[s] = __shfl(Sa[s], lc, 64) >= 0;
                }
                if (lane == lc)
                    for (int s = 0; s < S; ++s) A[s * ld + c] = Ac[s], AV[s * ld + c] = Vc[s], Aarg[s * ld + c] = Sa[s];
                for (int s = 0; s < S; ++s) {
                    double top = neg_inf(), av = neg_inf();
                    int aa = -1;
                    for (int r = 0; r < S; ++r) {
                        top = fmax(top, Ac[r] + jm[r][s]);
                        if (Rc[r] && jm[r][s] > neg_inf()) {
                            const double t = Vc[r] + jm[r][s];
                            if (aa < 0 || t > av) {
                                av = t;
                                aa = r;
                            }
                        }
                    }
                    double zz = 0.0;
                    if (top > neg_inf())
                        for (int r = 0; r < S; ++r) {
                            const double t = Ac[r] + jm[r][s];
                            if (t > neg_inf()) zz += exp(t - top);
                        }
                    const double as = lse_value(top, zz);
                    if (lane == lc) al[s * ld + c] = as, alV[s * ld + c] = av, alArg[s * ld + c] = aa;
                    if (!(mine && b > c && aa >= 0 && oc[s] > neg_inf())) continue;
                    if (wc[s] != wc[s]) {
                        ++cnt;
                        continue;
                    }
                    const double o = oc[s] + wc[s];
                    lse_add(Sm[s], Sz[s], as + o);
                    const double tv = av + o;
                    if (Sa[s] < 0 || tv > Sv[s]) {
                        Sv[s] = tv;
                        Sa[s] = c;
                    }
                }
            }
            // (frames the steps above did not publish: b = T, and a tile of one frame)
            if (mine && b > b0 + nstep)
                for (int s = 0; s < S; ++s)
                    A[s * ld + b] = lse_value(Sm[s], Sz[s]), AV[s * ld + b] = Sv[s], Aarg[s * ld + b] = Sa[s];
        }
        __syncthreads();    // the tile's tables are in memory before the next tile reads them
    }

    cnt = wave_sum(cnt);
    if (lane == 0) sh_cnt[q] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long total = 0;
    for (int r = 0; r < kWaves; ++r) total += sh_cnt[r];
    p.n_nan[traj] = total;
    double top = neg_inf(), zz = 0.0, best = neg_inf();
    int s = -1;
    for (int r = 0; r < S; ++r) {
        top = fmax(top, A[r * ld + T]);
        if (Aarg[r * ld + T] >= 0 && (s < 0 || AV[r * ld + T] > best)) {
            best = AV[r * ld + T];
            s = r;
        }
    }
    if (top > neg_inf())
        for (int r = 0; r < S; ++r)
            if (A[r * ld + T] > neg_inf()) zz += exp(A[r * ld + T] - top);
    p.fin[2 * traj] = lse_value(top, zz);
    p.fin[2 * traj + 1] = s < 0 ? quiet_nan() : best;
    if (s < 0) return;
    for (int b = T;;) {
        const int c = Aarg[s * ld + b];
        for (int t = c; t < b; ++t) states[t] = (uint8_t)s;
        if (c == 0) break;
        s = alArg[s * ld + c];
        b = c;
    }
}

template <int S> __global__ void __launch_bounds__(kWaves * 64) dwell_backward_kernel(DwellParams p)
{
    __shared__ double sh_m[S][64], sh_z[S][64];
    const int traj = blockIdx.x;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld;
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t base = (int64_t)traj * p.slot;
    double *beta = p.beta + base, *gamma = p.gamma + base;
    double jm[S][S];
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) jm[a][b] = p.log_jump[a * S + b];
    if (threadIdx.x < S) gamma[threadIdx.x * ld + T] = 0.0;
    __syncthreads();

    for (int b0 = (T - 1) / kDwellTile * kDwellTile; b0 >= 0; b0 -= kDwellTile) {
        // part 1: rows of the tile against the end frames right of it
        for (int r = q; r < kDwellTile; r += kWaves) {
            const int a = b0 + 1 + r;
            for (int s = 0; s < S; ++s) {
                double m = neg_inf(), z = 0.0;
                if (a < T) {
                    const double *Wr = td.W + (int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) - a;     // entry b at Wr[b]
                    for (int b = b0 + kDwellTile + 1 + lane; b <= T; b += 64) {
                        const double g = gamma[s * ld + b];
                        if (!(g > neg_inf())) continue;
                        const double om = omega(p, s, a, b, T);
                        if (!(om > neg_inf())) continue;
                        const double w = Wr[b];
                        if (w != w) continue;
                        lse_add(m, z, om + w + g);
                    }
                }
                for (int off = 32; off >= 1; off >>= 1) lse_merge(m, z, __shfl_xor(m, off, 64), __shfl_xor(z, off, 64));
                if (lane == 0) sh_m[s][r] = m, sh_z[s][r] = z;
            }
        }
        __syncthreads();
        // part 2: the tile's triangle, rows descending; lane = b keeps gamma(b, .)
        if (q == 0) {
            const int f = b0 + 1 + lane;
            const bool mine = f <= T;
            double g[S], bt[S];
            for (int s = 0; s < S; ++s) g[s] = f == T ? 0.0 : neg_inf(), bt[s] = neg_inf();
            for (int la = min(b0 + kDwellTile, T - 1) - b0 - 1; la >= 0; --la) {
                const int a = b0 + 1 + la;
                double bc[S];
                for (int s = 0; s < S; ++s) {
                    double t = neg_inf();
                    if (mine && f > a && g[s] > neg_inf()) {
                        const double om = omega(p, s, a, f, T);
                        const double w = td.W[(int64_t)s * td.w_per_state + gauss_wrow(T, a - 1) + (f - a)];
                        if (om > neg_inf() && w == w) t = om + w + g[s];
                    }
                    double m = wave_max(t);
                    double z = wave_sum(t > neg_inf() ? exp(t - m) : 0.0);
                    lse_merge(m, z, sh_m[s][la], sh_z[s][la]);
                    bc[s] = lse_value(m, z);
                }
                for (int s = 0; s < S; ++s) {
                    double top = neg_inf(), zz = 0.0;
                    for (int r = 0; r < S; ++r) top = fmax(top, jm[s][r] + bc[r]);
                    if (top > neg_inf())
                        for (int r = 0; r < S; ++r) {
                            const double t = jm[s][r] + bc[r];
                            if (t > neg_inf()) zz += exp(t - top);
                        }
                    if (lane == la) g[s] = lse_value(top, zz), bt[s] = bc[s];
                }
            }
            if (mine && f < T)
                for (int s = 0; s < S; ++s) beta[s * ld + f] = bt[s], gamma[s * ld + f] = g[s];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kDwellThreads) dwell_cover_kernel(DwellParams p)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const GaussTraj td = p.trajs[traj];
    const int T = td.T, ld = p.ld;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * (kDwellThreads / 64) + (threadIdx.x >> 6);
    const int t = tile * kDwellTile + lane, b = t + 1;
    if (tile * kDwellTile >= T) return;     // the whole wave
    const double logev = p.fin[2 * traj];
    const bool mine = b <= T;
    const int64_t base = (int64_t)traj * p.slot + (int64_t)s * ld;
    const double *__restrict__ W = td.W + (int64_t)s * td.w_per_state;
    const double *__restrict__ al = p.alpha + base;
    double *__restrict__ row_tot = p.row_tot + (((int64_t)traj * p.S + s) * p.ntile + tile) * p.Tm;
    const double g = mine ? p.gamma[base + b] : neg_inf();
    double acc = 0.0, stay = 0.0;
    const int a_end = min(tile * kDwellTile + kDwellTile, T);   // rows a < a_end cover a frame of the tile
    if (logev > neg_inf()) {
        for (int a = 0; a < a_end; ++a) {
            double qv = 0.0;
            const double head = a == 0 ? p.log_init[s] : al[a];
            if (head > neg_inf() && mine && b > a && g > neg_inf()) {
                const double om = omega(p, s, a, b, T);
                const double w = a == 0 ? td.F[(int64_t)s * (T + 1) + b] : W[gauss_wrow(T, a - 1) + (b - a)];
                if (om > neg_inf() && w == w) qv = exp(fmin(head + om + w + g - logev, 0.0));
            }
            stay += qv * (double)(b - a - 1);
            qv = wave_scan_down(qv, lane);
            if (t >= a) acc += qv;
            if (lane == 0) row_tot[a] = qv;
        }
    }
    if (mine) p.cover[base + t] = acc;
    stay = wave_sum(stay);
    if (lane == 0) p.stay_part[((int64_t)traj * p.S + s) * p.ntile + tile] = stay;
}

// post from cover and the row totals (wave_carry): one wave per (s, tile)
__global__ void __launch_bounds__(kDwellThreads) dwell_carry_kernel(DwellParams p)
{
    const int traj = blockIdx.z, s = blockIdx.y;
    const int T = p.trajs[traj].T;
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x * (kDwellThreads / 64) + (threadIdx.x >> 6);
    if (tile * kDwellTile >= T) return;
    const double *__restrict__ row_tot = p.row_tot + ((int64_t)traj * p.S + s) * p.ntile * p.Tm;
    const int64_t base = (int64_t)traj * p.slot + (int64_t)s * p.ld;
    wave_carry(row_tot, p.cover + base, p.post + base, T, p.Tm, tile, p.fin[2 * traj] > neg_inf(), lane);
}

// expected jumps s' -> s: sum_c exp(A(c, s') + log_jump[s'][s] + beta(c, s) - log evidence); one wave per trajectory
__global__ void __launch_bounds__(64) dwell_counts_kernel(DwellParams p)
{
    const int traj = blockIdx.x, lane = threadIdx.x, S = p.S, ld = p.ld;
    const int T = p.trajs[traj].T;
    const int64_t base = (int64_t)traj * p.slot;
    const double logev = p.fin[2 * traj];
    const bool live = logev > neg_inf();
    for (int r = 0; r < S; ++r)
        for (int s = 0; s < S; ++s) {
            const double j = p.log_jump[r * S + s];
            double acc = 0.0;
            if (live && j > neg_inf())
                for (int c = 1 + lane; c < T; c += 64) {
                    const double a = p.A[base + (int64_t)r * ld + c], bt = p.beta[base + (int64_t)s * ld + c];
                    if (a > neg_inf() && bt > neg_inf()) acc += exp(fmin(a + j + bt - logev, 0.0));
                }
            acc = wave_sum(acc);
            if (lane == 0) p.jumps[((int64_t)traj * S + r) * S + s] = acc;
        }
    if (lane != 0 || !p.stay_part) return;      // (no stay_part: the jumps alone, gauss_dwelllen.cpp)
    const int ntile = (T + kDwellTile - 1) / kDwellTile;
    for (int s = 0; s < S; ++s) {
        double acc = 0.0;
        for (int i = 0; i < ntile; ++i) acc += p.stay_part[((int64_t)traj * S + s) * p.ntile + i];
        p.stay[(int64_t)traj * S + s] = acc;
    }
}

} // namespace

int launch_dwell_forward(const DwellParams &p, void *stream)
{
    const dim3 grid((unsigned)p.n_traj), block(kWaves * 64);
    switch (p.S) {
    case 1: hipLaunchKernelGGL(dwell_forward_kernel<1>, grid, block, 0, (hipStream_t)stream, p); break;
    case 2: hipLaunchKernelGGL(dwell_forward_kernel<2>, grid, block, 0, (hipStream_t)stream, p); break;
    case 3: hipLaunchKernelGGL(dwell_forward_kernel<3>, grid, block, 0, (hipStream_t)stream, p); break;
    case 4: hipLaunchKernelGGL(dwell_forward_kernel<4>, grid, block, 0, (hipStream_t)stream, p); break;
    default: return 1;
    }
    return launched();
}

int launch_dwell_backward(const DwellParams &p, void *stream)
{
    const dim3 grid((unsigned)p.n_traj), block(kWaves * 64);
    switch (p.S) {
    case 1: hipLaunchKernelGGL(dwell_backward_kernel<1>, grid, block, 0, (hipStream_t)stream, p); break;
    case 2: hipLaunchKernelGGL(dwell_backward_kernel<2>, grid, block, 0, (hipStream_t)stream, p); break;
    case 3: hipLaunchKernelGGL(dwell_backward_kernel<3>, grid, block, 0, (hipStream_t)stream, p); break;
    case 4: hipLaunchKernelGGL(dwell_backward_kernel<4>, grid, block, 0, (hipStream_t)stream, p); break;
    default: return 1;
    }
    return launched();
}

int launch_dwell_cover(const DwellParams &p, void *stream)
{
    const int waves = kDwellThreads / 64;
    const dim3 grid((unsigned)((p.ntile + waves - 1) / waves), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(dwell_cover_kernel, grid, dim3(kDwellThreads), 0, (hipStream_t)stream, p);
    return launched();
}

int launch_dwell_carry(const DwellParams &p, void *stream)
{
    const int waves = kDwellThreads / 64;
    const dim3 grid((unsigned)((p.ntile + waves - 1) / waves), (unsigned)p.S, (unsigned)p.n_traj);
    hipLaunchKernelGGL(dwell_carry_kernel, grid, dim3(kDwellThreads), 0, (hipStream_t)stream, p);
    return launched();
}

int launch_dwell_counts(const DwellParams &p, void *stream)
{
    hipLaunchKernelGGL(dwell_counts_kernel, dim3((unsigned)p.n_traj), dim3(64), 0, (hipStream_t)stream, p);
    return launched();
}

} // namespace bild
