// Forward sensitivities of the Kalman-filter log-likelihood (bild_logl_sensitivities: sens.cpp).
//
// One task = (candidate r, covariance chain e), geometry of kalman_kernel (kalman.hip): L lanes (8, 16 or 32), lane i owns
// row i of the covariance C (registers) and of each of its P tangents dC_p (the task's LDS slice, element (i, c) at
// c L + i: lane i touches only its own row, and the lanes of one access hit consecutive doubles), in the modal basis of
// the state in force.  Rows of the tangents in registers as well do not fit: at L = 16 and P = 3 they spill.  At L = 32
// even the tangents in LDS spill (the row of C and the accumulator of a basis change are 128 VGPRs already), so 17 to
// 32 effective modes run P = 0 only (kSensMaxP32; sens.cpp refuses more).  Sums over modes are __shfl_xor butterflies (every lane ends with the same bits), vectors every lane
// needs whole (c, dc_p, lam, dlam_p, w) go through the task's LDS slice.  The filter runs forward only and keeps no per-frame record: per
// observed frame and dimension k of the chain, with S the innovation variance and e the innovation,
//     term   = -(e^2 / S + log S + log 2 pi) / 2
//     dterm  = -e de / S + e^2 dS / (2 S^2) - dS / (2 S)
//     Fisher += dS_p dS_q / (2 S^2) + de_p de_q / S
// and the task writes its sums alone (DESIGN.md section 14 has the recursion of the tangents).  A switch of state
// changes the basis of C, M and of every tangent through Q_new^T Q_old, which does not depend on the parameters (the host
// refuses derivatives that are not diagonal in each state's basis).  A task's sums depend on the model, its trajectory,
// its profile and the derivatives only.
#include <hip/hip_runtime.h>

#include "kalman_dev.h"
#include "sens.h"

namespace bild {
namespace {

// X <- A X A^T (conj_sym) for a symmetric X that lives in LDS, element (i, c) at X[c L + i]: first Z = A X into the
// task's L x (L + 1) block, then A Z^T back into X.  Only an accumulator row is held in registers.
template <int L> __device__ void conj_sym_lds(double *X, const double *__restrict__ Q, bool tr, double *buf, int i)
{
    double acc[L];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        wave_lds_fence();
#pragma unroll
        for (int c = 0; c < L; ++c) acc[c] = 0.0;
        for (int a = 0; a < L; ++a) {
            const double ai = tr ? Q[a * L + i] : Q[i * L + a];
#pragma unroll
            for (int c = 0; c < L; ++c) acc[c] = fma(ai, pass == 0 ? X[c * L + a] : buf[c * (L + 1) + a], acc[c]);
        }
        wave_lds_fence();
#pragma unroll
        for (int c = 0; c < L; ++c) {
            if (pass == 0) buf[i * (L + 1) + c] = acc[c];
            else X[c * L + i] = acc[c];
        }
    }
}

template <int L, int P> __global__ void __launch_bounds__(64) sens_kernel(const SensParams p)
{
    constexpr int TPB = 64 / L;                                // tasks per workgroup
    constexpr int SLOT = L * (L + 1) + (3 + 2 * P) * L + P * L * L; // basis-change block, lam, w, c, dlam_p, dc_p, dC_p
    constexpr int NF = P * (P + 1) / 2;
    __shared__ double lds[TPB * SLOT];
    const int lane = threadIdx.x, i = lane % L, slot = lane / L;
    const int64_t task = (int64_t)blockIdx.x * TPB + slot;
    if (task >= p.n * p.dstar_max) return;
    const int64_t r = task / p.dstar_max;
    const int e = (int)(task - r * p.dstar_max);
    const int j = p.traj_id ? p.traj_id[r] : 0;
    const TrajDesc &td = p.trajs[j];
    if (e >= td.dstar) return;
    const int T = td.T, nd = td.ndims[e], d = p.d, S_ = p.S;
    const double s2 = td.s2[e];
    double ds2[P > 0 ? P : 1];
#pragma unroll
    for (int q = 0; q < P; ++q) ds2[q] = p.ds2[((size_t)j * kChains + e) * kSensMaxP + q];
    int dk[kDMax];
#pragma unroll
    for (int k = 0; k < kDMax; ++k) dk[k] = k < nd ? td.dims[e][k] : 0;
    double *buf = lds + slot * SLOT, *lv = buf + L * (L + 1), *wv = lv + L, *xv = wv + L, *dlv = xv + L, *dxv = dlv + P * L;
    double *dC = dxv + P * L; // dC_p(i, c) at dC[(p L + c) L + i]
    const int32_t *seg_start = p.seg_start + r * p.K1, *seg_state = p.seg_state + r * p.K1;

    int s = seg_state[0];
    double lam_i, sig_i, wq_i, dlam_i[P > 0 ? P : 1], dsig_i[P > 0 ? P : 1];
    auto load_state = [&](int st) {
        lam_i = p.lam[st * L + i];
        sig_i = p.sig[st * L + i];
        wq_i = p.wq[st * L + i];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            dlam_i[q] = p.dlam[((size_t)q * S_ + st) * L + i];
            dsig_i[q] = p.dsig[((size_t)q * S_ + st) * L + i];
        }
        wave_lds_fence();
        lv[i] = lam_i;
        wv[i] = wq_i;
#pragma unroll
        for (int q = 0; q < P; ++q) dlv[q * L + i] = dlam_i[q];
        wave_lds_fence();
    };
    load_state(s);

    double C[L], M[kDMax], dM[P > 0 ? P : 1][kDMax];
#pragma unroll
    for (int c = 0; c < L; ++c) C[c] = p.C0[((size_t)s * L + i) * L + c];
#pragma unroll
    for (int k = 0; k < kDMax; ++k) M[k] = k < nd ? p.M0[((size_t)s * L + i) * d + dk[k]] : 0.0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
#pragma unroll
        for (int c = 0; c < L; ++c) dC[(q * L + c) * L + i] = p.dC0[(((size_t)q * S_ + s) * L + i) * L + c];
#pragma unroll
        for (int k = 0; k < kDMax; ++k) dM[q][k] = k < nd ? p.dM0[(((size_t)q * S_ + s) * L + i) * d + dk[k]] : 0.0;
    }
    double ll = 0.0, g[P > 0 ? P : 1], F[NF > 0 ? NF : 1];
#pragma unroll
    for (int q = 0; q < P; ++q) g[q] = 0.0;
#pragma unroll
    for (int q = 0; q < NF; ++q) F[q] = 0.0;
    int seg = 0;
    for (int t = 0; t < T; ++t) {
        if (t > 0) {
            while (seg + 1 < p.K1 && seg_start[seg + 1] <= t) ++seg;
            const int sn = seg_state[seg];
            if (sn != s) { // x <- Q_sn^T Q_s x, for C, M and every tangent
                const double *Qs = p.Q + (size_t)s * L * L, *Qn = p.Q + (size_t)sn * L * L;
                conj_sym<L>(C, Qs, false, buf, i);
                conj_sym<L>(C, Qn, true, buf, i);
                apply_vec<L>(M, Qs, false, buf, i);
                apply_vec<L>(M, Qn, true, buf, i);
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    conj_sym_lds<L>(dC + q * L * L, Qs, false, buf, i);
                    conj_sym_lds<L>(dC + q * L * L, Qn, true, buf, i);
                    apply_vec<L>(dM[q], Qs, false, buf, i);
                    apply_vec<L>(dM[q], Qn, true, buf, i);
                }
                s = sn;
                load_state(s);
            }
            // predict: tangents first, they read the old C and M
#pragma unroll
            for (int q = 0; q < P; ++q) {
#pragma unroll
                for (int k = 0; k < kDMax; ++k) {
                    const double dg = (p.has_dG && k < nd) ? p.dG[(((size_t)q * S_ + s) * L + i) * d + dk[k]] : 0.0;
                    dM[q][k] = fma(dlam_i[q], M[k], fma(lam_i, dM[q][k], dg));
                }
#pragma unroll
                for (int c = 0; c < L; ++c) {
                    double &x = dC[(q * L + c) * L + i];
                    x = fma(fma(dlam_i[q], lv[c], lam_i * dlv[q * L + c]), C[c], fma(lam_i * lv[c], x, c == i ? dsig_i[q] : 0.0));
                }
            }
#pragma unroll
            for (int k = 0; k < kDMax; ++k)
                if (k < nd) M[k] = fma(lam_i, M[k], p.G[((size_t)s * L + i) * d + dk[k]]);
#pragma unroll
            for (int c = 0; c < L; ++c) C[c] = fma(lam_i * lv[c], C[c], c == i ? sig_i : 0.0);
        }
        const double *x = td.x + (size_t)t * d;
        const bool obs = !isnan(x[dk[0]]);
        if (!obs) continue; // predicted, not updated (the condition is the same on every lane of the task)
        double cw = 0.0, dcw[P > 0 ? P : 1];
#pragma unroll
        for (int c = 0; c < L; ++c) cw = fma(C[c], wv[c], cw);
#pragma unroll
        for (int q = 0; q < P; ++q) {
            dcw[q] = 0.0;
#pragma unroll
            for (int c = 0; c < L; ++c) dcw[q] = fma(dC[(q * L + c) * L + i], wv[c], dcw[q]);
        }
        const double S = task_sum<L>(wq_i * cw) + s2, invS = 1.0 / S, logS = log(S);
        double dS[P > 0 ? P : 1];
#pragma unroll
        for (int q = 0; q < P; ++q) dS[q] = task_sum<L>(wq_i * dcw[q]) + ds2[q];
        double ev[kDMax], de[P > 0 ? P : 1][kDMax];
#pragma unroll
        for (int k = 0; k < kDMax; ++k) {
            ev[k] = k < nd ? x[dk[k]] - task_sum<L>(wq_i * M[k]) : 0.0;
#pragma unroll
            for (int q = 0; q < P; ++q) de[q][k] = k < nd ? -task_sum<L>(wq_i * dM[q][k]) : 0.0;
        }
        // sums of this frame
#pragma unroll
        for (int k = 0; k < kDMax; ++k) {
            if (k >= nd) continue;
            const double e2 = ev[k] * ev[k];
            ll += -0.5 * (e2 * invS + logS + kLog2Pi);
#pragma unroll
            for (int q = 0; q < P; ++q) g[q] += -ev[k] * de[q][k] * invS + 0.5 * dS[q] * invS * (e2 * invS - 1.0);
            int f = 0;
#pragma unroll
            for (int a = 0; a < P; ++a)
#pragma unroll
                for (int b = a; b < P; ++b, ++f) F[f] += 0.5 * dS[a] * dS[b] * invS * invS + de[a][k] * de[b][k] * invS;
        }
        // update: K = c / S, dK = dc / S - c dS / S^2
        const double Ki = cw * invS;
        double dKi[P > 0 ? P : 1];
#pragma unroll
        for (int q = 0; q < P; ++q) dKi[q] = (dcw[q] - cw * dS[q] * invS) * invS;
        wave_lds_fence();
        xv[i] = cw;
#pragma unroll
        for (int q = 0; q < P; ++q) dxv[q * L + i] = dcw[q];
        wave_lds_fence();
#pragma unroll
        for (int q = 0; q < P; ++q) {
#pragma unroll
            for (int c = 0; c < L; ++c) {
                double &x = dC[(q * L + c) * L + i];
                x = fma(-dKi[q], xv[c], fma(-Ki, dxv[q * L + c], x));
            }
#pragma unroll
            for (int k = 0; k < kDMax; ++k) dM[q][k] = fma(dKi[q], ev[k], fma(Ki, de[q][k], dM[q][k]));
        }
#pragma unroll
        for (int c = 0; c < L; ++c) C[c] = fma(-Ki, xv[c], C[c]);
#pragma unroll
        for (int k = 0; k < kDMax; ++k) M[k] = fma(Ki, ev[k], M[k]);
    }
    if (i == 0) {
        double *o = p.out + task * kSensStride;
        o[0] = ll;
#pragma unroll
        for (int q = 0; q < P; ++q) o[1 + q] = g[q];
#pragma unroll
        for (int q = 0; q < NF; ++q) o[1 + P + q] = F[q];
    }
}

template <int L> int launch_l(const SensParams &p, int P, dim3 grid, hipStream_t st)
{
    switch (P) {
    case 0: hipLaunchKernelGGL((sens_kernel<L, 0>), grid, dim3(64), 0, st, p); return 0;
    default: break;
    }
    if constexpr (L < 32) {
        switch (P) {
        case 1: hipLaunchKernelGGL((sens_kernel<L, 1>), grid, dim3(64), 0, st, p); return 0;
        case 2: hipLaunchKernelGGL((sens_kernel<L, 2>), grid, dim3(64), 0, st, p); return 0;
        case 3: hipLaunchKernelGGL((sens_kernel<L, 3>), grid, dim3(64), 0, st, p); return 0;
        case 4: hipLaunchKernelGGL((sens_kernel<L, 4>), grid, dim3(64), 0, st, p); return 0;
        default: break;
        }
    }
    return 1;
}

} // namespace

int launch_sens(const SensParams &p, int L, int P, void *stream)
{
    const int64_t tasks = p.n * p.dstar_max;
    if (tasks <= 0) return 0;
    const dim3 grid((unsigned)((tasks + 64 / L - 1) / (64 / L)));
    const hipStream_t st = (hipStream_t)stream;
    int rc = 1;
    switch (L) {
    case 8: rc = launch_l<8>(p, P, grid, st); break;
    case 16: rc = launch_l<16>(p, P, grid, st); break;
    case 32: rc = launch_l<32>(p, P, grid, st); break;
    default: return 1;
    }
    if (rc) return rc;
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace bild
