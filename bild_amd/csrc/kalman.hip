// Kalman filter and smoother of candidate profiles (bild_kalman_segments, bild_kalman_mixture: kalman.cpp).
//
// One task = (candidate r, covariance chain e): the filter of the chain's covariance and of the means of its <= kDMax
// dimensions, in the modal basis of the state in force (B = diag(lam), Sig = diag(sig) there; the model's modal analysis,
// likelihood.h), then the modified Bryson-Frazier (MBF) smoother backwards over the same frames.  A task runs on L lanes
// (8, 16 or 32: the smallest that holds the effective modes), lane i owns row i of the covariance (forward) and of the
// smoother's information matrix Lambda (backward), all in registers; 64 / L tasks share a wavefront and a workgroup of
// one wavefront.  Sums over modes are butterflies of __shfl_xor within the L lanes of the task (every lane ends with the
// same bits); vectors every lane needs whole (C- w, Lambda K, lam, w) go through the task's own LDS slice, ordered by
// wave_lds_fence.  A switch of state changes the basis, x <- Q_new^T Q_old x, through the task's L x (L + 1) LDS block.
//
// Forward, frame t (frame 0 starts from the steady state of its state, t >= 1 is first predicted with the state of t):
//     c = C- w,  S = w.c + s2,  e = x_t - w.M-,  K = c / S,  M = M- + K e,  C = C- - K c^T      (observed frames only)
// and the record of frame t -- c, S, observed, the filtered y-variance, e, the filtered y-mean, the state (DESIGN.md
// section 13) -- goes to an HBM workspace.  Backward, with lambda_{T-1} = 0, Lambda_{T-1} = 0 and u_t = P_t w, which is
// c s2 / S on an observed frame and c on a missing one (P_t w = c - K (w.c) = c (1 - (S - s2) / S)):
//     smoothed y-mean  = w.m_t + u_t.lambda_t,      smoothed y-variance = w.u_t - u_t^T Lambda_t u_t,
//     observed t:  lambda~ = w e / S + lambda - w (K.lambda),
//                  Lambda~ = Lambda - w v^T - v w^T + (K.v + 1 / S) w w^T,   v = Lambda K
//     missing t:   lambda~ = lambda,  Lambda~ = Lambda
//     lambda_{t-1} = diag(lam) lambda~,  Lambda_{t-1} = diag(lam) Lambda~ diag(lam)   (then R^T . R at a switch)
// Nothing of the predicted covariance is inverted.  Each task's results depend on the model, its trajectory and its
// profile only: not on the batch, its order or the chunking.
#include <hip/hip_runtime.h>

#include "kalman.h"
#include "kalman_dev.h"

namespace bild {
namespace {

template <int L> __global__ void __launch_bounds__(64) kalman_kernel(const KalParams p)
{
    constexpr int TPB = 64 / L;                 // tasks per workgroup
    constexpr int SLOT = L * (L + 1) + 3 * L;   // LDS doubles of a task: basis-change block, lam, w, one shared vector
    constexpr int REC = L + 4 + 2 * kDMax;
    __shared__ double lds[TPB * SLOT];
    const int lane = threadIdx.x, i = lane % L, slot = lane / L;
    const int64_t task = (int64_t)blockIdx.x * TPB + slot;
    if (task >= p.n * p.dstar_max) return;
    const int64_t r = task / p.dstar_max;
    const int e = (int)(task - r * p.dstar_max);
    const TrajDesc &td = p.trajs[p.traj_id ? p.traj_id[r] : 0];
    if (e >= td.dstar) return;
    const int T = td.T, nd = td.ndims[e], d = p.d, Tout = p.Tout;
    const double s2 = td.s2[e];
    int dk[kDMax];
#pragma unroll
    for (int k = 0; k < kDMax; ++k) dk[k] = k < nd ? td.dims[e][k] : 0;
    double *buf = lds + slot * SLOT, *lv = buf + L * (L + 1), *wv = lv + L, *xv = wv + L;
    const int32_t *seg_start = p.seg_start + r * p.K1, *seg_state = p.seg_state + r * p.K1;
    double *rec = p.rec + p.rec_off[task];
    const size_t orow = (size_t)r * Tout * d;

    int s = seg_state[0];
    double lam_i, sig_i, wq_i;
    auto load_state = [&](int st) {
        lam_i = p.lam[st * L + i];
        sig_i = p.sig[st * L + i];
        wq_i = p.wq[st * L + i];
        wave_lds_fence();
        lv[i] = lam_i;
        wv[i] = wq_i;
        wave_lds_fence();
    };
    load_state(s);

    // ---- forward: filter, per-frame outputs, records ----
    double C[L], M[kDMax];
#pragma unroll
    for (int c = 0; c < L; ++c) C[c] = p.C0[((size_t)s * L + i) * L + c];
#pragma unroll
    for (int k = 0; k < kDMax; ++k) M[k] = k < nd ? p.M0[((size_t)s * L + i) * d + dk[k]] : 0.0;
    int q = 0;
    for (int t = 0; t < T; ++t) {
        if (t > 0) {
            while (q + 1 < p.K1 && seg_start[q + 1] <= t) ++q;
            const int sn = seg_state[q];
            if (sn != s) { // x <- Q_sn^T Q_s x
                conj_sym<L>(C, p.Q + (size_t)s * L * L, false, buf, i);
                conj_sym<L>(C, p.Q + (size_t)sn * L * L, true, buf, i);
                apply_vec<L>(M, p.Q + (size_t)s * L * L, false, buf, i);
                apply_vec<L>(M, p.Q + (size_t)sn * L * L, true, buf, i);
                s = sn;
                load_state(s);
            }
#pragma unroll
            for (int k = 0; k < kDMax; ++k)
                if (k < nd) M[k] = fma(lam_i, M[k], p.G[((size_t)s * L + i) * d + dk[k]]);
#pragma unroll
            for (int c = 0; c < L; ++c) C[c] = fma(lam_i * lv[c], C[c], c == i ? sig_i : 0.0);
        }
        double cw = 0.0;
#pragma unroll
        for (int c = 0; c < L; ++c) cw = fma(C[c], wv[c], cw);
        const double wCw = task_sum<L>(wq_i * cw);
        const double S = wCw + s2;
        double pm[kDMax], ev[kDMax], fm[kDMax];
        const double *x = td.x + (size_t)t * d;
        const bool obs = !isnan(x[dk[0]]);
#pragma unroll
        for (int k = 0; k < kDMax; ++k) {
            pm[k] = task_sum<L>(wq_i * M[k]);
            ev[k] = obs && k < nd ? x[dk[k]] - pm[k] : 0.0;
            fm[k] = obs ? fma(ev[k], wCw / S, pm[k]) : pm[k];
        }
        const double fv = obs ? wCw * s2 / S : wCw;
        if (obs) {
            const double Ki = cw / S;
            wave_lds_fence();
            xv[i] = cw;
            wave_lds_fence();
#pragma unroll
            for (int c = 0; c < L; ++c) C[c] = fma(-Ki, xv[c], C[c]);
#pragma unroll
            for (int k = 0; k < kDMax; ++k) M[k] = fma(Ki, ev[k], M[k]);
        }
        double *rt = rec + (size_t)t * REC;
        rt[i] = cw;
        for (int j = i; j < REC - L; j += L) {
            rt[L + j] = j == 0 ? S : j == 1 ? (obs ? 1.0 : 0.0) : j == 2 ? fv : j < 2 + 1 + kDMax ? pick(ev, j - 3)
                      : j < 3 + 2 * kDMax ? pick(fm, j - 3 - kDMax) : (double)s;
        }
        if (i < nd) {
            const size_t o = orow + (size_t)t * d + dk[i];
            const double ei = pick(ev, i);
            if (p.out[0]) p.out[0][o] = obs ? -0.5 * (ei * ei / S + log(S) + kLog2Pi) : 0.0;
            if (p.out[1]) p.out[1][o] = pick(pm, i);
            if (p.out[2]) p.out[2][o] = S;
            if (p.out[3]) p.out[3][o] = pick(fm, i);
            if (p.out[4]) p.out[4][o] = fv;
            if (p.out[7]) p.out[7][o] = obs ? ei / sqrt(S) : __builtin_nan("");
        }
    }
    // frames behind the trajectory's end
    for (int t = T + i; t < Tout; t += L)
        for (int k = 0; k < nd; ++k) {
            const size_t o = orow + (size_t)t * d + dk[k];
#pragma unroll
            for (int w = 0; w < kKalOutputs; ++w)
                if (p.out[w]) p.out[w][o] = __builtin_nan("");
        }
    if (!p.out[5] && !p.out[6]) return;

    // ---- backward: MBF smoother ----
    double lam_v[kDMax] = {0.0, 0.0, 0.0};
    double Lam[L];
#pragma unroll
    for (int c = 0; c < L; ++c) Lam[c] = 0.0;
    // the records were written by the lanes of this task (one wavefront, one workgroup): wait for the stores
    __threadfence_block();
    {
        const int sT = (int)rec[(size_t)(T - 1) * REC + L + 3 + 2 * kDMax];
        if (sT != s) {
            s = sT;
            load_state(s);
        }
    }
    for (int t = T - 1; t >= 0; --t) {
        const double *rt = rec + (size_t)t * REC;
        const double cw = rt[i], S = rt[L], fv = rt[L + 2];
        const bool obs = rt[L + 1] != 0.0;
        double ev[kDMax], fm[kDMax];
#pragma unroll
        for (int k = 0; k < kDMax; ++k) {
            ev[k] = rt[L + 3 + k];
            fm[k] = rt[L + 3 + kDMax + k];
        }
        wave_lds_fence();
        xv[i] = cw;
        wave_lds_fence();
        const double scale = obs ? s2 / S : 1.0;
        double Lu = 0.0; // (Lambda u)_i
#pragma unroll
        for (int c = 0; c < L; ++c) Lu = fma(Lam[c], xv[c] * scale, Lu);
        const double uLu = task_sum<L>(cw * scale * Lu);
        double sm[kDMax];
#pragma unroll
        for (int k = 0; k < kDMax; ++k) sm[k] = fm[k] + task_sum<L>(cw * scale * lam_v[k]);
        if (i < nd) {
            const size_t o = orow + (size_t)t * d + dk[i];
            if (p.out[5]) p.out[5][o] = pick(sm, i);
            if (p.out[6]) p.out[6][o] = fv - uLu;
        }
        if (t == 0) break;
        if (obs) {
            const double Ki = cw / S, invS = 1.0 / S;
#pragma unroll
            for (int k = 0; k < kDMax; ++k) {
                const double kl = task_sum<L>(Ki * lam_v[k]);
                lam_v[k] = fma(wq_i, ev[k] / S - kl, lam_v[k]);
            }
            double v = 0.0; // (Lambda K)_i
#pragma unroll
            for (int c = 0; c < L; ++c) v = fma(Lam[c], xv[c] / S, v);
            const double alpha = task_sum<L>(Ki * v) + invS;
            wave_lds_fence();
            xv[i] = v;
            wave_lds_fence();
#pragma unroll
            for (int c = 0; c < L; ++c) Lam[c] = Lam[c] - wq_i * xv[c] - v * wv[c] + (wq_i * wv[c]) * alpha;
        }
#pragma unroll
        for (int k = 0; k < kDMax; ++k) lam_v[k] *= lam_i;
#pragma unroll
        for (int c = 0; c < L; ++c) Lam[c] *= lam_i * lv[c];
        const int sp = (int)rec[(size_t)(t - 1) * REC + L + 3 + 2 * kDMax];
        if (sp != s) { // lambda <- Q_sp^T Q_s lambda  (R^T, R = Q_s^T Q_sp the forward basis change)
            conj_sym<L>(Lam, p.Q + (size_t)s * L * L, false, buf, i);
            conj_sym<L>(Lam, p.Q + (size_t)sp * L * L, true, buf, i);
            apply_vec<L>(lam_v, p.Q + (size_t)s * L * L, false, buf, i);
            apply_vec<L>(lam_v, p.Q + (size_t)sp * L * L, true, buf, i);
            s = sp;
            load_state(s);
        }
    }
}

// mixture, pass 1: one thread per (block, frame, dimension) sums its block's candidates in index order
__global__ void __launch_bounds__(256) mix_block_kernel(const MixParams p)
{
    const int64_t per = (int64_t)p.Tout * p.d;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)p.nblk * per) return;
    const int b = (int)(idx / per);
    const int64_t tk = idx - (int64_t)b * per;
    if (tk / p.d >= p.blk_T[b]) return;
    const double ref = p.ref[(int64_t)p.ref_row[p.blk_traj[b]] * per + tk];
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = p.blk_start[b]; r < p.blk_start[b + 1]; ++r) {
        const double w = p.w[r], dm = p.mean[(int64_t)r * per + tk] - ref;
        s1 = fma(w, dm, s1);
        s2 = fma(w, p.var[(int64_t)r * per + tk], s2);
        s3 = fma(w * dm, dm, s3);
    }
    double *o = p.part + (idx * 3);
    o[0] = s1;
    o[1] = s2;
    o[2] = s3;
}

// mixture, pass 2: one thread per (run of one trajectory's blocks, frame, dimension) adds the blocks in order
__global__ void __launch_bounds__(256) mix_acc_kernel(const MixParams p)
{
    const int64_t per = (int64_t)p.Tout * p.d;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)p.nrun * per) return;
    const int run = (int)(idx / per);
    const int64_t tk = idx - (int64_t)run * per;
    const int b0 = p.run_b0[run], b1 = p.run_b0[run + 1];
    if (tk / p.d >= p.blk_T[b0]) return;
    double *a = p.acc + ((int64_t)p.blk_traj[b0] * per + tk) * 3;
    double s1 = a[0], s2 = a[1], s3 = a[2];
    for (int b = b0; b < b1; ++b) {
        const double *o = p.part + ((int64_t)b * per + tk) * 3;
        s1 += o[0];
        s2 += o[1];
        s3 += o[2];
    }
    a[0] = s1;
    a[1] = s2;
    a[2] = s3;
}

} // namespace

int launch_kalman(const KalParams &p, int L, void *stream)
{
    const int64_t tasks = p.n * p.dstar_max;
    if (tasks <= 0) return 0;
    const dim3 grid((unsigned)((tasks + 64 / L - 1) / (64 / L)));
    switch (L) {
    case 8: hipLaunchKernelGGL(kalman_kernel<8>, grid, dim3(64), 0, (hipStream_t)stream, p); break;
    case 16: hipLaunchKernelGGL(kalman_kernel<16>, grid, dim3(64), 0, (hipStream_t)stream, p); break;
    case 32: hipLaunchKernelGGL(kalman_kernel<32>, grid, dim3(64), 0, (hipStream_t)stream, p); break;
    default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_kalman_mix(const MixParams &p, void *stream)
{
    const int64_t per = (int64_t)p.Tout * p.d;
    if (p.nblk <= 0) return 0;
    hipLaunchKernelGGL(mix_block_kernel, dim3((unsigned)((p.nblk * per + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(mix_acc_kernel, dim3((unsigned)((p.nrun * per + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace bild
