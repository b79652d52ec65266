// Gradient of the exact evidence of GenericGaussianModel (include/bild_amd.h, "evidence sensitivities"; DESIGN.md section
// 20): the refusals, the chunks of whole trajectories, the segment recursion's launches and its formulas on the last column
// of the forward table (gauss_segdp.h: the functions gauss_segdp.cpp calls, so that logev is the same number), the weight
// table and the weighted tangent jobs (gauss_segtangent.h).  Kernels: gauss_segsens.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_segsens.h"
#include "gauss_segtangent.h"
#include "gauss_windows.h"

extern "C" int bild_gauss_segment_sensitivities(const bild_gauss_model *m, const bild_gauss_trajset *ts, const double *x, int k_max,
                                                const uint8_t *transitions, unsigned flags, const double *log_k_prior, int P,
                                                const bild_gauss_derivs *dm, int64_t scratch_bytes, bild_segsens_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    const int S = m->S;
    // (nothing here is padded to a T_max, so no trajectory is too long for it)
    BILD_TRY(segdp_check_call(S, k_max, flags, transitions, scratch_bytes, n_traj, T, std::numeric_limits<int>::max()));
    if (n_traj == 0) return BILD_OK;
    BILD_TRY(gauss_check_args(m, n_traj, T, x, 0, 1, nullptr, nullptr, nullptr, P, dm));
    const int K = k_max + 1;
    if (log_k_prior)
        for (int j = 0; j < n_traj; ++j) {
            bool any = false;
            for (int k = 0; k < K; ++k) {
                const double v = log_k_prior[(size_t)j * K + k];
                if (std::isnan(v) || v == std::numeric_limits<double>::infinity())
                    return fail(BILD_ERR_INVALID, "log_k_prior[%d][%d] is NaN or +inf", j, k);
                any = any || v > -std::numeric_limits<double>::infinity();
            }
            if (!any) return fail(BILD_ERR_INVALID, "log_k_prior of trajectory %d is -inf everywhere", j);
        }
    int Tm = 1;
    for (int j = 0; j < n_traj; ++j) Tm = std::max(Tm, T[j]);
    const bool omit = (flags & BILD_SEGDP_NAN_OMIT) != 0;
    const int ld = Tm + 1;
    const int64_t slot = (int64_t)K * S * ld, om_tri = gauss_w_per_state(Tm), om_slot = (int64_t)S * (om_tri + ld);

    SegTangent tangent;     // (before the frame: asynchronous copies read its vectors)
    tangent.stage(m, n_traj, T, x, P, dm);

    CallFrame call;
    BILD_TRY(call.open(m, ts));
    hipStream_t st = call.st;

    // a trajectory's share of the chunk: the recursion's tables and the weight table
    const int64_t per_traj = slot * (2 * (5 * 8 + 4) + 4 * 8) + om_slot * 8 + (int64_t)K * K * 8 + (int64_t)K * S * 40 + (int64_t)K * 16;
    int chunk = 0;
    BILD_TRY(call.chunk_of(per_traj, scratch_bytes, n_traj, &chunk));

    SegdpParams p{};
    SegsensWeights w{};
    uint8_t *d_tr = nullptr;
    double *d_coef = nullptr, *d_top = nullptr;
    BILD_TRY(call.alloc(&d_tr, (size_t)S * S));
    BILD_TRY(alloc_fwd(call, &p.A, (size_t)chunk * slot));
    BILD_TRY(alloc_fwd(call, &p.alpha, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.map_seg_start, (size_t)chunk * K * K));
    BILD_TRY(call.alloc(&p.map_seg_state, (size_t)chunk * K * K));
    BILD_TRY(call.alloc(&p.fin, (size_t)chunk * K * S * 5));
    BILD_TRY(call.alloc(&p.beta.M, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.beta.Z, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.gamma.M, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.gamma.Z, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&w.omega, (size_t)chunk * om_slot));
    BILD_TRY(call.alloc(&d_coef, (size_t)chunk * K));
    BILD_TRY(call.alloc(&d_top, (size_t)chunk * K));
    HIP_TRY(hipMemcpyAsync(d_tr, transitions, (size_t)S * S, hipMemcpyHostToDevice, st));
    p.tr = d_tr;
    p.slot = slot;
    p.S = S;
    p.K = K;
    p.Tm = Tm;
    p.ld = ld;
    p.ntile = (Tm + kSegdpTile - 1) / kSegdpTile;
    w.coef = d_coef;
    w.top = d_top;
    w.om_slot = om_slot;
    w.om_tri = om_tri;

    BILD_TRY(tangent.upload(call));
    BILD_TRY(tangent.reserve(call, chunk));

    const std::vector<long double> ntraces = trace_counts(S, transitions, K);
    std::vector<double> fin((size_t)chunk * K * S * 5), coef((size_t)chunk * K), top((size_t)chunk * K);
    std::vector<char> is_nan(chunk);
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();

    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        const int nc = std::min(chunk, n_traj - j0);
        p.trajs = call.d_trajs + j0;
        p.n_traj = nc;
        BILD_TRY(segdp_run_forward(p, k_max, st));
        BILD_TRY(segdp_run_backward(p, k_max, st));
        HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * K * S * 5 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        // logev of every k (segdp_evidence), the posterior over k, and the scale of every k's weights
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = T[jt];
            std::vector<double> logev(K), zk(K), lw(K);
            bool bad_traj = false;
            double lmax = ninf;
            for (int k = 0; k < K; ++k) {
                const SegdpEvidence e =
                    segdp_evidence(fin.data() + ((size_t)i * K + k) * S * 5, S, binom_ld(Tj - 1, k) * ntraces[k], omit);
                const double le = e.logev;
                logev[k] = le;
                zk[k] = e.z;
                top[(size_t)i * K + k] = e.top;
                const double lp = log_k_prior ? log_k_prior[(size_t)jt * K + k] : 0.0;
                lw[k] = lp > ninf ? lp + le : ninf;     // a k of prior weight 0 does not count, NaN or not
                if (std::isnan(lw[k])) bad_traj = true;
                else lmax = std::max(lmax, lw[k]);
                if (out->logev) out->logev[(size_t)jt * K + k] = le;
            }
            // pi normalised over k: log sum_k pi_k ev_k = lmax + log sum exp(lw - lmax) - log sum exp(log_k_prior)
            double tot = 0.0, lpmax = ninf, ptot = 0.0;
            for (int k = 0; k < K; ++k) lpmax = std::max(lpmax, log_k_prior ? log_k_prior[(size_t)jt * K + k] : 0.0);
            for (int k = 0; k < K; ++k) ptot += std::exp((log_k_prior ? log_k_prior[(size_t)jt * K + k] : 0.0) - lpmax);
            const bool dead = !bad_traj && lmax == ninf;    // no k of positive prior weight has a profile of positive weight
            if (!bad_traj && !dead)
                for (int k = 0; k < K; ++k) tot += lw[k] > ninf ? std::exp(lw[k] - lmax) : 0.0;
            is_nan[i] = bad_traj || dead;
            for (int k = 0; k < K; ++k) {
                const double kp = bad_traj || dead ? nan : (lw[k] > ninf ? std::exp(lw[k] - lmax) / tot : 0.0);
                if (out->k_post) out->k_post[(size_t)jt * K + k] = kp;
                coef[(size_t)i * K + k] = (kp > 0.0 && zk[k] > 0.0) ? kp / zk[k] : 0.0;
            }
            if (out->log_marginal)
                out->log_marginal[jt] = bad_traj ? nan : dead ? ninf : lmax + std::log(tot) - (lpmax + std::log(ptot));
        }
        HIP_TRY(hipMemcpyAsync(d_coef, coef.data(), (size_t)nc * K * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_top, top.data(), (size_t)nc * K * 8, hipMemcpyHostToDevice, st));
        if (launch_segsens_weight(p, w, st)) return fail(BILD_ERR_HIP, "launch of the weight kernel failed");
        BILD_TRY(tangent.run(call, j0, nc, is_nan.data(), w.omega, om_slot, om_tri, ld, out->exp_logl, out->grad, out->fisher));
    }
    return BILD_OK;
}
