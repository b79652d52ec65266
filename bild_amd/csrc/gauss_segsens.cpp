// Gradient of the exact evidence of GenericGaussianModel (include/bild_amd.h, "evidence sensitivities"; DESIGN.md section
// 20): the forward and backward passes of the segment recursion and its formulas on the last column of the forward table
// through SegdpCall (gauss_segdp.h), as bild_gauss_segment_evidence runs them, so that logev is the same number; the
// posterior over k, the call's own weight table and the weighted tangent jobs (gauss_segtangent.h).  Kernels:
// gauss_segsens.hip.
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
    SegdpCall rec;          // (both before the frame, with the host copies below: asynchronous copies use their vectors)
    SegTangent tangent;
    std::vector<double> coef, top;
    // (nothing here is padded to a T_max, so no trajectory is too long for it)
    BILD_TRY(rec.check(m, ts, k_max, transitions, std::numeric_limits<int>::max(), flags, scratch_bytes, out));
    const int n_traj = rec.n_traj, K = rec.K;
    if (n_traj == 0) return BILD_OK;
    BILD_TRY(gauss_check_args(m, n_traj, rec.T, x, 0, 1, nullptr, nullptr, nullptr, P, dm));
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
    tangent.stage(m, n_traj, rec.T, x, P, dm);

    // the call's own tables: the weights, and the coefficient and scale of every k
    SegsensWeights w{};
    w.om_tri = gauss_w_per_state(rec.Tm);
    w.om_slot = (int64_t)rec.S * (w.om_tri + rec.Tm + 1);

    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kSegdpForward | kSegdpBackward, (w.om_slot + K + K) * 8));
    hipStream_t st = call.st;
    const int chunk = rec.chunk;
    BILD_TRY(call.alloc(&w.omega, (size_t)chunk * w.om_slot));
    double *d_coef = nullptr, *d_top = nullptr;
    BILD_TRY(call.alloc(&d_coef, (size_t)chunk * K));
    BILD_TRY(call.alloc(&d_top, (size_t)chunk * K));
    w.coef = d_coef;
    w.top = d_top;
    BILD_TRY(tangent.upload(call));
    BILD_TRY(tangent.reserve(call, chunk));

    coef.resize((size_t)chunk * K);
    top.resize((size_t)chunk * K);
    std::vector<char> is_nan(chunk);
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();

    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        const int nc = std::min(chunk, n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        BILD_TRY(rec.read_back(call, nc));

        // logev of every k, the posterior over k, and the scale of every k's weights
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i;
            std::vector<double> zk(K), lw(K);
            bool bad_traj = false;
            double lmax = ninf;
            rec.each_k(i, rec.T[jt], [&](int k, const SegdpEvidence &e) {
                zk[k] = e.z;
                top[(size_t)i * K + k] = e.top;
                const double lp = log_k_prior ? log_k_prior[(size_t)jt * K + k] : 0.0;
                lw[k] = lp > ninf ? lp + e.logev : ninf;    // a k of prior weight 0 does not count, NaN or not
                if (std::isnan(lw[k])) bad_traj = true;
                else lmax = std::max(lmax, lw[k]);
                if (out->logev) out->logev[(size_t)jt * K + k] = e.logev;
            });
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
        if (launch_segsens_weight(rec.p, w, st)) return fail(BILD_ERR_HIP, "launch of the weight kernel failed");
        BILD_TRY(tangent.run(call, j0, nc, is_nan.data(), w.omega, w.om_slot, w.om_tri, rec.p.ld, out->exp_logl, out->grad, out->fisher));
    }
    return BILD_OK;
}
