// Exact inference under a dwell-time prior (include/bild_amd.h, "exact inference under a dwell-time prior"; DESIGN.md
// section 21): the refusals and the upload of the prior (gauss_dwelldraw.cpp's as well), the chunks of whole trajectories,
// the launches on the set's stream, and the NaN rule on what comes back.  Kernels: gauss_dwell.hip.
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_dwell.h"

namespace {

using namespace bild;

// finite or -inf
int check_logs(const char *name, const double *a, size_t n)
{
    if (!a) return fail(BILD_ERR_INVALID, "%s is NULL", name);
    for (size_t i = 0; i < n; ++i)
        if (std::isnan(a[i]) || (std::isinf(a[i]) && a[i] > 0.0))
            return fail(BILD_ERR_INVALID, "%s[%zu] = %g; entries must be finite or -inf", name, i, a[i]);
    return BILD_OK;
}

} // namespace

namespace bild {

int dwell_check_call(int S, int L, const double *log_init, const double *log_jump, const double *log_dwell, const double *log_surv,
                     int n_traj, const int *T, int T_max, int64_t scratch_bytes)
{
    if (S > kDwellMaxS) return fail(BILD_ERR_UNSUPPORTED, "the model has %d states; the dwell-time recursion supports at most %d", S, kDwellMaxS);
    if (L < 1) return fail(BILD_ERR_INVALID, "L = %d: the dwell tables need at least one length", L);
    BILD_TRY(check_logs("log_init", log_init, (size_t)S));
    BILD_TRY(check_logs("log_jump", log_jump, (size_t)S * S));
    BILD_TRY(check_logs("log_dwell", log_dwell, (size_t)S * L));
    BILD_TRY(check_logs("log_surv", log_surv, (size_t)S * L));
    bool any_init = false;
    for (int s = 0; s < S; ++s) {
        if (!std::isinf(log_jump[s * S + s]))
            return fail(BILD_ERR_INVALID, "log_jump[%d][%d] = %g; the diagonal must be -inf (a self-jump would split a segment)", s, s,
                        log_jump[s * S + s]);
        any_init = any_init || !std::isinf(log_init[s]);
    }
    if (!any_init) return fail(BILD_ERR_INVALID, "log_init is -inf everywhere");
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    for (int j = 0; j < n_traj; ++j) {
        if (T[j] > T_max) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames, more than T_max = %d", j, T[j], T_max);
        if (T[j] > L) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames, more than the L = %d lengths of the dwell tables", j, T[j], L);
    }
    return BILD_OK;
}

int dwell_upload_prior(CallFrame &call, int S, int L, const double *log_init, const double *log_jump, const double *log_dwell,
                       const double *log_surv, DwellPrior *prior)
{
    const size_t n_jump = (size_t)S * S, n_len = (size_t)S * L;
    std::vector<double> host(S + n_jump + 2 * n_len);
    std::copy_n(log_init, S, host.data());
    std::copy_n(log_jump, n_jump, host.data() + S);
    std::copy_n(log_dwell, n_len, host.data() + S + n_jump);
    std::copy_n(log_surv, n_len, host.data() + S + n_jump + n_len);
    double *d = nullptr;
    BILD_TRY(call.alloc(&d, host.size()));
    HIP_TRY(hipMemcpy(d, host.data(), host.size() * 8, hipMemcpyHostToDevice));     // (synchronous: `host` ends here)
    *prior = DwellPrior{d, d + S, d + S + n_jump, d + S + n_jump + n_len};
    return BILD_OK;
}

} // namespace bild

extern "C" int bild_gauss_dwell_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                         const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                         unsigned flags, int64_t scratch_bytes, bild_dwell_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (flags & ~BILD_DWELL_NAN_OMIT) return fail(BILD_ERR_INVALID, "flags = %u: unknown bits", flags);
    const int S = m->S;
    BILD_TRY(dwell_check_call(S, L, log_init, log_jump, log_dwell, log_surv, n_traj, T, T_max, scratch_bytes));
    int Tm = 1;
    for (int j = 0; j < n_traj; ++j) Tm = std::max(Tm, T[j]);
    if (n_traj == 0) return BILD_OK;
    const bool omit = (flags & BILD_DWELL_NAN_OMIT) != 0, marg = out->log_post != nullptr;
    const bool stats = marg;    // log_post == NULL: the forward pass alone
    const int ld = Tm + 1, ntile = (Tm + kDwellTile - 1) / kDwellTile;
    const int64_t slot = (int64_t)S * ld, rows = (int64_t)S * ntile * Tm;

    CallFrame call;
    BILD_TRY(call.open(m, ts));
    hipStream_t st = call.st;

    const int64_t per_traj = slot * (4 * 8 + 2 * 4 + (stats ? 4 * 8 : 0)) + (stats ? (rows + (int64_t)S * ntile + S * S + S) * 8 : 0) + Tm + 24;
    int chunk = 0;
    BILD_TRY(call.chunk_of(per_traj, scratch_bytes, n_traj, &chunk));

    DwellParams p{};
    DwellPrior dp{};
    BILD_TRY(dwell_upload_prior(call, S, L, log_init, log_jump, log_dwell, log_surv, &dp));
    BILD_TRY(call.alloc(&p.A, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.AV, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.alpha, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.alphaV, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.Aarg, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.alphaArg, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.fin, (size_t)chunk * 2));
    BILD_TRY(call.alloc(&p.n_nan, (size_t)chunk));
    BILD_TRY(call.alloc(&p.map_states, (size_t)chunk * Tm));
    if (stats) {
        BILD_TRY(call.alloc(&p.beta, (size_t)chunk * slot));
        BILD_TRY(call.alloc(&p.gamma, (size_t)chunk * slot));
        BILD_TRY(call.alloc(&p.cover, (size_t)chunk * slot));
        BILD_TRY(call.alloc(&p.post, (size_t)chunk * slot));
        BILD_TRY(call.alloc(&p.row_tot, (size_t)chunk * rows));
        BILD_TRY(call.alloc(&p.stay_part, (size_t)chunk * S * ntile));
        BILD_TRY(call.alloc(&p.jumps, (size_t)chunk * S * S));
        BILD_TRY(call.alloc(&p.stay, (size_t)chunk * S));
    }
    p.log_init = dp.log_init;
    p.log_jump = dp.log_jump;
    p.log_dwell = dp.log_dwell;
    p.log_surv = dp.log_surv;
    p.slot = slot;
    p.S = S;
    p.L = L;
    p.Tm = Tm;
    p.ld = ld;
    p.ntile = ntile;

    std::vector<double> fin((size_t)chunk * 2), post(stats ? (size_t)chunk * slot : 0), jumps(stats ? (size_t)chunk * S * S : 0),
        stay(stats ? (size_t)chunk * S : 0);
    std::vector<long long> n_nan((size_t)chunk);
    std::vector<uint8_t> states((size_t)chunk * Tm);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        const int nc = std::min(chunk, n_traj - j0);
        p.trajs = call.d_trajs + j0;
        p.n_traj = nc;
        if (launch_dwell_forward(p, st)) return fail(BILD_ERR_HIP, "launch of the forward pass of the dwell-time recursion failed");
        if (stats) {
            if (launch_dwell_backward(p, st)) return fail(BILD_ERR_HIP, "launch of the backward pass of the dwell-time recursion failed");
            if (launch_dwell_cover(p, st) || launch_dwell_carry(p, st) || launch_dwell_counts(p, st))
                return fail(BILD_ERR_HIP, "launch of the statistics of the dwell-time recursion failed");
            HIP_TRY(hipMemcpyAsync(post.data(), p.post, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(jumps.data(), p.jumps, (size_t)nc * S * S * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(stay.data(), p.stay, (size_t)nc * S * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * 2 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_nan.data(), p.n_nan, (size_t)nc * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(states.data(), p.map_states, (size_t)nc * Tm, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = T[jt];
            const bool bad = !omit && n_nan[i] > 0;
            const double logev = bad ? nan : fin[2 * i];
            const bool usable = !bad && !std::isinf(fin[2 * i]);
            if (out->logev) out->logev[jt] = logev;
            if (out->map_logjoint) out->map_logjoint[jt] = fin[2 * i + 1];
            if (out->n_nan_windows) out->n_nan_windows[jt] = n_nan[i];
            if (out->map_states) {
                uint8_t *row = out->map_states + (size_t)jt * T_max;
                for (int t = 0; t < T_max; ++t) row[t] = t < Tj ? states[(size_t)i * Tm + t] : 255;
            }
            if (marg) {
                double *lp = out->log_post + (size_t)jt * S * T_max;
                for (int s = 0; s < S; ++s)
                    for (int t = 0; t < T_max; ++t)
                        lp[(size_t)s * T_max + t] = usable && t < Tj ? std::log(post[(size_t)i * slot + (size_t)s * ld + t]) : nan;
            }
            if (stats && out->exp_jumps)
                for (int e = 0; e < S * S; ++e) out->exp_jumps[(size_t)jt * S * S + e] = usable ? jumps[(size_t)i * S * S + e] : nan;
            if (stats && out->exp_stay)
                for (int s = 0; s < S; ++s) out->exp_stay[(size_t)jt * S + s] = usable ? stay[(size_t)i * S + s] : nan;
        }
    }
    return BILD_OK;
}
