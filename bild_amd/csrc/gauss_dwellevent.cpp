// Exact switch counts and first-contact times under a dwell-time prior (include/bild_amd.h, "switch counts under a dwell-time
// prior" and "first-contact times under a dwell-time prior"): the forward pass of the dwell-time
// recursion through DwellCall (gauss_dwell.h), as bild_gauss_dwell_evidence runs it, so that logev and n_nan_windows are the
// same numbers and the NaN rule the same; the calls' own tables and kernels.  Kernels: gauss_dwellevent.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_dwellevent.h"

extern "C" int bild_gauss_dwell_switch_counts(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                              const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                              int k_max, unsigned flags, int64_t scratch_bytes, bild_dwell_switch_counts_out *out)
{
    using namespace bild;
    DwellCall rec;      // (before the frame, with the host copy below: asynchronous copies write them)
    std::vector<double> last;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    if (k_max < 0) return fail(BILD_ERR_INVALID, "k_max = %d is negative", k_max);
    if (k_max > std::max(T_max, 1) - 1) return fail(BILD_ERR_INVALID, "k_max = %d: a trajectory of T_max = %d frames has at most %d switches", k_max, T_max, std::max(T_max, 1) - 1);
    if (rec.n_traj == 0) return BILD_OK;
    const int S = rec.S, Tm = rec.Tm, ld = Tm + 1;
    const int64_t slot = (int64_t)S * ld, col = (int64_t)(k_max + 1) * S;

    // the call's own tables: the two rows of alpha and the column A_n(T, .)
    DwellLevels o{};
    o.k_max = k_max;
    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kDwellForward, (2 * slot + col) * 8));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk;
    BILD_TRY(call.alloc(&o.lev, (size_t)chunk * 2 * slot));
    BILD_TRY(call.alloc(&o.last, (size_t)chunk * col));
    last.resize((size_t)chunk * col);
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
    const int n_top = std::min(k_max, Tm - 1);      // no trajectory of the call has more switches

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        for (int n = 0; n <= n_top; ++n)
            if (launch_dwell_level(p, o, n, st)) return fail(BILD_ERR_HIP, "launch of level %d of the switch counts failed", n);
        HIP_TRY(hipMemcpyAsync(last.data(), o.last, (size_t)nc * col * 8, hipMemcpyDeviceToHost, st));
        BILD_TRY(rec.read_back(call, nc));

        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt];
            const DwellVerdict v = rec.verdict(i);
            if (out->logev) out->logev[jt] = v.logev;
            if (out->n_nan_windows) out->n_nan_windows[jt] = rec.n_nan[i];
            // levels n > T - 1 have no profile; the sum for the tail runs over n ascending, s ascending inside
            double total = 0.0;
            for (int n = 0; n <= k_max; ++n)
                for (int s = 0; s < S; ++s) {
                    const double lc = !v.usable ? nan : n > Tj - 1 ? ninf : last[(size_t)i * col + (size_t)n * S + s] - v.logev;
                    if (out->log_count) out->log_count[(size_t)jt * col + (size_t)n * S + s] = lc;
                    if (lc > ninf) total += std::exp(lc);
                }
            if (out->log_tail) out->log_tail[jt] = !v.usable ? nan : k_max >= Tj - 1 ? ninf : std::log(std::max(0.0, 1.0 - total));
        }
    }
    return BILD_OK;
}

extern "C" int bild_gauss_dwell_first_contact(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                              const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                              unsigned target, unsigned flags, int64_t scratch_bytes, bild_dwell_first_contact_out *out)
{
    using namespace bild;
    DwellCall rec;      // (before the frame, with the host copies below: asynchronous copies write them)
    std::vector<double> first, init2, jump2;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    const int S = rec.S, Tm = rec.Tm, ld = Tm + 1;
    const unsigned all = (1u << S) - 1u;
    if (target == 0 || (target & ~all) || target == all)
        return fail(BILD_ERR_INVALID, "target = 0x%x: a non-empty proper subset of the %d states, bit s for state s", target, S);
    if (rec.n_traj == 0) return BILD_OK;

    // the second prior block: nothing starts in G and nothing jumps into it
    const double ninf = -std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    init2.assign(log_init, log_init + S);
    jump2.assign(log_jump, log_jump + (size_t)S * S);
    for (int s = 0; s < S; ++s) {
        if (!(target >> s & 1u)) continue;
        init2[s] = ninf;
        for (int r = 0; r < S; ++r) jump2[(size_t)r * S + s] = ninf;
    }
    rec.second(init2.data(), jump2.data());

    DwellContact o{};
    o.target = target;
    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kDwellForward | kDwellBackward, (int64_t)ld * 8));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk;
    BILD_TRY(call.alloc(&o.first, (size_t)chunk * ld));
    o.Ax = rec.p2.A;
    first.resize((size_t)chunk * ld);

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        if (launch_dwell_contact(p, o, st)) return fail(BILD_ERR_HIP, "launch of the first-contact kernel failed");
        HIP_TRY(hipMemcpyAsync(first.data(), o.first, (size_t)nc * ld * 8, hipMemcpyDeviceToHost, st));
        BILD_TRY(rec.read_back(call, nc));

        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt];
            const DwellVerdict v = rec.verdict(i);
            const double *f = first.data() + (size_t)i * ld;
            if (out->logev) out->logev[jt] = v.logev;
            if (out->n_nan_windows) out->n_nan_windows[jt] = rec.n_nan[i];
            if (out->log_first)
                for (int t = 0; t < T_max; ++t) out->log_first[(size_t)jt * T_max + t] = v.usable && t < Tj ? f[t] - v.logev : nan;
            if (out->log_never) out->log_never[jt] = v.usable ? f[Tm] - v.logev : nan;
        }
    }
    return BILD_OK;
}
