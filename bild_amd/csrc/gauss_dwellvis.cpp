// Exact posterior of the number of visits to a set of states under a dwell-time prior (include/bild_amd_visits.h; DESIGN.md
// section 30): the forward pass of the dwell-time recursion through DwellCall (gauss_dwell.h), as bild_gauss_dwell_evidence
// runs it, so that logev and n_nan_windows are the same numbers and the NaN rule the same; the call's own table and kernel.
// Kernel: gauss_dwellvis.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/bild_amd_visits.h"
#include "gauss_call.h"
#include "gauss_dwellvis.h"

extern "C" int bild_gauss_dwell_visits(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                       const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                       int n_max, unsigned target, unsigned flags, int64_t scratch_bytes, bild_dwell_visits_out *out)
{
    using namespace bild;
    DwellCall rec;      // (before the frame, with the host copy below: asynchronous copies write them)
    std::vector<double> last;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    const int S = rec.S, Tm = rec.Tm;
    const unsigned all = (1u << S) - 1u;
    if (target == 0 || (target & ~all) || target == all)
        return fail(BILD_ERR_INVALID, "target = 0x%x: a non-empty proper subset of the %d states, bit s for state s", target, S);
    if (n_max < 0) return fail(BILD_ERR_INVALID, "n_max = %d is negative", n_max);
    if (rec.n_traj == 0) return BILD_OK;

    // the call's own tables: alpha of every switch frame, and the rows A(T, ., n); no trajectory of the call has more than
    // (Tm + 1) / 2 visits
    DwellVisits o{};
    o.target = target;
    o.n_top = std::min(n_max, (Tm + 1) / 2);
    o.ldn = o.n_top + 1;
    o.stride = (int64_t)S * Tm * o.ldn;
    const int64_t rows = (int64_t)o.ldn * S, col = (int64_t)(n_max + 1) * S;
    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kDwellForward, dwell_visits_bytes(S, Tm, o.n_top)));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk;
    BILD_TRY(call.alloc(&o.alpha, (size_t)chunk * (size_t)o.stride));
    BILD_TRY(call.alloc(&o.last, (size_t)chunk * rows));
    last.resize((size_t)chunk * rows);
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        const int T_top = *std::max_element(rec.T + j0, rec.T + j0 + nc);       // no trajectory of the chunk ends later
        for (int b = 1; b <= T_top; ++b)
            if (launch_dwell_visits(p, o, b, st)) return fail(BILD_ERR_HIP, "launch of end frame %d of the visit recursion failed", b);
        HIP_TRY(hipMemcpyAsync(last.data(), o.last, (size_t)nc * rows * 8, hipMemcpyDeviceToHost, st));
        BILD_TRY(rec.read_back(call, nc));

        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt], top = (Tj + 1) / 2;
            const DwellVerdict v = rec.verdict(i);
            if (out->logev) out->logev[jt] = v.logev;
            if (out->n_nan_windows) out->n_nan_windows[jt] = rec.n_nan[i];
            // rows n > (T + 1) / 2 have no profile (and no end frame ran for a trajectory without frames); the sum for the
            // tail runs over n ascending, s ascending inside
            double total = 0.0;
            for (int n = 0; n <= n_max; ++n)
                for (int s = 0; s < S; ++s) {
                    const double lv = !v.usable ? nan : n > top || Tj < 1 ? ninf : last[(size_t)i * rows + (size_t)n * S + s] - v.logev;
                    if (out->log_visits) out->log_visits[(size_t)jt * col + (size_t)n * S + s] = lv;
                    if (lv > ninf) total += std::exp(lv);
                }
            if (out->log_tail) out->log_tail[jt] = !v.usable ? nan : n_max >= top ? ninf : std::log(std::max(0.0, 1.0 - total));
        }
    }
    return BILD_OK;
}
