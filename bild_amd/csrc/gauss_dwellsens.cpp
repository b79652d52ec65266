// Gradient of the exact evidence under a dwell-time prior (include/bild_amd.h, "evidence sensitivities under a dwell-time
// prior"): the forward and backward passes of the dwell-time recursion through DwellCall
// (gauss_dwell.h), as bild_gauss_dwell_evidence runs them, so that logev is the same number and the NaN rule the same; the
// call's own weight table and the weighted tangent jobs (gauss_segtangent.h).  Kernel: gauss_dwellsens.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_dwellsens.h"
#include "gauss_segtangent.h"
#include "gauss_windows.h"

extern "C" int bild_gauss_dwell_sensitivities(const bild_gauss_model *m, const bild_gauss_trajset *ts, const double *x, int L,
                                              const double *log_init, const double *log_jump, const double *log_dwell,
                                              const double *log_surv, unsigned flags, int P, const bild_gauss_derivs *dm,
                                              int64_t scratch_bytes, bild_dwellsens_out *out)
{
    using namespace bild;
    DwellCall rec;          // (both before the frame: asynchronous copies use their vectors)
    SegTangent tangent;
    // (nothing here is padded to a T_max, so no trajectory is too long for it)
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, std::numeric_limits<int>::max(), flags, scratch_bytes, out));
    if (rec.n_traj == 0) return BILD_OK;
    BILD_TRY(gauss_check_args(m, rec.n_traj, rec.T, x, 0, 1, nullptr, nullptr, nullptr, P, dm));
    tangent.stage(m, rec.n_traj, rec.T, x, P, dm);

    // the call's own table: the weights
    DwellsensWeights w{};
    w.om_tri = gauss_w_per_state(rec.Tm);
    w.om_slot = (int64_t)rec.S * (w.om_tri + rec.Tm + 1);

    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kDwellForward | kDwellBackward, w.om_slot * 8));
    const int chunk = rec.chunk;
    BILD_TRY(call.alloc(&w.omega, (size_t)chunk * w.om_slot));
    BILD_TRY(tangent.upload(call));
    BILD_TRY(tangent.reserve(call, chunk));
    std::vector<char> skip(chunk);

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        BILD_TRY(rec.read_back(call, nc));

        // a trajectory that is NaN, or has no profile of positive weight, launches no job
        for (int i = 0; i < nc; ++i) {
            const DwellVerdict v = rec.verdict(i);
            skip[i] = !v.usable;
            if (out->logev) out->logev[j0 + i] = v.logev;
            if (out->n_nan_windows) out->n_nan_windows[j0 + i] = rec.n_nan[i];
        }
        if (launch_dwellsens_weight(rec.p, w, call.st)) return fail(BILD_ERR_HIP, "launch of the weight kernel failed");
        BILD_TRY(tangent.run(call, j0, nc, skip.data(), w.omega, w.om_slot, w.om_tri, rec.p.ld, out->exp_logl, out->grad, out->fisher));
    }
    return BILD_OK;
}
