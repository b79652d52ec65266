// Gradient of the exact evidence under a dwell-time prior (include/bild_amd.h, "evidence sensitivities under a dwell-time
// prior"): the refusals, the chunks of whole trajectories, the forward and backward passes of the
// dwell-time recursion as bild_gauss_dwell_evidence launches them (so that logev is the same number), the NaN rule, the
// weight table and the weighted tangent jobs (gauss_segtangent.h).  Kernel: gauss_dwellsens.hip.
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
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (flags & ~BILD_DWELL_NAN_OMIT) return fail(BILD_ERR_INVALID, "flags = %u: unknown bits", flags);
    const int S = m->S;
    // (nothing here is padded to a T_max, so no trajectory is too long for it)
    BILD_TRY(dwell_check_call(S, L, log_init, log_jump, log_dwell, log_surv, n_traj, T, std::numeric_limits<int>::max(), scratch_bytes));
    if (n_traj == 0) return BILD_OK;
    BILD_TRY(gauss_check_args(m, n_traj, T, x, 0, 1, nullptr, nullptr, nullptr, P, dm));
    int Tm = 1;
    for (int j = 0; j < n_traj; ++j) Tm = std::max(Tm, T[j]);
    const bool omit = (flags & BILD_DWELL_NAN_OMIT) != 0;
    const int ld = Tm + 1;
    const int64_t slot = (int64_t)S * ld, om_tri = gauss_w_per_state(Tm), om_slot = (int64_t)S * (om_tri + ld);

    SegTangent tangent;     // (before the frame: asynchronous copies read its vectors)
    tangent.stage(m, n_traj, T, x, P, dm);

    CallFrame call;
    BILD_TRY(call.open(m, ts));
    hipStream_t st = call.st;

    // a trajectory's share of the chunk: the eight tables of the recursion and the weight table
    const int64_t per_traj = slot * (6 * 8 + 2 * 4) + om_slot * 8 + Tm + 24;
    int chunk = 0;
    BILD_TRY(call.chunk_of(per_traj, scratch_bytes, n_traj, &chunk));

    DwellParams p{};
    DwellPrior dp{};
    DwellsensWeights w{};
    BILD_TRY(dwell_upload_prior(call, S, L, log_init, log_jump, log_dwell, log_surv, &dp));
    BILD_TRY(call.alloc(&p.A, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.AV, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.alpha, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.alphaV, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.Aarg, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.alphaArg, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.beta, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.gamma, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.fin, (size_t)chunk * 2));
    BILD_TRY(call.alloc(&p.n_nan, (size_t)chunk));
    BILD_TRY(call.alloc(&p.map_states, (size_t)chunk * Tm));
    BILD_TRY(call.alloc(&w.omega, (size_t)chunk * om_slot));
    p.log_init = dp.log_init;
    p.log_jump = dp.log_jump;
    p.log_dwell = dp.log_dwell;
    p.log_surv = dp.log_surv;
    p.slot = slot;
    p.S = S;
    p.L = L;
    p.Tm = Tm;
    p.ld = ld;
    p.ntile = (Tm + kDwellTile - 1) / kDwellTile;
    w.om_slot = om_slot;
    w.om_tri = om_tri;

    BILD_TRY(tangent.upload(call));
    BILD_TRY(tangent.reserve(call, chunk));

    std::vector<double> fin((size_t)chunk * 2);
    std::vector<long long> n_nan((size_t)chunk);
    std::vector<char> skip(chunk);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        const int nc = std::min(chunk, n_traj - j0);
        p.trajs = call.d_trajs + j0;
        p.n_traj = nc;
        if (launch_dwell_forward(p, st)) return fail(BILD_ERR_HIP, "launch of the forward pass of the dwell-time recursion failed");
        if (launch_dwell_backward(p, st)) return fail(BILD_ERR_HIP, "launch of the backward pass of the dwell-time recursion failed");
        HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * 2 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_nan.data(), p.n_nan, (size_t)nc * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        // section 21's NaN rule; a trajectory that is NaN, or has no profile of positive weight, launches no job
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i;
            const bool bad = !omit && n_nan[i] > 0;
            skip[i] = bad || std::isinf(fin[2 * i]);
            if (out->logev) out->logev[jt] = bad ? nan : fin[2 * i];
            if (out->n_nan_windows) out->n_nan_windows[jt] = n_nan[i];
        }
        if (launch_dwellsens_weight(p, w, st)) return fail(BILD_ERR_HIP, "launch of the weight kernel failed");
        BILD_TRY(tangent.run(call, j0, nc, skip.data(), w.omega, om_slot, om_tri, ld, out->exp_logl, out->grad, out->fisher));
    }
    return BILD_OK;
}
