// Expected segment-length counts under a dwell-time prior (include/bild_amd.h, "expected segment lengths under a dwell-time
// prior"): the refusals, the chunks of whole trajectories, the forward and backward passes of the
// dwell-time recursion and its jump counts as bild_gauss_dwell_evidence launches them (so that logev, n_nan_windows and
// exp_jumps are the same numbers), the length kernels, and the NaN rule on what comes back.  Kernels: gauss_dwelllen.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_dwelllen.h"

extern "C" int bild_gauss_dwell_lengths(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                        const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                        unsigned flags, int64_t scratch_bytes, bild_dwell_lengths_out *out)
{
    using namespace bild;
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (flags & ~BILD_DWELL_NAN_OMIT) return fail(BILD_ERR_INVALID, "flags = %u: unknown bits", flags);
    const int S = m->S;
    BILD_TRY(dwell_check_call(S, L, log_init, log_jump, log_dwell, log_surv, n_traj, T, T_max, scratch_bytes));
    if (n_traj == 0) return BILD_OK;
    int Tm = 1;
    for (int j = 0; j < n_traj; ++j) Tm = std::max(Tm, T[j]);
    const bool omit = (flags & BILD_DWELL_NAN_OMIT) != 0;
    const int ld = Tm + 1, nblk = (Tm + kDwellLenBlock - 1) / kDwellLenBlock;
    const int64_t slot = (int64_t)S * ld, part = (int64_t)S * nblk * Tm;

    CallFrame call;
    BILD_TRY(call.open(m, ts));
    hipStream_t st = call.st;

    // a trajectory's share of the chunk: the eight tables of the recursion, the blocks' shares, D and C, the jumps and I
    const int64_t per_traj = slot * (6 * 8 + 2 * 4) + (part + 2 * slot + S * S + S) * 8 + Tm + 24;
    int chunk = 0;
    BILD_TRY(call.chunk_of(per_traj, scratch_bytes, n_traj, &chunk));

    DwellParams p{};
    DwellPrior dp{};
    DwellLengths o{};
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
    BILD_TRY(call.alloc(&p.jumps, (size_t)chunk * S * S));      // (stay_part stays null: the jump half of the counts alone)
    BILD_TRY(call.alloc(&o.part, (size_t)chunk * part));
    BILD_TRY(call.alloc(&o.dwell, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&o.cens, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&o.init, (size_t)chunk * S));
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
    o.nblk = nblk;

    const bool lengths = out->exp_dwell || out->exp_cens;
    std::vector<double> fin((size_t)chunk * 2), jumps((size_t)chunk * S * S), first((size_t)chunk * S),
        dwell(lengths ? (size_t)chunk * slot : 0), cens(lengths ? (size_t)chunk * slot : 0);
    std::vector<long long> n_nan((size_t)chunk);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        const int nc = std::min(chunk, n_traj - j0);
        p.trajs = call.d_trajs + j0;
        p.n_traj = nc;
        if (launch_dwell_forward(p, st)) return fail(BILD_ERR_HIP, "launch of the forward pass of the dwell-time recursion failed");
        if (launch_dwell_backward(p, st)) return fail(BILD_ERR_HIP, "launch of the backward pass of the dwell-time recursion failed");
        if (launch_dwell_counts(p, st)) return fail(BILD_ERR_HIP, "launch of the jump counts of the dwell-time recursion failed");
        if (launch_dwell_lengths(p, o, st)) return fail(BILD_ERR_HIP, "launch of the length kernels failed");
        HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * 2 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_nan.data(), p.n_nan, (size_t)nc * sizeof(long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(jumps.data(), p.jumps, (size_t)nc * S * S * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(first.data(), o.init, (size_t)nc * S * 8, hipMemcpyDeviceToHost, st));
        if (lengths) {
            HIP_TRY(hipMemcpyAsync(dwell.data(), o.dwell, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(cens.data(), o.cens, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));

        // section 21's NaN rule; behind a trajectory's T the length tables are 0, and so is D at l = T
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = T[jt];
            const bool bad = !omit && n_nan[i] > 0;
            const bool usable = !bad && !std::isinf(fin[2 * i]);
            if (out->logev) out->logev[jt] = bad ? nan : fin[2 * i];
            if (out->n_nan_windows) out->n_nan_windows[jt] = n_nan[i];
            if (out->exp_jumps)
                for (int e = 0; e < S * S; ++e) out->exp_jumps[(size_t)jt * S * S + e] = usable ? jumps[(size_t)i * S * S + e] : nan;
            if (out->exp_init)
                for (int s = 0; s < S; ++s) out->exp_init[(size_t)jt * S + s] = usable ? first[(size_t)i * S + s] : nan;
            for (int s = 0; s < S && lengths; ++s) {
                const double *d = dwell.data() + (size_t)i * slot + (size_t)s * ld, *c = cens.data() + (size_t)i * slot + (size_t)s * ld;
                const size_t row = ((size_t)jt * S + s) * T_max;
                for (int t = 0; t < T_max; ++t) {
                    if (out->exp_dwell) out->exp_dwell[row + t] = t >= Tj ? 0.0 : usable ? d[t] : nan;
                    if (out->exp_cens) out->exp_cens[row + t] = t >= Tj ? 0.0 : usable ? c[t] : nan;
                }
            }
        }
    }
    return BILD_OK;
}
