// Exact online filtering under a dwell-time prior (include/bild_amd.h, "exact online filtering under a dwell-time prior";
// DESIGN.md section 25): the forward pass of the dwell-time recursion through DwellCall (gauss_dwell.h), as
// bild_gauss_dwell_evidence runs it, so that logev is the same number; the call's own tables, the filter kernel, and the NaN
// rule of a truncated trajectory on what comes back.  Kernel: gauss_dwellfilt.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_dwellfilt.h"

extern "C" int bild_gauss_dwell_filter(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                       const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                       int run_max, unsigned flags, int64_t scratch_bytes, bild_dwell_filter_out *out)
{
    using namespace bild;
    DwellCall rec;      // (before the frame, with the host copies below: asynchronous copies write them)
    std::vector<double> prefix, filt, mean, runs;
    std::vector<int32_t> n_surv, n_dwell;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    if (run_max < 0) return fail(BILD_ERR_INVALID, "run_max = %d is negative", run_max);
    if (out->log_run && run_max == 0) return fail(BILD_ERR_INVALID, "log_run is given with run_max = 0");
    if (rec.n_traj == 0) return BILD_OK;
    const int S = rec.S, Tm = rec.Tm;

    DwellFilter o{};
    o.R = out->log_run ? run_max : 0;
    const int R = o.R;

    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kDwellForward, dwell_filter_bytes(S, Tm, R)));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk;
    const size_t frames = (size_t)chunk * Tm;
    BILD_TRY(call.alloc(&o.prefix, frames));
    BILD_TRY(call.alloc(&o.filt, frames * S));
    BILD_TRY(call.alloc(&o.run_mean, frames));
    BILD_TRY(call.alloc(&o.n_surv, frames));
    BILD_TRY(call.alloc(&o.n_dwell, frames));
    if (R) BILD_TRY(call.alloc(&o.log_run, frames * S * R));

    prefix.resize(frames);
    filt.resize(frames * S);
    mean.resize(frames);
    n_surv.resize(frames);
    n_dwell.resize(frames);
    runs.resize(frames * S * R);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        const size_t fr = (size_t)nc * Tm;
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        if (launch_dwell_filter(p, o, st)) return fail(BILD_ERR_HIP, "launch of the filter kernel failed");
        HIP_TRY(hipMemcpyAsync(prefix.data(), o.prefix, fr * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(filt.data(), o.filt, fr * S * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(mean.data(), o.run_mean, fr * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_surv.data(), o.n_surv, fr * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_dwell.data(), o.n_dwell, fr * 4, hipMemcpyDeviceToHost, st));
        if (R) HIP_TRY(hipMemcpyAsync(runs.data(), o.log_run, fr * S * R * 8, hipMemcpyDeviceToHost, st));
        BILD_TRY(rec.read_back(call, nc));

        // frame t speaks of x[:t + 1]: that trajectory's forward pass counts nA at its end frames e <= t and nG at t + 1
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt];
            if (out->logev) out->logev[jt] = rec.verdict(i).logev;
            int64_t before = 0;     // sum of nA(e), e <= t
            for (int t = 0; t < T_max; ++t) {
                const size_t at = (size_t)i * Tm + t, to = (size_t)jt * T_max + t;
                const bool in = t < Tj;
                const int64_t skipped = in ? before + n_surv[at] : 0;
                const bool keep = in && (rec.omit || skipped == 0);
                if (out->n_nan_windows) out->n_nan_windows[to] = skipped;
                if (out->prefix_logev) out->prefix_logev[to] = keep ? prefix[at] : nan;
                if (out->run_mean) out->run_mean[to] = keep ? mean[at] : nan;
                for (int s = 0; s < S; ++s) {
                    if (out->log_filtered)
                        out->log_filtered[((size_t)jt * S + s) * T_max + t] = keep ? filt[((size_t)i * S + s) * Tm + t] : nan;
                    if (!R) continue;
                    const double *from = keep ? runs.data() + (((size_t)i * S + s) * Tm + t) * R : nullptr;
                    double *row = out->log_run + (((size_t)jt * S + s) * T_max + t) * R;
                    for (int r = 0; r < R; ++r) row[r] = from ? from[r] : nan;
                }
                if (in) before += n_dwell[at];
            }
        }
    }
    return BILD_OK;
}
