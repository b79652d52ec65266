// Exact fixed-lag smoothing under a dwell-time prior (include/bild_amd.h, "exact fixed-lag smoothing under a dwell-time prior";
// DESIGN.md section 26): the forward pass of the dwell-time recursion through DwellCall (gauss_dwell.h), as
// bild_gauss_dwell_evidence runs it, so that logev is the same number; the filter kernel for the two counts of NaN windows per
// prefix; the call's own tables, the two kernels of gauss_dwelllag.hip, and the NaN rule of a truncated trajectory on what comes
// back.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_dwellfilt.h"
#include "gauss_dwelllag.h"

static_assert(bild::kDwellLagMax == BILD_DWELL_LAG_MAX, "the kernels' window and the limit of the C ABI");

extern "C" int bild_gauss_dwell_lag(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                    const double *log_jump, const double *log_dwell, const double *log_surv, int T_max, int lag,
                                    unsigned flags, int64_t scratch_bytes, bild_dwell_lag_out *out)
{
    using namespace bild;
    DwellCall rec;      // (before the frame, with the host copies below: asynchronous copies write them)
    std::vector<double> lagged;
    std::vector<int32_t> n_surv, n_dwell;
    std::vector<int64_t> skipped;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    if (lag < 0) return fail(BILD_ERR_INVALID, "lag = %d is negative", lag);
    if (lag > kDwellLagMax)
        return fail(BILD_ERR_UNSUPPORTED, "lag = %d: a window of lag + 1 frames is one wavefront, at most %d", lag, kDwellLagMax);
    if (rec.n_traj == 0) return BILD_OK;
    const int S = rec.S, Tm = rec.Tm, nl = lag + 1;

    DwellFilter f{};
    DwellLag o{};
    o.lag = lag;

    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kDwellForward, dwell_filter_bytes(S, Tm, 0) + dwell_lag_bytes(S, Tm, lag)));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk;
    const size_t frames = (size_t)chunk * Tm;
    BILD_TRY(call.alloc(&f.prefix, frames));
    BILD_TRY(call.alloc(&f.filt, frames * S));
    BILD_TRY(call.alloc(&f.run_mean, frames));
    BILD_TRY(call.alloc(&f.n_surv, frames));
    BILD_TRY(call.alloc(&f.n_dwell, frames));
    BILD_TRY(call.alloc(&o.Hbase, (size_t)chunk * p.slot));
    BILD_TRY(call.alloc(&o.Kbase, (size_t)chunk * p.slot));
    BILD_TRY(call.alloc(&o.lagged, frames * S * nl));

    if (out->log_lagged) lagged.resize(frames * S * nl);
    n_surv.resize(frames);
    n_dwell.resize(frames);
    skipped.resize((size_t)Tm);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        const size_t fr = (size_t)nc * Tm;
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        if (launch_dwell_filter(p, f, st)) return fail(BILD_ERR_HIP, "launch of the filter kernel failed");
        if (launch_dwell_lag_bases(p, o, st)) return fail(BILD_ERR_HIP, "launch of the base kernel of the fixed-lag smoother failed");
        if (launch_dwell_lag_windows(p, o, st)) return fail(BILD_ERR_HIP, "launch of the window kernel of the fixed-lag smoother failed");
        if (out->log_lagged) HIP_TRY(hipMemcpyAsync(lagged.data(), o.lagged, fr * S * nl * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_surv.data(), f.n_surv, fr * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(n_dwell.data(), f.n_dwell, fr * 4, hipMemcpyDeviceToHost, st));
        BILD_TRY(rec.read_back(call, nc));

        // the cut u speaks of x[:u]: that trajectory's forward pass counts nA at its end frames e < u and nG at u
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt];
            if (out->logev) out->logev[jt] = rec.verdict(i).logev;
            int64_t before = 0;     // sum of nA(e), e <= t
            bool clean = true;      // no cut of the trajectory has skipped a window
            for (int t = 0; t < Tj; ++t) {
                const size_t at = (size_t)i * Tm + t;
                skipped[t] = before + n_surv[at];
                before += n_dwell[at];
                clean = clean && skipped[t] == 0;
            }
            if (out->n_nan_windows)
                for (int t = 0; t < T_max; ++t) out->n_nan_windows[(size_t)jt * T_max + t] = t < Tj ? skipped[t] : 0;
            if (!out->log_lagged) continue;
            for (int s = 0; s < S; ++s) {
                double *rows = out->log_lagged + ((size_t)jt * S + s) * T_max * nl;
                const double *from = lagged.data() + ((size_t)i * S + s) * Tm * nl;
                if (rec.omit || clean) {
                    std::copy(from, from + (size_t)Tj * nl, rows);
                } else {
                    for (int t = 0; t < Tj; ++t)
                        for (int l = 0; l < nl; ++l) {
                            const size_t at = (size_t)t * nl + l;
                            rows[at] = skipped[std::min(t + l, Tj - 1)] == 0 ? from[at] : nan;
                        }
                }
                std::fill(rows + (size_t)Tj * nl, rows + (size_t)T_max * nl, nan);
            }
        }
    }
    return BILD_OK;
}
