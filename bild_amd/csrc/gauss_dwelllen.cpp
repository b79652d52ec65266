// Expected segment-length counts under a dwell-time prior (include/bild_amd.h, "expected segment lengths under a dwell-time
// prior"): the forward and backward passes of the dwell-time recursion through DwellCall
// (gauss_dwell.h) and its jump counts, as bild_gauss_dwell_evidence runs them, so that logev, n_nan_windows and exp_jumps
// are the same numbers and the NaN rule the same; the call's own tables and the length kernels.  Kernels: gauss_dwelllen.hip.
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
    DwellCall rec;      // (before the frame, with the host copies below: asynchronous copies write them)
    std::vector<double> jumps, first, dwell, cens;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    if (rec.n_traj == 0) return BILD_OK;
    const int S = rec.S, Tm = rec.Tm, ld = Tm + 1;
    const int64_t slot = (int64_t)S * ld;

    // the call's own tables: the blocks' shares, D, C and I
    DwellLengths o{};
    o.nblk = (Tm + kDwellLenBlock - 1) / kDwellLenBlock;
    const int64_t part = (int64_t)S * o.nblk * Tm;

    CallFrame call;
    // (no kDwellCover, so stay_part stays null: the jump half of the counts alone)
    BILD_TRY(rec.open(call, m, ts, kDwellForward | kDwellBackward | kDwellJumps, (part + slot + slot + S) * 8));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk;
    BILD_TRY(call.alloc(&o.part, (size_t)chunk * part));
    BILD_TRY(call.alloc(&o.dwell, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&o.cens, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&o.init, (size_t)chunk * S));

    const bool lengths = out->exp_dwell || out->exp_cens;
    jumps.resize((size_t)chunk * S * S);
    first.resize((size_t)chunk * S);
    dwell.resize(lengths ? (size_t)chunk * slot : 0);
    cens.resize(lengths ? (size_t)chunk * slot : 0);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        if (launch_dwell_counts(p, st)) return fail(BILD_ERR_HIP, "launch of the jump counts of the dwell-time recursion failed");
        if (launch_dwell_lengths(p, o, st)) return fail(BILD_ERR_HIP, "launch of the length kernels failed");
        HIP_TRY(hipMemcpyAsync(jumps.data(), p.jumps, (size_t)nc * S * S * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(first.data(), o.init, (size_t)nc * S * 8, hipMemcpyDeviceToHost, st));
        if (lengths) {
            HIP_TRY(hipMemcpyAsync(dwell.data(), o.dwell, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(cens.data(), o.cens, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
        }
        BILD_TRY(rec.read_back(call, nc));

        // behind a trajectory's T the length tables are 0, and so is D at l = T
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt];
            const DwellVerdict v = rec.verdict(i);
            if (out->logev) out->logev[jt] = v.logev;
            if (out->n_nan_windows) out->n_nan_windows[jt] = rec.n_nan[i];
            if (out->exp_jumps)
                for (int e = 0; e < S * S; ++e) out->exp_jumps[(size_t)jt * S * S + e] = v.usable ? jumps[(size_t)i * S * S + e] : nan;
            if (out->exp_init)
                for (int s = 0; s < S; ++s) out->exp_init[(size_t)jt * S + s] = v.usable ? first[(size_t)i * S + s] : nan;
            for (int s = 0; s < S && lengths; ++s) {
                const double *d = dwell.data() + (size_t)i * slot + (size_t)s * ld, *c = cens.data() + (size_t)i * slot + (size_t)s * ld;
                const size_t row = ((size_t)jt * S + s) * T_max;
                for (int t = 0; t < T_max; ++t) {
                    if (out->exp_dwell) out->exp_dwell[row + t] = t >= Tj ? 0.0 : v.usable ? d[t] : nan;
                    if (out->exp_cens) out->exp_cens[row + t] = t >= Tj ? 0.0 : v.usable ? c[t] : nan;
                }
            }
        }
    }
    return BILD_OK;
}
