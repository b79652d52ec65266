// Exact inference under a dwell-time prior (include/bild_amd.h, "exact inference under a dwell-time prior"; DESIGN.md
// section 21).  DwellCall is the host side of the recursion that bild_gauss_dwell_evidence here, gauss_dwellsens.cpp,
// gauss_dwelllen.cpp, gauss_dwellfilt.cpp and gauss_dwelldraw.cpp share (gauss_dwell.h): the refusals, the frame on the set's stream, the chunks
// of whole trajectories, the prior's upload, the tables, the kernels' parameters, the two passes, and the NaN rule on what
// comes back.  Kernels: gauss_dwell.hip.
#include <algorithm>
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

// What every call on a dwell-time prior refuses about the prior and the set's lengths: more than kDwellMaxS states, L < 1 or
// shorter than a trajectory, a NaN or +inf table entry, a finite diagonal of log_jump, log_init that is -inf everywhere, a
// negative scratch_bytes, T_max shorter than a trajectory.  A BILD_* code.
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

} // namespace

namespace bild {

DwellVerdict dwell_nan_rule(const double *fin, long long n_nan, bool omit)
{
    const bool bad = !omit && n_nan > 0;
    return DwellVerdict{bad, !bad && !std::isinf(fin[0]), bad ? std::numeric_limits<double>::quiet_NaN() : fin[0]};
}

int DwellCall::check(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L_, const double *log_init, const double *log_jump,
                     const double *log_dwell, const double *log_surv, int T_max, unsigned flags, int64_t scratch, const void *out)
{
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (flags & ~BILD_DWELL_NAN_OMIT) return fail(BILD_ERR_INVALID, "flags = %u: unknown bits", flags);
    S = m->S;
    L = L_;
    BILD_TRY(dwell_check_call(S, L, log_init, log_jump, log_dwell, log_surv, n_traj, T, T_max, scratch));
    for (int j = 0; j < n_traj; ++j) Tm = std::max(Tm, T[j]);
    n = n_traj;
    omit = (flags & BILD_DWELL_NAN_OMIT) != 0;
    scratch_bytes = scratch;
    prior[0] = log_init, prior[1] = log_jump, prior[2] = log_dwell, prior[3] = log_surv;
    return BILD_OK;
}

int DwellCall::open(CallFrame &call, const bild_gauss_model *m, const bild_gauss_trajset *ts, unsigned sets_, int64_t own_bytes)
{
    sets = sets_;
    BILD_TRY(call.open(m, ts));
    const bool two = prior2[0] != nullptr;
    BILD_TRY(call.chunk_of(dwell_table_bytes(sets, S, Tm) + (two ? dwell_table_bytes(kDwellForward, S, Tm) : 0) + own_bytes,
                           scratch_bytes, n, &chunk));

    // the four prior tables, and the second block's two, in one device block (synchronous copy: `host` ends here)
    const size_t len[6] = {(size_t)S, (size_t)S * S, (size_t)S * L, (size_t)S * L, (size_t)S, (size_t)S * S};
    const double *from[6] = {prior[0], prior[1], prior[2], prior[3], prior2[0], prior2[1]};
    const double **member[6] = {&p.log_init, &p.log_jump, &p.log_dwell, &p.log_surv, &p2.log_init, &p2.log_jump};
    const int blocks = two ? 6 : 4;
    std::vector<double> host;
    for (int t = 0; t < blocks; ++t) host.insert(host.end(), from[t], from[t] + len[t]);
    double *d = nullptr;
    BILD_TRY(call.alloc(&d, host.size()));
    HIP_TRY(hipMemcpy(d, host.data(), host.size() * 8, hipMemcpyHostToDevice));
    for (int t = 0; t < blocks; d += len[t++]) *member[t] = d;

    const int ld = Tm + 1, ntile = dwell_ntile(Tm);
    const int64_t slot = (int64_t)S * ld;
#define X(name, set, entries) \
    if (sets & (set)) BILD_TRY(call.alloc(&p.name, (size_t)chunk * (size_t)(entries)));
    BILD_DWELL_TABLES(X)
#undef X
    p.slot = slot;
    p.S = S;
    p.L = L;
    p.Tm = Tm;
    p.ld = ld;
    p.ntile = ntile;
    if (sets & kDwellForward) {
        fin.resize((size_t)chunk * 2);
        n_nan.resize((size_t)chunk);
    }
    if (two) {
        const double *init2 = p2.log_init, *jump2 = p2.log_jump;
        p2 = p;
        p2.log_init = init2, p2.log_jump = jump2;
#define X(name, set, entries) \
    if ((set) == kDwellForward) BILD_TRY(call.alloc(&p2.name, (size_t)chunk * (size_t)(entries)));
        BILD_DWELL_TABLES(X)
#undef X
    }
    return BILD_OK;
}

int DwellCall::run(CallFrame &call, const GaussTraj *trajs, int nc)
{
    p.trajs = trajs;
    p.n_traj = nc;
    if ((sets & kDwellForward) && launch_dwell_forward(p, call.st))
        return fail(BILD_ERR_HIP, "launch of the forward pass of the dwell-time recursion failed");
    if ((sets & kDwellBackward) && launch_dwell_backward(p, call.st))
        return fail(BILD_ERR_HIP, "launch of the backward pass of the dwell-time recursion failed");
    if (prior2[0]) {
        p2.trajs = trajs;
        p2.n_traj = nc;
        if (launch_dwell_forward(p2, call.st)) return fail(BILD_ERR_HIP, "launch of the forward pass on the second prior block failed");
    }
    return BILD_OK;
}

int DwellCall::read_back(CallFrame &call, int nc)
{
    HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * 2 * 8, hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipMemcpyAsync(n_nan.data(), p.n_nan, (size_t)nc * sizeof(long long), hipMemcpyDeviceToHost, call.st));
    HIP_TRY(hipStreamSynchronize(call.st));
    return BILD_OK;
}

} // namespace bild

extern "C" int bild_gauss_dwell_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                         const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                         unsigned flags, int64_t scratch_bytes, bild_dwell_out *out)
{
    DwellCall rec;      // (before the frame, with the host copies below: asynchronous copies write them)
    std::vector<double> post, jumps, stay;
    std::vector<uint8_t> states;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    if (rec.n_traj == 0) return BILD_OK;
    const bool stats = out->log_post != nullptr;    // log_post == NULL: the forward pass alone
    const int S = rec.S, Tm = rec.Tm;

    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, stats ? kDwellForward | kDwellBackward | kDwellStats : kDwellForward, 0));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk, ld = p.ld;
    const int64_t slot = p.slot;

    if (stats) {
        post.resize((size_t)chunk * slot);
        jumps.resize((size_t)chunk * S * S);
        stay.resize((size_t)chunk * S);
    }
    states.resize((size_t)chunk * Tm);
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        if (stats) {
            if (launch_dwell_cover(p, st) || launch_dwell_carry(p, st) || launch_dwell_counts(p, st))
                return fail(BILD_ERR_HIP, "launch of the statistics of the dwell-time recursion failed");
            HIP_TRY(hipMemcpyAsync(post.data(), p.post, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(jumps.data(), p.jumps, (size_t)nc * S * S * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(stay.data(), p.stay, (size_t)nc * S * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(states.data(), p.map_states, (size_t)nc * Tm, hipMemcpyDeviceToHost, st));
        BILD_TRY(rec.read_back(call, nc));

        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = rec.T[jt];
            const DwellVerdict v = rec.verdict(i);
            if (out->logev) out->logev[jt] = v.logev;
            if (out->map_logjoint) out->map_logjoint[jt] = rec.fin[2 * i + 1];
            if (out->n_nan_windows) out->n_nan_windows[jt] = rec.n_nan[i];
            if (out->map_states) {
                uint8_t *row = out->map_states + (size_t)jt * T_max;
                for (int t = 0; t < T_max; ++t) row[t] = t < Tj ? states[(size_t)i * Tm + t] : 255;
            }
            if (stats) {
                double *lp = out->log_post + (size_t)jt * S * T_max;
                for (int s = 0; s < S; ++s)
                    for (int t = 0; t < T_max; ++t)
                        lp[(size_t)s * T_max + t] = v.usable && t < Tj ? std::log(post[(size_t)i * slot + (size_t)s * ld + t]) : nan;
            }
            if (stats && out->exp_jumps)
                for (int e = 0; e < S * S; ++e) out->exp_jumps[(size_t)jt * S * S + e] = v.usable ? jumps[(size_t)i * S * S + e] : nan;
            if (stats && out->exp_stay)
                for (int s = 0; s < S; ++s) out->exp_stay[(size_t)jt * S + s] = v.usable ? stay[(size_t)i * S + s] : nan;
        }
    }
    return BILD_OK;
}
