// Exact window support under a dwell-time prior (include/bild_amd_windows.h): the forward and the
// backward pass of the dwell-time recursion through DwellCall (gauss_dwell.h), as bild_gauss_dwell_evidence runs them, so that
// logev and n_nan_windows are the same numbers and the NaN rule the same; the refusals about the windows, the queries of a
// chunk's trajectories and one launch of the window kernel over them.  Kernel: gauss_dwellwin.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "../../include/bild_amd_windows.h"
#include "gauss_call.h"
#include "gauss_dwellwin.h"

extern "C" int bild_gauss_dwell_windows(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                        const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                        int64_t scratch_bytes, int64_t n_win, const int32_t *win_traj, const int32_t *win_u,
                                        const int32_t *win_v, const uint32_t *win_target, unsigned flags, bild_dwell_windows_out *out)
{
    using namespace bild;
    DwellCall rec;      // (before the frame, with the host copies below: asynchronous copies read and write them)
    std::vector<DwellWinQuery> queries;
    std::vector<double> num;
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, flags, scratch_bytes, out));
    if (n_win < 0 || n_win > std::numeric_limits<int32_t>::max()) return fail(BILD_ERR_INVALID, "n_win = %lld: between 0 and 2^31 - 1", (long long)n_win);
    if (n_win > 0 && (!win_traj || !win_u || !win_v || !win_target)) return fail(BILD_ERR_INVALID, "win_traj, win_u, win_v or win_target is NULL");
    const int S = rec.S, n = (int)n_win;
    const unsigned all = (1u << S) - 1u;
    for (int i = 0; i < n; ++i) {
        const int j = win_traj[i];
        if (j < 0 || j >= rec.n_traj) return fail(BILD_ERR_INVALID, "win_traj[%d] = %d: the set has %d trajectories", i, j, rec.n_traj);
        if (i > 0 && j < win_traj[i - 1]) return fail(BILD_ERR_INVALID, "win_traj[%d] = %d after %d: win_traj must not decrease", i, j, win_traj[i - 1]);
        if (win_u[i] < 0 || win_u[i] >= win_v[i] || win_v[i] > rec.T[j])
            return fail(BILD_ERR_INVALID, "window %d = [%d, %d): 0 <= u < v <= T = %d of trajectory %d expected", i, win_u[i], win_v[i], rec.T[j], j);
        const unsigned g = win_target[i];
        if (g == 0 || (g & ~all) || g == all)
            return fail(BILD_ERR_INVALID, "win_target[%d] = 0x%x: a non-empty proper subset of the %d states, bit s for state s", i, g, S);
    }
    if (rec.n_traj == 0) return BILD_OK;

    // a trajectory's share of a chunk beside the tables: the kappa rows, the descriptors and the outputs of its queries; the
    // chunks are sized by the set's largest
    const auto row = [&](int i) { return (int64_t)S * (win_v[i] - win_u[i] - 1); };
    int64_t own = 0;
    for (int i = 0, i1 = 0; i < n; i = i1) {
        int64_t bytes = 0;
        for (i1 = i; i1 < n && win_traj[i1] == win_traj[i]; ++i1) bytes += row(i1) * 8 + (int64_t)sizeof(DwellWinQuery) + 8;
        own = std::max(own, bytes);
    }

    DwellWindows o{};
    CallFrame call;
    BILD_TRY(rec.open(call, m, ts, kDwellForward | kDwellBackward, own));
    hipStream_t st = call.st;
    const DwellParams &p = rec.p;
    const int chunk = rec.chunk;

    // the queries, chunk by chunk: the slot of the trajectory and the kappa row inside the chunk
    queries.resize((size_t)n);
    num.resize((size_t)n);
    int64_t kappa_top = 0;
    for (int j0 = 0, i = 0; j0 < rec.n_traj; j0 += chunk) {
        int64_t at = 0;
        for (; i < n && win_traj[i] < j0 + chunk; ++i) {
            queries[(size_t)i] = DwellWinQuery{win_traj[i] - j0, win_u[i], win_v[i], win_target[i], at};
            at += row(i);
        }
        kappa_top = std::max(kappa_top, at);
    }
    DwellWinQuery *d_queries = nullptr;
    double *d_num = nullptr;
    BILD_TRY(call.alloc(&d_queries, (size_t)n));
    BILD_TRY(call.alloc(&o.kappa, (size_t)kappa_top));
    BILD_TRY(call.alloc(&d_num, (size_t)n));
    if (n > 0) HIP_TRY(hipMemcpyAsync(d_queries, queries.data(), (size_t)n * sizeof(DwellWinQuery), hipMemcpyHostToDevice, st));
    const double nan = std::numeric_limits<double>::quiet_NaN();

    for (int j0 = 0, i0 = 0; j0 < rec.n_traj; j0 += chunk) {
        const int nc = std::min(chunk, rec.n_traj - j0);
        int i1 = i0;
        while (i1 < n && win_traj[i1] < j0 + nc) ++i1;
        BILD_TRY(rec.run(call, call.d_trajs + j0, nc));
        if (i1 > i0) {
            o.queries = d_queries + i0;
            o.num = d_num + i0;
            o.n = i1 - i0;
            if (launch_dwell_windows(p, o, st)) return fail(BILD_ERR_HIP, "launch of the window kernel failed");
            HIP_TRY(hipMemcpyAsync(num.data() + i0, d_num + i0, (size_t)(i1 - i0) * 8, hipMemcpyDeviceToHost, st));
        }
        BILD_TRY(rec.read_back(call, nc));

        for (int i = 0; i < nc; ++i) {
            const DwellVerdict v = rec.verdict(i);
            if (out->logev) out->logev[j0 + i] = v.logev;
            if (out->n_nan_windows) out->n_nan_windows[j0 + i] = rec.n_nan[i];
        }
        if (out->log_all)
            for (int i = i0; i < i1; ++i) {
                const DwellVerdict v = rec.verdict(win_traj[i] - j0);
                out->log_all[i] = v.usable ? num[(size_t)i] - v.logev : nan;
            }
        i0 = i1;
    }
    return BILD_OK;
}
