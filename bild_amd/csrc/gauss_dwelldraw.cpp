// Exact posterior draws of profiles under a dwell-time prior (include/bild_amd.h, "exact posterior draws under a dwell-time
// prior"): the refusals, the draws grouped by trajectory (gauss_draws.h), the chunks of whole
// trajectories, the prior's upload (dwell_upload_prior), the backward pass of gauss_dwell.hip and the draw kernels on the
// set's stream.  Kernels: gauss_dwelldraw.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_draws.h"
#include "gauss_dwelldraw.h"

extern "C" int bild_gauss_dwell_draw(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                     const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                     int64_t scratch_bytes, int64_t n_draws, const int32_t *draw_traj, const int64_t *draw_stream, int U,
                                     const double *uniforms, uint64_t seed, bild_dwelldraw_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    const int S = m->S;
    BILD_TRY(dwell_check_call(S, L, log_init, log_jump, log_dwell, log_surv, n_traj, T, T_max, scratch_bytes));
    BILD_TRY(draws_check_count(n_draws));
    if (U < 0) return fail(BILD_ERR_INVALID, "U = %d is negative", U);
    if (uniforms && U < 1) return fail(BILD_ERR_INVALID, "U = %d: a replay needs at least one uniform a draw", U);
    if (n_draws == 0) return BILD_OK;
    if (!draw_traj) return fail(BILD_ERR_INVALID, "draw_traj is NULL");
    const int n = (int)n_draws;
    DrawGroups g;       // (its vectors, and the host copies below, outlive the stream's work: declared before the frame)
    BILD_TRY(g.group(n_traj, T, n, draw_traj, nullptr, 0, uniforms, U));
    const int n_used = (int)g.used.size(), Tm = g.Tm;
    const int ld = Tm + 1;
    const int64_t slot = (int64_t)S * ld;

    std::vector<GaussTraj> all(n_traj), mine(n_used);
    std::vector<DwelldrawParams> blocks;    // the draw kernel's parameters, one block per chunk
    CallFrame call;
    BILD_TRY(call.open(m, ts));
    hipStream_t st = call.st;

    // a trajectory's share of the chunk: beta, gamma and the head's pair
    int chunk = 0;
    BILD_TRY(call.chunk_of(slot * 2 * 8 + 16, scratch_bytes, n_used, &chunk));
    blocks.resize((n_used + chunk - 1) / chunk);

    DwellParams bp{};
    DwelldrawParams p{};
    DwellPrior dp{};
    double *d_beta = nullptr, *d_gamma = nullptr, *d_u = nullptr;
    GaussTraj *d_used = nullptr;
    int32_t *d_order = nullptr, *d_slot = nullptr;
    int64_t *d_stream = nullptr;
    DwelldrawParams *d_blocks = nullptr;
    const bool keep = out->uniforms_out && U > 0;
    BILD_TRY(call.alloc(&d_blocks, blocks.size()));
    BILD_TRY(dwell_upload_prior(call, S, L, log_init, log_jump, log_dwell, log_surv, &dp));
    BILD_TRY(call.alloc(&d_used, (size_t)n_used));
    BILD_TRY(call.alloc(&d_beta, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&d_gamma, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.head, (size_t)chunk * 2));
    BILD_TRY(call.alloc(&d_order, (size_t)n));
    BILD_TRY(call.alloc(&d_slot, (size_t)n));
    if (draw_stream) BILD_TRY(call.alloc(&d_stream, (size_t)n));
    if (out->states) BILD_TRY(call.alloc(&p.states, (size_t)n * T_max));
    BILD_TRY(call.alloc(&p.n_switches, (size_t)n));
    BILD_TRY(call.alloc(&p.n_uniforms, (size_t)n));
    BILD_TRY(call.alloc(&p.logl, (size_t)n));
    BILD_TRY(call.alloc(&p.log_prior, (size_t)n));
    if (uniforms) BILD_TRY(call.alloc(&d_u, (size_t)n * U));
    if (keep) BILD_TRY(call.alloc(&p.uniforms_out, (size_t)n * U));

    HIP_TRY(hipMemcpy(all.data(), call.d_trajs, (size_t)n_traj * sizeof(GaussTraj), hipMemcpyDeviceToHost));
    for (int u = 0; u < n_used; ++u) mine[u] = all[g.used[u]];
    HIP_TRY(hipMemcpyAsync(d_used, mine.data(), (size_t)n_used * sizeof(GaussTraj), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_order, g.order.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (draw_stream) HIP_TRY(hipMemcpyAsync(d_stream, draw_stream, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (uniforms) HIP_TRY(hipMemcpyAsync(d_u, uniforms, (size_t)n * U * 8, hipMemcpyHostToDevice, st));
    if (keep) HIP_TRY(hipMemsetAsync(p.uniforms_out, 0, (size_t)n * U * 8, st));

    bp.log_init = p.log_init = dp.log_init;
    bp.log_jump = p.log_jump = dp.log_jump;
    bp.log_dwell = p.log_dwell = dp.log_dwell;
    bp.log_surv = p.log_surv = dp.log_surv;
    bp.beta = d_beta;
    bp.gamma = d_gamma;
    p.beta = d_beta;
    p.gamma = d_gamma;
    bp.slot = p.slot = slot;
    bp.S = p.S = S;
    bp.L = p.L = L;
    bp.Tm = Tm;
    bp.ld = p.ld = ld;
    bp.ntile = (Tm + kDwellTile - 1) / kDwellTile;
    p.stream = d_stream;
    p.uniforms = d_u;
    p.seed = seed;
    p.U = U;
    p.T_max = T_max;

    for (int u0 = 0; u0 < n_used; u0 += chunk) {
        const int nc = std::min(chunk, n_used - u0);
        int i0 = 0, ni = 0;
        g.chunk(u0, nc, &i0, &ni);
        HIP_TRY(hipMemcpyAsync(d_slot + i0, g.slot_of.data() + i0, (size_t)ni * 4, hipMemcpyHostToDevice, st));
        bp.trajs = p.trajs = d_used + u0;
        bp.n_traj = p.n_traj = nc;
        if (launch_dwell_backward(bp, st)) return fail(BILD_ERR_HIP, "launch of the backward pass of the dwell-time recursion failed");
        p.order = d_order + i0;
        p.slot_of = d_slot + i0;
        p.n_draws = ni;
        const size_t c = (size_t)(u0 / chunk);
        blocks[c] = p;
        HIP_TRY(hipMemcpyAsync(d_blocks + c, &blocks[c], sizeof(DwelldrawParams), hipMemcpyHostToDevice, st));
        if (launch_dwelldraw_head(p, st) || launch_dwelldraw(p, d_blocks + c, st)) return fail(BILD_ERR_HIP, "launch of the draw kernels failed");
    }
    if (out->states) HIP_TRY(hipMemcpyAsync(out->states, p.states, (size_t)n * T_max, hipMemcpyDeviceToHost, st));
    if (out->n_switches) HIP_TRY(hipMemcpyAsync(out->n_switches, p.n_switches, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (out->logl) HIP_TRY(hipMemcpyAsync(out->logl, p.logl, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (out->log_prior) HIP_TRY(hipMemcpyAsync(out->log_prior, p.log_prior, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (out->n_uniforms) HIP_TRY(hipMemcpyAsync(out->n_uniforms, p.n_uniforms, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (keep) HIP_TRY(hipMemcpyAsync(out->uniforms_out, p.uniforms_out, (size_t)n * U * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BILD_OK;
}
