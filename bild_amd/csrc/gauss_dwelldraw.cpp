// Exact posterior draws of profiles under a dwell-time prior (include/bild_amd.h, "exact posterior draws under a dwell-time
// prior"): the refusals of the recursion, the frame, the prior's upload, the beta and gamma tables and
// the backward pass of gauss_dwell.hip through DwellCall (gauss_dwell.h), here over the trajectories that a draw names
// (gauss_draws.h: the draws grouped by trajectory, the upload of their descriptors); the refusals about the draws and the
// draw kernels on the set's stream.  Kernels: gauss_dwelldraw.hip.
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
    DwellCall rec;      // the backward half of the recursion alone
    BILD_TRY(rec.check(m, ts, L, log_init, log_jump, log_dwell, log_surv, T_max, 0u, scratch_bytes, out));
    BILD_TRY(draws_check_count(n_draws));
    if (U < 0) return fail(BILD_ERR_INVALID, "U = %d is negative", U);
    if (uniforms && U < 1) return fail(BILD_ERR_INVALID, "U = %d: a replay needs at least one uniform a draw", U);
    if (n_draws == 0) return BILD_OK;
    if (!draw_traj) return fail(BILD_ERR_INVALID, "draw_traj is NULL");
    const int n = (int)n_draws;
    DrawGroups g;       // (its vectors, and the parameter blocks below, outlive the stream's work: declared before the frame)
    BILD_TRY(g.group(rec.n_traj, rec.T, n, draw_traj, nullptr, 0, uniforms, U));
    const int n_used = (int)g.used.size();
    rec.over(n_used, g.Tm);     // the chunks run over the trajectories that a draw names

    std::vector<DwelldrawParams> blocks;    // the draw kernel's parameters, one block per chunk
    CallFrame call;
    // a trajectory's share of the chunk: beta, gamma and the head's pair
    BILD_TRY(rec.open(call, m, ts, kDwellBackward, 16));
    hipStream_t st = call.st;
    const int chunk = rec.chunk;
    blocks.resize((n_used + chunk - 1) / chunk);

    const DwellParams &bp = rec.p;
    DwelldrawParams p{};
    double *d_u = nullptr;
    int64_t *d_stream = nullptr;
    DwelldrawParams *d_blocks = nullptr;
    const bool keep = out->uniforms_out && U > 0;
    BILD_TRY(call.alloc(&d_blocks, blocks.size()));
    BILD_TRY(call.alloc(&p.head, (size_t)chunk * 2));
    if (draw_stream) BILD_TRY(call.alloc(&d_stream, (size_t)n));
    if (out->states) BILD_TRY(call.alloc(&p.states, (size_t)n * T_max));
    BILD_TRY(call.alloc(&p.n_switches, (size_t)n));
    BILD_TRY(call.alloc(&p.n_uniforms, (size_t)n));
    BILD_TRY(call.alloc(&p.logl, (size_t)n));
    BILD_TRY(call.alloc(&p.log_prior, (size_t)n));
    if (uniforms) BILD_TRY(call.alloc(&d_u, (size_t)n * U));
    if (keep) BILD_TRY(call.alloc(&p.uniforms_out, (size_t)n * U));

    BILD_TRY(g.upload(call, rec.n_traj));
    if (draw_stream) HIP_TRY(hipMemcpyAsync(d_stream, draw_stream, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (uniforms) HIP_TRY(hipMemcpyAsync(d_u, uniforms, (size_t)n * U * 8, hipMemcpyHostToDevice, st));
    if (keep) HIP_TRY(hipMemsetAsync(p.uniforms_out, 0, (size_t)n * U * 8, st));

    p.log_init = bp.log_init;
    p.log_jump = bp.log_jump;
    p.log_dwell = bp.log_dwell;
    p.log_surv = bp.log_surv;
    p.beta = bp.beta;
    p.gamma = bp.gamma;
    p.slot = bp.slot;
    p.S = bp.S;
    p.L = bp.L;
    p.ld = bp.ld;
    p.stream = d_stream;
    p.uniforms = d_u;
    p.seed = seed;
    p.U = U;
    p.T_max = T_max;

    for (int u0 = 0; u0 < n_used; u0 += chunk) {
        const int nc = std::min(chunk, n_used - u0);
        int i0 = 0, ni = 0;
        BILD_TRY(g.chunk(call, u0, nc, &i0, &ni));
        BILD_TRY(rec.run(call, g.d_used + u0, nc));
        p.trajs = g.d_used + u0;
        p.n_traj = nc;
        p.order = g.d_order + i0;
        p.slot_of = g.d_slot + i0;
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
