// Exact posterior draws of profiles (include/bild_amd.h, "exact posterior draws"): the refusals of the
// recursion, the frame, the transitions' upload, the beta and gamma tables and the backward recursion (segdp_run_backward)
// through SegdpCall (gauss_segdp.h), here over the trajectories that a draw names (gauss_draws.h: the draws grouped by
// trajectory, the upload of their descriptors); the refusals about the draws and the draw kernel on the set's stream.
// Kernels: gauss_segdraw.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_draws.h"
#include "gauss_segdraw.h"

extern "C" int bild_gauss_segment_draw(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max, const uint8_t *transitions,
                                       int T_max, int64_t scratch_bytes, int64_t n_draws, const int32_t *draw_traj, const int32_t *draw_k,
                                       const double *uniforms, uint64_t seed, bild_segdraw_out *out)
{
    SegdpCall rec;      // the backward half of the recursion alone
    BILD_TRY(rec.check(m, ts, k_max, transitions, T_max, 0u, scratch_bytes, out));
    BILD_TRY(draws_check_count(n_draws));
    if (n_draws == 0) return BILD_OK;
    if (!draw_traj || !draw_k) return fail(BILD_ERR_INVALID, "draw_traj or draw_k is NULL");
    if (!out->seg_start || !out->seg_state || !out->logl) return fail(BILD_ERR_INVALID, "seg_start, seg_state or logl is NULL");
    const int n = (int)n_draws, K = rec.K, U = std::max(1, 2 * k_max);
    DrawGroups g;       // (its vectors, and the parameter blocks below, outlive the stream's work: declared before the frame)
    BILD_TRY(g.group(rec.n_traj, rec.T, n, draw_traj, draw_k, k_max, uniforms, U));
    const int n_used = (int)g.used.size();
    rec.over(n_used, g.Tm);     // the chunks run over the trajectories that a draw names

    std::vector<SegdrawParams> blocks;      // the draw kernel's parameters, one block per chunk
    CallFrame call;
    // a trajectory's share of the chunk: beta and gamma, (M, Z) each, and the heads
    BILD_TRY(rec.open(call, m, ts, kSegdpBackward, (int64_t)K * 16));
    hipStream_t st = call.st;
    const int chunk = rec.chunk;
    blocks.resize((n_used + chunk - 1) / chunk);

    const SegdpParams &bp = rec.p;
    SegdrawParams p{};
    int32_t *d_k = nullptr;
    double *d_u = nullptr;
    SegdrawParams *d_blocks = nullptr;
    BILD_TRY(call.alloc(&d_blocks, blocks.size()));
    BILD_TRY(call.alloc(&p.head, (size_t)chunk * K * 2));
    BILD_TRY(call.alloc(&d_k, (size_t)n));
    BILD_TRY(call.alloc(&p.seg_start, (size_t)n * K));
    BILD_TRY(call.alloc(&p.seg_state, (size_t)n * K));
    BILD_TRY(call.alloc(&p.logl, (size_t)n));
    if (uniforms) BILD_TRY(call.alloc(&d_u, (size_t)n * U));
    if (out->uniforms_out) BILD_TRY(call.alloc(&p.uniforms_out, (size_t)n * U));

    BILD_TRY(g.upload(call, rec.n_traj));
    HIP_TRY(hipMemcpyAsync(d_k, draw_k, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (uniforms) HIP_TRY(hipMemcpyAsync(d_u, uniforms, (size_t)n * U * 8, hipMemcpyHostToDevice, st));
    if (p.uniforms_out) HIP_TRY(hipMemsetAsync(p.uniforms_out, 0, (size_t)n * U * 8, st));

    p.tr = bp.tr;
    p.beta = bp.beta;
    p.gamma = bp.gamma;
    p.draw_k = d_k;
    p.uniforms = d_u;
    p.seed = seed;
    p.slot = bp.slot;
    p.S = bp.S;
    p.K = K;
    p.ld = bp.ld;
    p.U = U;

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
        HIP_TRY(hipMemcpyAsync(d_blocks + c, &blocks[c], sizeof(SegdrawParams), hipMemcpyHostToDevice, st));
        if (launch_segdraw_head(p, st) || launch_segdraw(p, d_blocks + c, st)) return fail(BILD_ERR_HIP, "launch of the draw kernels failed");
    }
    HIP_TRY(hipMemcpyAsync(out->seg_start, p.seg_start, (size_t)n * K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->seg_state, p.seg_state, (size_t)n * K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->logl, p.logl, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (p.uniforms_out) HIP_TRY(hipMemcpyAsync(out->uniforms_out, p.uniforms_out, (size_t)n * U * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BILD_OK;
}
