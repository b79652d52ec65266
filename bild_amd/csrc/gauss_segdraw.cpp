// Exact posterior draws of profiles (include/bild_amd.h, "exact posterior draws"): the refusals, the
// draws grouped by trajectory (gauss_draws.h), the chunks of whole trajectories, the backward recursion of the evidence
// (segdp_run_backward) and the draw kernel on the set's stream.  Kernels: gauss_segdraw.hip.
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
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    const int S = m->S;
    BILD_TRY(segdp_check_call(S, k_max, 0u, transitions, scratch_bytes, n_traj, T, T_max));
    BILD_TRY(draws_check_count(n_draws));
    if (n_draws == 0) return BILD_OK;
    if (!draw_traj || !draw_k) return fail(BILD_ERR_INVALID, "draw_traj or draw_k is NULL");
    if (!out->seg_start || !out->seg_state || !out->logl) return fail(BILD_ERR_INVALID, "seg_start, seg_state or logl is NULL");
    const int n = (int)n_draws, K = k_max + 1, U = std::max(1, 2 * k_max);
    DrawGroups g;       // (its vectors, and the host copies below, outlive the stream's work: declared before the frame)
    BILD_TRY(g.group(n_traj, T, n, draw_traj, draw_k, k_max, uniforms, U));
    const int n_used = (int)g.used.size(), Tm = g.Tm;
    const int ld = Tm + 1;
    const int64_t slot = (int64_t)K * S * ld;

    std::vector<GaussTraj> all(n_traj), mine(n_used);
    std::vector<SegdrawParams> blocks;      // the draw kernel's parameters, one block per chunk
    CallFrame call;
    BILD_TRY(call.open(m, ts));
    hipStream_t st = call.st;

    // a trajectory's share of the chunk: beta and gamma, (M, Z) each, and the heads
    int chunk = 0;
    BILD_TRY(call.chunk_of(slot * 4 * 8 + (int64_t)K * 16, scratch_bytes, n_used, &chunk));
    blocks.resize((n_used + chunk - 1) / chunk);

    SegdpParams bp{};
    SegdrawParams p{};
    uint8_t *d_tr = nullptr;
    GaussTraj *d_used = nullptr;
    int32_t *d_order = nullptr, *d_slot = nullptr, *d_k = nullptr;
    double *d_u = nullptr;
    SegdrawParams *d_blocks = nullptr;
    BILD_TRY(call.alloc(&d_blocks, blocks.size()));
    BILD_TRY(call.alloc(&d_tr, (size_t)S * S));
    BILD_TRY(call.alloc(&d_used, (size_t)n_used));
    BILD_TRY(call.alloc(&bp.beta.M, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&bp.beta.Z, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&bp.gamma.M, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&bp.gamma.Z, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.head, (size_t)chunk * K * 2));
    BILD_TRY(call.alloc(&d_order, (size_t)n));
    BILD_TRY(call.alloc(&d_slot, (size_t)n));
    BILD_TRY(call.alloc(&d_k, (size_t)n));
    BILD_TRY(call.alloc(&p.seg_start, (size_t)n * K));
    BILD_TRY(call.alloc(&p.seg_state, (size_t)n * K));
    BILD_TRY(call.alloc(&p.logl, (size_t)n));
    if (uniforms) BILD_TRY(call.alloc(&d_u, (size_t)n * U));
    if (out->uniforms_out) BILD_TRY(call.alloc(&p.uniforms_out, (size_t)n * U));

    HIP_TRY(hipMemcpy(all.data(), call.d_trajs, (size_t)n_traj * sizeof(GaussTraj), hipMemcpyDeviceToHost));
    for (int u = 0; u < n_used; ++u) mine[u] = all[g.used[u]];
    HIP_TRY(hipMemcpyAsync(d_used, mine.data(), (size_t)n_used * sizeof(GaussTraj), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tr, transitions, (size_t)S * S, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_order, g.order.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_k, draw_k, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (uniforms) HIP_TRY(hipMemcpyAsync(d_u, uniforms, (size_t)n * U * 8, hipMemcpyHostToDevice, st));
    if (p.uniforms_out) HIP_TRY(hipMemsetAsync(p.uniforms_out, 0, (size_t)n * U * 8, st));

    bp.tr = d_tr;
    bp.slot = slot;
    bp.S = S;
    bp.K = K;
    bp.Tm = Tm;
    bp.ld = ld;
    p.tr = d_tr;
    p.beta = bp.beta;
    p.gamma = bp.gamma;
    p.draw_k = d_k;
    p.uniforms = d_u;
    p.seed = seed;
    p.slot = slot;
    p.S = S;
    p.K = K;
    p.ld = ld;
    p.U = U;

    for (int u0 = 0; u0 < n_used; u0 += chunk) {
        const int nc = std::min(chunk, n_used - u0);
        int i0 = 0, ni = 0;
        g.chunk(u0, nc, &i0, &ni);
        HIP_TRY(hipMemcpyAsync(d_slot + i0, g.slot_of.data() + i0, (size_t)ni * 4, hipMemcpyHostToDevice, st));
        bp.trajs = p.trajs = d_used + u0;
        bp.n_traj = p.n_traj = nc;
        BILD_TRY(segdp_run_backward(bp, k_max, st));
        p.order = d_order + i0;
        p.slot_of = d_slot + i0;
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
