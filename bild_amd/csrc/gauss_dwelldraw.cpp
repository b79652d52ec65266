// Exact posterior draws of profiles under a dwell-time prior (include/bild_amd.h, "exact posterior draws under a dwell-time
// prior"): the refusals, the draws grouped by trajectory, the chunks of whole trajectories, the backward
// pass of gauss_dwell.hip and the draw kernels on the set's stream.  Kernels: gauss_dwelldraw.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "likelihood.h"
#include "gauss_dwelldraw.h"
#include "internal.h"

namespace {

using namespace bild;

#define DD_TRY(x)                       \
    do {                                \
        int rc_ = (x);                  \
        if (rc_ != BILD_OK) return rc_; \
    } while (0)

// Device memory of one call, freed on every path
struct Bufs {
    std::vector<void *> ptrs;
    ~Bufs()
    {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class X> int alloc(X **out, size_t count)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(X));
        if (e != hipSuccess) return fail(BILD_ERR_NOMEM, "hipMalloc(%zu) failed: %s", count * sizeof(X), hipGetErrorString(e));
        ptrs.push_back(p);
        *out = static_cast<X *>(p);
        return BILD_OK;
    }
};

} // namespace

extern "C" int bild_gauss_dwell_draw(const bild_gauss_model *m, const bild_gauss_trajset *ts, int L, const double *log_init,
                                     const double *log_jump, const double *log_dwell, const double *log_surv, int T_max,
                                     int64_t scratch_bytes, int64_t n_draws, const int32_t *draw_traj, const int64_t *draw_stream, int U,
                                     const double *uniforms, uint64_t seed, bild_dwelldraw_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    DD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    const int S = m->S;
    DD_TRY(dwell_check_call(S, L, log_init, log_jump, log_dwell, log_surv, n_traj, T, T_max, scratch_bytes));
    if (n_draws < 0 || n_draws > std::numeric_limits<int32_t>::max())
        return fail(BILD_ERR_INVALID, "n_draws = %lld: between 0 and 2^31 - 1", (long long)n_draws);
    if (U < 0) return fail(BILD_ERR_INVALID, "U = %d is negative", U);
    if (uniforms && U < 1) return fail(BILD_ERR_INVALID, "U = %d: a replay needs at least one uniform a draw", U);
    if (n_draws == 0) return BILD_OK;
    if (!draw_traj) return fail(BILD_ERR_INVALID, "draw_traj is NULL");
    const int n = (int)n_draws;
    for (int r = 0; r < n; ++r)
        if (draw_traj[r] < 0 || draw_traj[r] >= n_traj)
            return fail(BILD_ERR_INVALID, "draw_traj[%d] = %d: the set has %d trajectories", r, draw_traj[r], n_traj);
    if (uniforms)
        for (int64_t i = 0; i < (int64_t)n * U; ++i)
            if (!(uniforms[i] >= 0.0 && uniforms[i] < 1.0))
                return fail(BILD_ERR_INVALID, "uniforms[%lld, %lld] = %g: outside [0, 1)", (long long)(i / U), (long long)(i % U), uniforms[i]);

    // the trajectories that a draw names, ascending, and the draws grouped by them (within a trajectory: in the call's order)
    std::vector<int> rank(n_traj, -1), used;
    for (int r = 0; r < n; ++r) rank[draw_traj[r]] = 0;
    for (int j = 0; j < n_traj; ++j)
        if (rank[j] == 0) {
            rank[j] = (int)used.size();
            used.push_back(j);
        }
    const int n_used = (int)used.size();
    std::vector<int32_t> order(n), slot_of(n);
    std::vector<int> first(n_used + 1, 0);
    for (int r = 0; r < n; ++r) ++first[rank[draw_traj[r]] + 1];
    for (int u = 0; u < n_used; ++u) first[u + 1] += first[u];
    {
        std::vector<int> fill(first.begin(), first.end() - 1);
        for (int r = 0; r < n; ++r) order[fill[rank[draw_traj[r]]]++] = r;
    }
    int Tm = 1;
    for (int j : used) Tm = std::max(Tm, T[j]);
    const int ld = Tm + 1;
    const int64_t slot = (int64_t)S * ld;

    const GaussTraj *d_trajs = nullptr;
    void *stream = nullptr;
    std::mutex *mu = nullptr;
    DD_TRY(internal_gauss_set_device(m, ts, &d_trajs, &stream, &mu));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(*mu);      // the set's stream: one call at a time

    // chunks of whole trajectories within the budget (at least one): beta, gamma and the head's pair
    const int64_t per_traj = slot * 2 * 8 + 16;
    int64_t budget = scratch_bytes;
    if (budget == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<int64_t>((int64_t)1 << 30, (int64_t)(free_b / 3));
    }
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(budget / per_traj, n_used));

    std::vector<GaussTraj> all(n_traj), mine(n_used);      // (host copies outlive the stream's work: declared before Drain)
    std::vector<DwelldrawParams> blocks((n_used + chunk - 1) / chunk);      // the draw kernel's parameters, one block per chunk
    const size_t n_prior = (size_t)S + (size_t)S * S + 2 * (size_t)S * L;
    std::vector<double> prior(n_prior);
    Bufs bufs;
    struct Drain {      // (declared after the buffers: on an error path the stream is drained before they are freed)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    DwellParams bp{};
    DwelldrawParams p{};
    double *d_prior = nullptr, *d_beta = nullptr, *d_gamma = nullptr, *d_u = nullptr;
    GaussTraj *d_used = nullptr;
    int32_t *d_order = nullptr, *d_slot = nullptr;
    int64_t *d_stream = nullptr;
    DwelldrawParams *d_blocks = nullptr;
    const bool keep = out->uniforms_out && U > 0;
    DD_TRY(bufs.alloc(&d_blocks, blocks.size()));
    DD_TRY(bufs.alloc(&d_prior, n_prior));
    DD_TRY(bufs.alloc(&d_used, (size_t)n_used));
    DD_TRY(bufs.alloc(&d_beta, (size_t)chunk * slot));
    DD_TRY(bufs.alloc(&d_gamma, (size_t)chunk * slot));
    DD_TRY(bufs.alloc(&p.head, (size_t)chunk * 2));
    DD_TRY(bufs.alloc(&d_order, (size_t)n));
    DD_TRY(bufs.alloc(&d_slot, (size_t)n));
    if (draw_stream) DD_TRY(bufs.alloc(&d_stream, (size_t)n));
    if (out->states) DD_TRY(bufs.alloc(&p.states, (size_t)n * T_max));
    DD_TRY(bufs.alloc(&p.n_switches, (size_t)n));
    DD_TRY(bufs.alloc(&p.n_uniforms, (size_t)n));
    DD_TRY(bufs.alloc(&p.logl, (size_t)n));
    DD_TRY(bufs.alloc(&p.log_prior, (size_t)n));
    if (uniforms) DD_TRY(bufs.alloc(&d_u, (size_t)n * U));
    if (keep) DD_TRY(bufs.alloc(&p.uniforms_out, (size_t)n * U));

    std::copy_n(log_init, S, prior.data());
    std::copy_n(log_jump, (size_t)S * S, prior.data() + S);
    std::copy_n(log_dwell, (size_t)S * L, prior.data() + S + S * S);
    std::copy_n(log_surv, (size_t)S * L, prior.data() + S + S * S + (size_t)S * L);
    HIP_TRY(hipMemcpy(all.data(), d_trajs, (size_t)n_traj * sizeof(GaussTraj), hipMemcpyDeviceToHost));
    for (int u = 0; u < n_used; ++u) mine[u] = all[used[u]];
    HIP_TRY(hipMemcpyAsync(d_used, mine.data(), (size_t)n_used * sizeof(GaussTraj), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_prior, prior.data(), n_prior * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_order, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (draw_stream) HIP_TRY(hipMemcpyAsync(d_stream, draw_stream, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (uniforms) HIP_TRY(hipMemcpyAsync(d_u, uniforms, (size_t)n * U * 8, hipMemcpyHostToDevice, st));
    if (keep) HIP_TRY(hipMemsetAsync(p.uniforms_out, 0, (size_t)n * U * 8, st));

    bp.log_init = p.log_init = d_prior;
    bp.log_jump = p.log_jump = d_prior + S;
    bp.log_dwell = p.log_dwell = d_prior + S + S * S;
    bp.log_surv = p.log_surv = p.log_dwell + (size_t)S * L;
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
        for (int u = u0; u < u0 + nc; ++u)
            for (int i = first[u]; i < first[u + 1]; ++i) slot_of[i] = u - u0;
        const int i0 = first[u0], ni = first[u0 + nc] - i0;
        HIP_TRY(hipMemcpyAsync(d_slot + i0, slot_of.data() + i0, (size_t)ni * 4, hipMemcpyHostToDevice, st));
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
