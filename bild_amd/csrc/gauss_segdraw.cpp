// Exact posterior draws of profiles (include/bild_amd.h, "exact posterior draws"): the refusals, the
// draws grouped by trajectory, the chunks of whole trajectories, the backward recursion of gauss_segdp.hip level after level
// and the draw kernel on the set's stream.  Kernels: gauss_segdraw.hip.
#include <algorithm>
#include <cmath>
#include <limits>
#include <numeric>

#include "likelihood.h"
#include "gauss_segdraw.h"
#include "internal.h"

namespace {

using namespace bild;

#define SW_TRY(x)                       \
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

extern "C" int bild_gauss_segment_draw(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max, const uint8_t *transitions,
                                       int T_max, int64_t scratch_bytes, int64_t n_draws, const int32_t *draw_traj, const int32_t *draw_k,
                                       const double *uniforms, uint64_t seed, bild_segdraw_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    SW_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (k_max < 0 || k_max > kSegdpMaxK)
        return fail(BILD_ERR_UNSUPPORTED, "k_max = %d: the segment recursion supports 0 <= k_max <= %d", k_max, kSegdpMaxK);
    const int S = m->S;
    if (!transitions) return fail(BILD_ERR_INVALID, "transitions is NULL");
    for (int i = 0; i < S * S; ++i)
        if (transitions[i] > 1) return fail(BILD_ERR_INVALID, "transitions[%d] = %d; must be 0 or 1", i, transitions[i]);
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    for (int j = 0; j < n_traj; ++j)
        if (T[j] > T_max) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames, more than T_max = %d", j, T[j], T_max);
    if (n_draws < 0 || n_draws > std::numeric_limits<int32_t>::max())
        return fail(BILD_ERR_INVALID, "n_draws = %lld: between 0 and 2^31 - 1", (long long)n_draws);
    if (n_draws == 0) return BILD_OK;
    if (!draw_traj || !draw_k) return fail(BILD_ERR_INVALID, "draw_traj or draw_k is NULL");
    if (!out->seg_start || !out->seg_state || !out->logl) return fail(BILD_ERR_INVALID, "seg_start, seg_state or logl is NULL");
    const int n = (int)n_draws, K = k_max + 1, U = std::max(1, 2 * k_max);
    for (int r = 0; r < n; ++r) {
        if (draw_traj[r] < 0 || draw_traj[r] >= n_traj)
            return fail(BILD_ERR_INVALID, "draw_traj[%d] = %d: the set has %d trajectories", r, draw_traj[r], n_traj);
        if (draw_k[r] < 0 || draw_k[r] > k_max) return fail(BILD_ERR_INVALID, "draw_k[%d] = %d: outside 0 .. k_max = %d", r, draw_k[r], k_max);
    }
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
    const int64_t slot = (int64_t)K * S * ld;

    const GaussTraj *d_trajs = nullptr;
    void *stream = nullptr;
    std::mutex *mu = nullptr;
    SW_TRY(internal_gauss_set_device(m, ts, &d_trajs, &stream, &mu));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(*mu);      // the set's stream: one call at a time

    // chunks of whole trajectories within the budget (at least one): beta and gamma, (M, Z) each, and the heads
    const int64_t per_traj = slot * 4 * 8 + (int64_t)K * 16;
    int64_t budget = scratch_bytes;
    if (budget == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<int64_t>((int64_t)1 << 30, (int64_t)(free_b / 3));
    }
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(budget / per_traj, n_used));

    std::vector<GaussTraj> all(n_traj), mine(n_used);      // (host copies outlive the stream's work: declared before Drain)
    std::vector<SegdrawParams> blocks((n_used + chunk - 1) / chunk);    // the draw kernel's parameters, one block per chunk
    Bufs bufs;
    struct Drain {      // (declared after the buffers: on an error path the stream is drained before they are freed)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    SegdpParams bp{};
    SegdrawParams p{};
    uint8_t *d_tr = nullptr;
    GaussTraj *d_used = nullptr;
    int32_t *d_order = nullptr, *d_slot = nullptr, *d_k = nullptr;
    double *d_u = nullptr;
    SegdrawParams *d_blocks = nullptr;
    SW_TRY(bufs.alloc(&d_blocks, blocks.size()));
    SW_TRY(bufs.alloc(&d_tr, (size_t)S * S));
    SW_TRY(bufs.alloc(&d_used, (size_t)n_used));
    SW_TRY(bufs.alloc(&bp.beta.M, (size_t)chunk * slot));
    SW_TRY(bufs.alloc(&bp.beta.Z, (size_t)chunk * slot));
    SW_TRY(bufs.alloc(&bp.gamma.M, (size_t)chunk * slot));
    SW_TRY(bufs.alloc(&bp.gamma.Z, (size_t)chunk * slot));
    SW_TRY(bufs.alloc(&p.head, (size_t)chunk * K * 2));
    SW_TRY(bufs.alloc(&d_order, (size_t)n));
    SW_TRY(bufs.alloc(&d_slot, (size_t)n));
    SW_TRY(bufs.alloc(&d_k, (size_t)n));
    SW_TRY(bufs.alloc(&p.seg_start, (size_t)n * K));
    SW_TRY(bufs.alloc(&p.seg_state, (size_t)n * K));
    SW_TRY(bufs.alloc(&p.logl, (size_t)n));
    if (uniforms) SW_TRY(bufs.alloc(&d_u, (size_t)n * U));
    if (out->uniforms_out) SW_TRY(bufs.alloc(&p.uniforms_out, (size_t)n * U));

    HIP_TRY(hipMemcpy(all.data(), d_trajs, (size_t)n_traj * sizeof(GaussTraj), hipMemcpyDeviceToHost));
    for (int u = 0; u < n_used; ++u) mine[u] = all[used[u]];
    HIP_TRY(hipMemcpyAsync(d_used, mine.data(), (size_t)n_used * sizeof(GaussTraj), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_tr, transitions, (size_t)S * S, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_order, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
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
        for (int u = u0; u < u0 + nc; ++u)
            for (int i = first[u]; i < first[u + 1]; ++i) slot_of[i] = u - u0;
        const int i0 = first[u0], ni = first[u0 + nc] - i0;
        HIP_TRY(hipMemcpyAsync(d_slot + i0, slot_of.data() + i0, (size_t)ni * 4, hipMemcpyHostToDevice, st));
        bp.trajs = p.trajs = d_used + u0;
        bp.n_traj = p.n_traj = nc;
        if (launch_segdp_init(bp, true, st)) return fail(BILD_ERR_HIP, "launch of the backward recursion's first level failed");
        for (int lv = 0; lv < k_max; ++lv)
            if (launch_segdp_blevel(bp, lv, st) || launch_segdp_bmix(bp, lv + 1, st))
                return fail(BILD_ERR_HIP, "launch of level %d of the backward recursion failed", lv);
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
