// The bookkeeping of a call that draws profiles (gauss_segdraw.cpp, gauss_dwelldraw.cpp): what it refuses about the draws,
// the draws grouped by the trajectory they name, so that a chunk of trajectories finds its draws in one run, and the device
// descriptors of the trajectories that a draw names.  Host only; private to the library.
#pragma once
#include <limits>

#include "gauss.h"
#include "gauss_call.h"

namespace bild {

inline int draws_check_count(int64_t n_draws)
{
    if (n_draws < 0 || n_draws > std::numeric_limits<int32_t>::max())
        return fail(BILD_ERR_INVALID, "n_draws = %lld: between 0 and 2^31 - 1", (long long)n_draws);
    return BILD_OK;
}

struct DrawGroups {
    std::vector<int> used;          // the trajectories that a draw names, ascending
    std::vector<int> first;         // the draws of used[u]: order[first[u]] .. order[first[u + 1] - 1]
    std::vector<int32_t> order;     // the draws grouped by trajectory; within a trajectory in the call's order
    std::vector<int32_t> slot_of;   // per place in `order`: the trajectory's place in its chunk (chunk())
    std::vector<GaussTraj> mine;    // the descriptors of `used` (upload(); an asynchronous copy reads them)
    const GaussTraj *d_used = nullptr;              // upload(): `mine` on the device; chunks run over it, not over the set
    const int32_t *d_order = nullptr;               // ... and `order`
    int32_t *d_slot = nullptr;                      // ... and room for `slot_of` (chunk())
    int Tm = 1;                     // the longest trajectory in `used`

    // Refuses, draw by draw, a draw_traj outside the set and (draw_k not NULL) a draw_k outside 0 .. k_max, then a replayed
    // uniform (n x U, or NULL) outside [0, 1); then groups the n draws.  A BILD_* code.
    int group(int n_traj, const int *T, int n, const int32_t *draw_traj, const int32_t *draw_k, int k_max, const double *uniforms, int U)
    {
        for (int r = 0; r < n; ++r) {
            if (draw_traj[r] < 0 || draw_traj[r] >= n_traj)
                return fail(BILD_ERR_INVALID, "draw_traj[%d] = %d: the set has %d trajectories", r, draw_traj[r], n_traj);
            if (draw_k && (draw_k[r] < 0 || draw_k[r] > k_max))
                return fail(BILD_ERR_INVALID, "draw_k[%d] = %d: outside 0 .. k_max = %d", r, draw_k[r], k_max);
        }
        if (uniforms)
            for (int64_t i = 0; i < (int64_t)n * U; ++i)
                if (!(uniforms[i] >= 0.0 && uniforms[i] < 1.0))
                    return fail(BILD_ERR_INVALID, "uniforms[%lld, %lld] = %g: outside [0, 1)", (long long)(i / U), (long long)(i % U),
                                uniforms[i]);
        std::vector<int> rank(n_traj, -1);
        for (int r = 0; r < n; ++r) rank[draw_traj[r]] = 0;
        for (int j = 0; j < n_traj; ++j)
            if (rank[j] == 0) {
                rank[j] = (int)used.size();
                used.push_back(j);
            }
        order.resize(n);
        slot_of.resize(n);
        first.assign(used.size() + 1, 0);
        for (int r = 0; r < n; ++r) ++first[rank[draw_traj[r]] + 1];
        for (size_t u = 0; u < used.size(); ++u) first[u + 1] += first[u];
        std::vector<int> fill(first.begin(), first.end() - 1);
        for (int r = 0; r < n; ++r) order[fill[rank[draw_traj[r]]]++] = r;
        for (int j : used) Tm = std::max(Tm, T[j]);
        return BILD_OK;
    }

    // The set's descriptors back from the device, those of `used` gathered; they and `order` go up on the frame's stream,
    // to memory of the frame.  The groups are declared BEFORE the frame.  A BILD_* code.
    int upload(CallFrame &call, int n_traj)
    {
        std::vector<GaussTraj> all(n_traj);
        GaussTraj *d = nullptr;
        int32_t *d_o = nullptr;
        BILD_TRY(call.alloc(&d, used.size()));
        BILD_TRY(call.alloc(&d_o, order.size()));
        BILD_TRY(call.alloc(&d_slot, order.size()));
        HIP_TRY(hipMemcpy(all.data(), call.d_trajs, (size_t)n_traj * sizeof(GaussTraj), hipMemcpyDeviceToHost));
        mine.resize(used.size());
        for (size_t u = 0; u < used.size(); ++u) mine[u] = all[used[u]];
        HIP_TRY(hipMemcpyAsync(d, mine.data(), mine.size() * sizeof(GaussTraj), hipMemcpyHostToDevice, call.st));
        HIP_TRY(hipMemcpyAsync(d_o, order.data(), order.size() * 4, hipMemcpyHostToDevice, call.st));
        d_used = d;
        d_order = d_o;
        return BILD_OK;
    }

    // the chunk of the nc trajectories used[u0 ..]: fills slot_of for its draws, which are places *i0 .. *i0 + *ni - 1 of
    // `order`, and sends that part of it to d_slot.  A BILD_* code.
    int chunk(CallFrame &call, int u0, int nc, int *i0, int *ni)
    {
        for (int u = u0; u < u0 + nc; ++u)
            for (int i = first[u]; i < first[u + 1]; ++i) slot_of[i] = u - u0;
        *i0 = first[u0];
        *ni = first[u0 + nc] - *i0;
        HIP_TRY(hipMemcpyAsync(d_slot + *i0, slot_of.data() + *i0, (size_t)*ni * 4, hipMemcpyHostToDevice, call.st));
        return BILD_OK;
    }
};

} // namespace bild
