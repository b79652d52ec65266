// Host pieces the trajectory generators share (sim.cpp: Rouse, gauss_sim.cpp: GenericGaussianModel): the device memory
// of one call and the rule that cuts a call's normals into upload chunks.  Private to the library.
#pragma once
#include "likelihood.h"

namespace bild {

// device memory of one call, freed on every path
struct SimBufs {
    std::vector<void *> ptrs;
    hipStream_t stream = nullptr;
    ~SimBufs()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        for (void *p : ptrs) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
    template <class X> int put(X **out, const void *host, size_t count)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(X));
        if (e != hipSuccess) return fail(BILD_ERR_NOMEM, "hipMalloc(%zu) failed: %s", count * sizeof(X), hipGetErrorString(e));
        ptrs.push_back(p);
        *out = static_cast<X *>(p);
        if (host && count) HIP_TRY(hipMemcpyAsync(p, host, count * sizeof(X), hipMemcpyHostToDevice, stream));
        return BILD_OK;
    }
};

// the upload budget of the normals: the caller's scratch_bytes, or at most 1 GiB and a third of the free memory
inline int64_t sim_scratch_bytes(int64_t scratch_bytes, size_t free_bytes)
{
    return scratch_bytes > 0 ? scratch_bytes : std::min<int64_t>(1ll << 30, (int64_t)(free_bytes / 3));
}

// the chunk that starts at trajectory `first`: whole trajectories while their normals (z_off: per trajectory, offsets
// into all of the call's) fit `budget` doubles, at least one -> one past its last trajectory
inline int sim_chunk_end(const std::vector<int64_t> &z_off, int first, int n, int64_t budget)
{
    int last = first + 1;
    while (last < n && z_off[last + 1] - z_off[first] <= budget) ++last;
    return last;
}

} // namespace bild
