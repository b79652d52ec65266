// The frame of one exact-inference call: the lock that serialises the calls on a stream, the stream, the device memory of the
// call and the rule that cuts the call into chunks.  exact.cpp opens one itself; the calls on the segment recursion and on
// the dwell-time recursion declare one and have it opened by the recursion's owner (SegdpCall of gauss_segdp.h: gauss_segdp.cpp,
// gauss_segdraw.cpp, gauss_segsens.cpp; DwellCall of gauss_dwell.h: gauss_dwell.cpp, gauss_dwelldraw.cpp, gauss_dwellsens.cpp,
// gauss_dwelllen.cpp, gauss_dwellfilt.cpp); gauss_segtangent.cpp and DrawGroups (gauss_draws.h) allocate through it.  Host only; private to the
// library.
#pragma once
#include "internal.h"
#include "likelihood.h"

namespace bild {

// A call opens one frame, allocates through it and issues its work on `st`.  The members are declared in the order lock,
// stream, allocations, and the destructor undoes them from the other end: it first waits for the stream, so that no kernel
// or copy still uses the memory, then frees the allocations, and only then (the lock is the first member) lets the next call
// onto the stream.  That holds on every return path, an error path included.  Host vectors that asynchronous copies read
// or write are declared before the frame, so that they outlive the wait.
struct CallFrame {
    std::unique_lock<std::mutex> lock;
    hipStream_t st = nullptr;
    const GaussTraj *d_trajs = nullptr;     // the set's device descriptors (open(m, ts) only)
    std::vector<void *> ptrs;
    int64_t budget = 0;                     // bytes, from the last chunk_of()

    CallFrame() = default;
    CallFrame(const CallFrame &) = delete;
    CallFrame &operator=(const CallFrame &) = delete;
    ~CallFrame()
    {
        if (st) (void)hipStreamSynchronize(st);
        for (void *p : ptrs) (void)hipFree(p);
    }

    // on the stream of a GenericGaussianModel trajectory set, under the set's lock
    int open(const bild_gauss_model *m, const bild_gauss_trajset *ts)
    {
        void *stream = nullptr;
        std::mutex *mu = nullptr;
        BILD_TRY(internal_gauss_set_device(m, ts, &d_trajs, &stream, &mu));
        lock = std::unique_lock<std::mutex>(*mu);   // the set's stream: one call at a time
        st = (hipStream_t)stream;
        return BILD_OK;
    }

    // on a stream that the caller names, with the lock that guards it (none for a stream of the call's own)
    void open(hipStream_t stream, std::unique_lock<std::mutex> held)
    {
        lock = std::move(held);
        st = stream;
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

    // The chunk rule: as many of the n items (whole trajectories, or blocks) as fit the budget, at least one.  The budget is
    // scratch_bytes, or, where that is 0, at most 1 GiB and a third of the free memory.  A BILD_* code; the chunk in *chunk.
    int chunk_of(int64_t per_item_bytes, int64_t scratch_bytes, int n, int *chunk)
    {
        budget = scratch_bytes;
        if (budget == 0) {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            budget = std::min<int64_t>((int64_t)1 << 30, (int64_t)(free_b / 3));
        }
        *chunk = (int)std::max<int64_t>(1, std::min<int64_t>(budget / per_item_bytes, n));
        return BILD_OK;
    }
};

} // namespace bild
