// Table walk: the part of an AMIS batch that needs no Kalman frame (gfx950).
//
// With the tables of a trajectory set in place (common.h: prefix / transient / pair table) most candidates of a batch
// -- 96 % of the headline batch -- are a handful of table lookups: the running log-likelihood of the switch-free
// filter up to the first switch, then one transient (or pair) entry plus a difference of running sums per switch
// (reference: the loop bild/amis.py:735-739 over MSRouse_logL, bild/src/MSRouse_logL.pyx:95-256, of which this is an
// exact-to-rounding restatement).  That arithmetic needs no filter state, so it does not belong
// on a 16-lane row of the frame-loop kernel (84 registers per lane, LDS tables, spills): here ONE LANE takes one task
//
//   * reads its segment list -- or the sampler's own (s, theta) row, which it converts to switch frames exactly as
//     FixedkSampler.st2profile does (bild/amis.py:685-688: sequential cumsum, one multiplication by T - 1, floor, + 1;
//     no contraction) --,
//   * cleans it (kernels.hip: boundaries that switch nothing, empty segments and segments beyond the trajectory go),
//   * fetches, for all switches at once, the entries the walk may need (independent loads: one round trip),
//   * walks from synchronised point to synchronised point adding the same numbers in the same order as the frame-loop
//     kernel's `land`, and
//   * either writes the result, or -- at the first chain of switches the tables do not cover -- appends the task to
//     a work list for the frame-loop kernel, which runs only those (kernels.hip, KParams::work).
//
// Everything is kept in registers: the lists are indexed with compile-time constants only (loops over KMAX slots,
// fully unrolled), so nothing goes to scratch memory.  Results are bit-identical to the single-kernel launch
// (BILD_NO_SPLIT) for every task -- those finished here by construction of the walk, the others because the frame-loop
// kernel starts them from scratch.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <limits.h>
#include <stdlib.h>

#include "config.h"
#include "common.h"
#include "walk_task.h"

namespace bild {
namespace {

constexpr int kWalkThreads = 256;

template <int KMAX, bool ST>
__global__ void __launch_bounds__(kWalkThreads) walk_kernel(const WalkParams p)
{
    // Appending to the work lists: positions are handed out per workgroup in LDS, then ONE global atomic per bucket and
    // workgroup reserves the group's stretch of the list.  (Per-task atomics on sixteen words serialise in L2; so do
    // per-wave ones once a launch has thousands of waves: 25 us of a 200 000-candidate launch.)
    __shared__ int cnt[kWorkBuckets], base[kWorkBuckets];
    const int tid = threadIdx.x;
    const int64_t task = (int64_t)blockIdx.x * kWalkThreads + tid;
    if (tid < kWorkBuckets) cnt[tid] = 0;
    // the counters of the NEXT launch on this workspace (the other of two sets): nobody reads or writes them now
    if (p.work_counts_next != nullptr && task < kWorkBuckets) p.work_counts_next[task] = 0;
    __syncthreads();
    int bucket = -1;
    if (task < p.n * p.dstar_max) bucket = walk_task<KMAX, ST>(p, task, [](auto &&...) {});
    if (p.debug & 2) bucket = -1;
    int pos = 0;
    if (bucket >= 0) pos = atomicAdd(&cnt[bucket], 1);
    __syncthreads();
    if (tid < kWorkBuckets && cnt[tid] > 0) base[tid] = atomicAdd(p.work_counts + tid, cnt[tid]);
    __syncthreads();
    if (bucket >= 0) p.work[(int64_t)bucket * p.work_cap + base[bucket] + pos] = (int32_t)task;
}

template <bool ST>
int launch_st(const WalkParams &p, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    const int64_t ntasks = p.n * p.dstar_max;
    const unsigned grid = (unsigned)((ntasks + kWalkThreads - 1) / kWalkThreads);
    // one instantiation per list length (k = K1 - 1 switches per candidate)
#define BILD_WALK_CASE(KMAX)                                                                  \
    if (p.K1 == KMAX) {                                                                       \
        if (ev0 && ev1) hipExtLaunchKernelGGL((walk_kernel<KMAX, ST>), dim3(grid), dim3(kWalkThreads), 0, st, ev0, ev1, 0, p); \
        else hipLaunchKernelGGL((walk_kernel<KMAX, ST>), dim3(grid), dim3(kWalkThreads), 0, st, p);      \
        return (int)hipGetLastError();                                                        \
    }
    BILD_WALK_CASE(1)
    BILD_WALK_CASE(2)
    BILD_WALK_CASE(3)
    BILD_WALK_CASE(4)
    BILD_WALK_CASE(5)
    BILD_WALK_CASE(6)
    BILD_WALK_CASE(7)
    BILD_WALK_CASE(8)
    BILD_WALK_CASE(9)
    BILD_WALK_CASE(10)
    BILD_WALK_CASE(11)
    BILD_WALK_CASE(12)
    BILD_WALK_CASE(13)
    BILD_WALK_CASE(14)
    BILD_WALK_CASE(15)
    BILD_WALK_CASE(16)
#undef BILD_WALK_CASE
    return (int)hipErrorInvalidValue;
}

} // namespace

namespace {
__global__ void mark_refused_rows_kernel(const int32_t *__restrict__ seg_start, int K1, int64_t n, double *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n && seg_start[r * K1] < 0) out[r] = __longlong_as_double(0x7ff8000000000000ll);
}
} // namespace

// (s, theta) rows whose lists were all converted for a single launch of the frame loop: NaN for the rows the conversion refused
int launch_mark_refused_rows(const int32_t *seg_start, int K1, int64_t n, double *out, void *stream)
{
    if (n <= 0) return 0;
    const int bs = 256;
    hipLaunchKernelGGL(mark_refused_rows_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, reinterpret_cast<hipStream_t>(stream),
                       seg_start, K1, n, out);
    return (int)hipGetLastError();
}

int launch_walk(const WalkParams &p, void *stream, void *ev_start, void *ev_stop)
{
    if (p.n <= 0) return 0;
    if (bild::config().walk_debug) const_cast<WalkParams &>(p).debug = bild::config().walk_debug;
    if (p.n * p.dstar_max > (int64_t)INT_MAX) return (int)hipErrorInvalidValue; // task indices in the work lists are int32
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t ev0 = reinterpret_cast<hipEvent_t>(ev_start), ev1 = reinterpret_cast<hipEvent_t>(ev_stop);
    return p.ss ? launch_st<true>(p, st, ev0, ev1) : launch_st<false>(p, st, ev0, ev1);
}

} // namespace bild
