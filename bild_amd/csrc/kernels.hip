// Rouse Kalman-filter log-likelihood kernels for gfx950 (MI355X, CDNA4).
//
// What is computed (reference bild/src/MSRouse_logL.pyx:186-256, MSRouse_logL_py.py:96-121):
// for every task = (sample, covariance chain e) a T-step Kalman filter over the N-monomer
// chain, observed through y = w.x with localization noise s2[e]; the task's result is the
// sum of the per-frame Gaussian log-densities of the dimensions that use chain e.
//
// Mapping to the machine
// ----------------------
// * One task runs on a *group* of G lanes of a wavefront (G = 13 for the default 2-state model,
//   which reduces to 10 modes: one lane per column of [C | M]), floor(64/G) groups per wave,
//   4 waves per workgroup.  Recursions are independent, so there is no inter-workgroup
//   traffic and no grid-level synchronisation.
// * The filter state is the augmented matrix  A = [ C | M ]  (NP x (NP + d)): covariance
//   and the d mean vectors.  A is distributed BY COLUMN: lane gl of the group owns columns
//   gl*CPL .. gl*CPL+CPL-1 in registers (CPL*NP doubles).  With C symmetric,
//       Cw_j = sum_i w_i C_ij                       is a lane-local dot product,
//       yhat_dim = sum_i w_i M_i,dim                is the same dot product on an M column,
//       C_:j -= Cw (Cw_j / S),  M_:dim += Cw (nu/S) are the same lane-local rank-1 update,
//   so covariance and mean columns are processed by identical code and the only
//   cross-lane step per frame is an all-gather of the NP numbers Cw through LDS.
// * kModal: the recursion is carried in the eigenbasis Q_s of the current state's
//   (symmetric) propagator B_s, where the predict  C <- B C B + Sig  is elementwise,
//   C'_ij <- lam_i lam_j C'_ij + sig_i delta_ij.  A state switch s -> s2 applies the
//   orthogonal basis change R = Q_s2^T Q_s:  A <- R A (all columns), C <- C R^T.
// * kDense: the canonical recursion, C <- B C B + Sig every frame (pyx:220-241), done as
//   two lane-local mat-vecs per column with an in-group transpose through LDS between
//   them.  Same code path as the modal basis change.
// * Propagator / basis-change matrices are staged once per workgroup into LDS and read
//   as group-wide broadcasts (ds_read_b128); one LDS operand pair feeds 2*CPL FMAs per row.
// * fp64 throughout (v_fma_f64).  The modal predict is elementwise, so there is no GEMM to move to the matrix
//   pipe here (the one use tried in this kernel -- the cross-lane sum S = s2 + w.(Cw) as two
//   v_mfma_f64_4x4x4_4b, "block layout" below -- gains 2-5 % and is an opt-in geometry: the f64 matrix
//   and vector instructions draw on the same FMA throughput).  The DENSE recursion, which IS two small GEMMs
//   per frame, runs on the matrix pipe in dense_mfma.hip whenever the chain tiles into 4x4 blocks; the kDense
//   code below serves the other chain lengths.
// * sum_t log S_t is accumulated as a running product with exponent extraction
//   (frexp) and one log per task, instead of one log per frame.
//
// This file holds the __global__ kernels, the launchers and the choice of a geometry.  The task loop every logl kernel inlines is
// logl_body.h, the device helpers of a frame frame_ops.h, the LDS layout common.h: LdsLayout.  The geometry table (BILD_GEOMETRIES)
// stays here: the geometry sweep of the tests parses it out of this file.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <hip/hip_ext.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>

#include "config.h"
#include "common.h"
#include "walk_task.h"

#include "frame_ops.h"
#include "logl_body.h"

namespace bild {
namespace {

template <int NP, int CPL, int G, int W, int OCC, int LAY, int MODE, int FLAVOR, bool DUMP = false, bool JUMP = false, bool BUILD = false>
__global__ void __launch_bounds__(64 * W, OCC) logl_kernel(const KParams p)
{
    // The listed frame loop (geometry 23) takes the two-row frame whenever no wave has to carry more than two tasks: the list fits
    // the grid's row pairs once.  A task alone on its wave -- the chains that end the launch -- then issues ~45 instead of ~61 vector
    // instructions per frame (10k x k = 4: step 51.9-52.2 -> 48.3 us); longer lists (throughput-bound: four tasks per wave share one
    // instruction stream) keep the one-row frame.  The length is known only here, behind the walk; both frames give the same bits.
    if constexpr (LAY == 3 && MODE == kModal && JUMP && !DUMP && !BUILD) {
        if (p.work != nullptr) {
            int64_t tot = 0;
            for (int bq = 0; bq < kWorkBuckets; ++bq) tot += p.work_counts[bq];
            if (tot <= (int64_t)gridDim.x * W * (64 / G / 2)) {
                logl_body<NP, CPL, G, W, OCC, LAY, MODE, FLAVOR, DUMP, JUMP, BUILD, true>(p);
                return;
            }
        }
    }
    logl_body<NP, CPL, G, W, OCC, LAY, MODE, FLAVOR, DUMP, JUMP, BUILD>(p);
}

// ---- the one-launch path: table walk and listed frame loop in one grid --------------------------------------------------------
// Where the hand-off stays inside a workgroup (LDS and barriers: no work lists, no atomics, no waiting on other workgroups), the
// frame loop needs no second launch: each workgroup walks a contiguous slice of the batch and runs the tasks its walk could not
// finish itself.  A listed task of the first layer finds its cleaned list, its walk plan and its expected frames in the LDS areas
// of its rows -- written by the walk lane, with the values the frame loop's prologue would compute (the same expressions on the
// same list, see walk_task.h) -- and starts at the state vectors.  DESIGN.md section 4.
typedef __attribute__((address_space(3))) double lds_base_t; // (the LDS base: LdsLayout counts in doubles)

// The walk of the workgroup's slice [t0, t1) (<= kOneSlice tasks; slice position j on wave j % W, lane j / W) and the deal of its
// listed tasks: heaviest first (expected frames, then task index), position q on wave (q + rot) % W, row (pair) q / W.  Inline: the
// parameters stay kernel arguments (scalar loads; out of line they were a private copy in scratch, read by dependent flat loads), and
// the staging loads the kernel issued in front of it are waited for together with the walk's first loads, not before them.
template <int KMAX, bool ST, int W>
__device__ __forceinline__ void walk_one(const WalkParams &p, int64_t t0, int64_t t1, const LdsLayout L, lds_base_t *base)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, gpw = L.groups / W; // (rows per wave)
    __attribute__((address_space(3))) OneHand *const h = (__attribute__((address_space(3))) OneHand *)(base + L.hand0);
    const int64_t task = t0 + (int64_t)lane * W + wv;
    int la[KMAX], lb[KMAX], lm1[KMAX], lm2[KMAX];
    double lv1[KMAX], lv2[KMAX];
    unsigned lkeep = 0;
    double lx0 = 0.0;
    int lw = 0;
    int bucket = -1;
    if (task < t1)
        bucket = walk_task<KMAX, ST>(p, task, [&](const int (&a)[KMAX], const int (&b)[KMAX], unsigned keep, const double (&v1)[KMAX],
                                                   const double (&v2)[KMAX], const int (&m1)[KMAX], const int (&m2)[KMAX], double x0, int w) {
#pragma unroll
            for (int i = 0; i < KMAX; ++i) {
                la[i] = a[i];
                lb[i] = b[i];
                lv1[i] = v1[i];
                lv2[i] = v2[i];
                lm1[i] = m1[i];
                lm2[i] = m2[i];
            }
            lkeep = keep;
            lx0 = x0;
            lw = w;
        });
    if (p.debug & 2) bucket = -1;
    const bool listed = bucket >= 0;
    const unsigned long long mask = __ballot(listed);
    if (lane == 0) h->cnt[wv] = (int32_t)__popcll(mask);
    __syncthreads();
    int n = 0, j = (int)__popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int c = h->cnt[k];
        n += c;
        j += k < wv ? c : 0;
    }
    if (listed) {
        h->reg_task[j] = (int32_t)task;
        h->reg_w[j] = lw;
    }
    if (tid == 0) h->n = n;
    __syncthreads();
    if (listed) {
        int q = 0;
        for (int k = 0; k < n; ++k) {
            const int wk = h->reg_w[k], tk = h->reg_task[k];
            q += (wk > lw || (wk == lw && tk < (int)task)) ? 1 : 0;
        }
        h->task[q] = (int32_t)task;
        const bool pair = n <= W * gpw / 2; // (logl_one_kernel: the two-row frame while the tasks fit the row pairs once)
        const int per_wave = pair ? gpw / 2 : gpw;
        if (q < W * per_wave) {
            const int rot = (int)(blockIdx.x / 256) % W;
            const int row0 = ((q + rot) % W) * gpw + (pair ? 2 * (q / W) : q / W);
            for (int rr = 0; rr < (pair ? 2 : 1); ++rr) {
                __attribute__((address_space(3))) int32_t *const sl =
                    (__attribute__((address_space(3))) int32_t *)(base + L.seg0) + (size_t)(row0 + rr) * (2 * group_seg_doubles());
                lds_base_t *const wk = base + L.walk0 + (size_t)(row0 + rr) * kWalkDoubles;
                sl[0] = la[0];
                sl[kSegLds] = lb[0];
                wk[0] = lx0;
                int cnt = 1;
#pragma unroll
                for (int i = 1; i < KMAX; ++i) {
                    if ((lkeep >> i) & 1u) {
                        sl[cnt] = la[i];
                        sl[kSegLds + cnt] = lb[i];
                        wk[3 * cnt] = lv1[i];
                        wk[3 * cnt + 1] = lv2[i];
                        wk[3 * cnt + 2] = __hiloint2double(lm2[i], lm1[i]);
                        ++cnt;
                    }
                }
                wk[1] = __hiloint2double(lw, cnt); // (slots 1 and 2 belong to no switch)
            }
        }
    }
    __syncthreads();
}

template <int NP, int CPL, int G, int W, int OCC, int LAY, int FLAVOR>
__global__ void __launch_bounds__(64 * W, OCC) logl_one_kernel(const KParams p, const WalkParams wp)
{
    static_assert(LAY == 3 && CPL == 1 && G == 16 && W <= 4, "the one-launch path serves the listed frame loop (geometry 23)");
    extern __shared__ __align__(16) double smem[];
    constexpr int kThreads = 64 * W, GPW = 64 / G, HDR = state_header_doubles(NP);
    const int64_t ntasks = wp.n * wp.dstar_max;
    const int64_t slice = (ntasks + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * slice;
    if (t0 >= ntasks) return;
    const int64_t t1 = t0 + slice < ntasks ? t0 + slice : ntasks;
    // the tables of the frame loop, as logl_body stages them: the first kPre doubles per thread are asked for HERE, in front of the
    // walk, and written to LDS behind it -- their round trip overlaps the walk's first one (the headline model: 460 doubles, all of them)
    const int tid = threadIdx.x;
    const LdsLayout L(NP, W * GPW, p.tab_doubles, p.S);
    const int lds_tab = L.img0; // (the tables and the state headers)
    auto stage_src = [&](int i) {
        return i < p.tab_doubles ? p.tab + i : p.states + (size_t)((i - p.tab_doubles) / HDR) * StateBlock::size(NP) + (i - p.tab_doubles) % HDR;
    };
    constexpr int kPre = 4;
    double pre[kPre];
#pragma unroll
    for (int u = 0; u < kPre; ++u) {
        const int i = tid + u * kThreads;
        pre[u] = i < lds_tab ? *stage_src(i) : 0.0;
    }
    lds_base_t *const base = (lds_base_t *)smem;
    static_assert(kOneLaunchMaxK1 == 5, "one walk instantiation per list length the host sends here");
    switch (wp.K1) {
#define BILD_ONE_CASE(KMAX)                                                                  \
    case KMAX:                                                                               \
        if (wp.ss) walk_one<KMAX, true, W>(wp, t0, t1, L, base);                           \
        else walk_one<KMAX, false, W>(wp, t0, t1, L, base);                                \
        break;
        BILD_ONE_CASE(1) BILD_ONE_CASE(2) BILD_ONE_CASE(3) BILD_ONE_CASE(4) BILD_ONE_CASE(5)
#undef BILD_ONE_CASE
    default: return;
    }
#pragma unroll
    for (int u = 0; u < kPre; ++u)
        if (tid + u * kThreads < lds_tab) smem[tid + u * kThreads] = pre[u];
    for (int i = tid + kPre * kThreads; i < lds_tab; i += kThreads) smem[i] = *stage_src(i);
    __syncthreads();
    const OneHand *const hand = reinterpret_cast<const OneHand *>(smem + L.hand0);
    const int n = hand->n;
    if (n == 0) return; // (every task of the slice finished by the walk)
    // the two-row frame while the workgroup's tasks fit its row pairs once (logl_kernel makes the same choice for the whole grid)
    if (n <= W * GPW / 2) logl_body<NP, CPL, G, W, OCC, LAY, kModal, FLAVOR, false, true, false, true, true>(p, hand);
    else logl_body<NP, CPL, G, W, OCC, LAY, kModal, FLAVOR, false, true, false, false, true>(p, hand);
}

// The running log-likelihood of every record of the prefix table (common.h), from the sums its builder left in the record: one thread
// per (task, frame); the sums of the dimensions are added in the order piece_value adds them (lane order: dimension 0, 1, 2).
__global__ void prefix_L_kernel(const TrajDesc *__restrict__ trajs, int n_traj, int S, int NP, int dstar_max, int blocks_per_task,
                                double *__restrict__ prefix, double *__restrict__ prefix_L)
{
    const int task = blockIdx.x / blocks_per_task; // (j * dstar_max + e) * S + s
    const int s = task % S, e = (task / S) % dstar_max, j = task / (S * dstar_max);
    if (j >= n_traj) return;
    const TrajDesc &td = trajs[j];
    const int t = (blockIdx.x % blocks_per_task) * blockDim.x + threadIdx.x;
    if (e >= td.dstar || t >= td.T) return;
    const int NC = NP + kDMax, REC = prefix_record_doubles(NP);
    const int kRecP = NC * NP + kDMax, kRecE = kRecP + 1, kRecL = kRecP + 2, kRecNv = kRecP + 3;
    const int64_t r = td.prefix_rec0 + ((int64_t)e * S + s) * td.T + t;
    double *rec = prefix + r * REC;
    const int nd = td.ndims[e];
    double tot = 0.0;
    for (int m = 0; m < nd; ++m) tot += rec[NC * NP + m];
    const double L = piece_from_sums(tot, rec[kRecP], (int)rec[kRecE], (int)rec[kRecNv], nd);
    rec[kRecL] = L;
    if (prefix_L) prefix_L[r] = L;
}

__global__ void reduce_partials_kernel(const double *__restrict__ partial, double *__restrict__ out, int64_t n,
                                       int dstar_max)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double tot = 0.0;
    for (int e = 0; e < dstar_max; ++e) tot += partial[r * dstar_max + e];
    out[r] = tot;
}

// Optional check of device-resident descriptors (BILD_VALIDATE_DEVICE): the indices below drive LDS and HBM
// addressing in the likelihood kernels.  err[0] = first kind of violation seen (1 traj_id, 2 first start, 3 order of
// starts, 4 state), err[1] = a sample that shows it.
__global__ void validate_kernel(const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_state,
                                const int32_t *__restrict__ traj_id, const int32_t *__restrict__ order, int64_t n, int K1,
                                int S, int n_traj, int *err)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int bad = 0;
    // order must be a permutation: in range, and every sample hit exactly once (err[2 + sample] counts the hits)
    if (order) {
        if (order[r] < 0 || order[r] >= n) bad = 5;
        else if (atomicAdd(err + 2 + order[r], 1) != 0) bad = 5;
    }
    if (traj_id && (traj_id[r] < 0 || traj_id[r] >= n_traj)) bad = 1;
    const int32_t *a = seg_start + r * K1, *b = seg_state + r * K1;
    if (!bad && a[0] != 0) bad = 2;
    for (int i = 0; i < K1 && !bad; ++i) {
        if (i > 0 && (a[i] < a[i - 1] || a[i] < 1)) bad = 3;
        else if (b[i] < 0 || b[i] >= S) bad = 4;
    }
    if (bad && atomicCAS(err, 0, bad) == 0) err[1] = (int)(r < INT_MAX ? r : INT_MAX);
}

// MODES: the geometry's last field (BILD_GEOMETRIES).  Only the kernels of the paths a launch can reach the geometry on are
// instantiated -- the rule of geometry_for, a field of 0 counting as modal; any other combination is refused.
template <int NP, int CPL, int G, int W, int OCC, int LAY, int MODES>
int launch_geom(int mode, const KParams &p, int grid, size_t lds, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1)
{
    constexpr int kThreads = 64 * W;
    hipError_t err;
    auto go = [&](auto k) -> int {
        err = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return (int)err;
        // timed launches: the events are attached to the dispatch itself (start and end of the kernel as the profiler sees
        // them), not recorded around it -- events AROUND a launch add the latency of two barrier packets, 12-14 us, to a
        // kernel of this size
        if (ev0 && ev1) hipExtLaunchKernelGGL(k, dim3(grid), dim3(kThreads), (unsigned)lds, st, ev0, ev1, 0, p);
        else hipLaunchKernelGGL(k, dim3(grid), dim3(kThreads), lds, st, p);
        return (int)hipGetLastError();
    };
    // G != 0 (an external force on the chain) never occurs through the reference's entry points
    // (rouse.Model is built with F = 0, models.py:246): keep it out of the common kernels
    // (and trajectories without a single missing frame out of the masked ones)
    const int flavor = p.has_G ? 0 : (p.all_valid ? 2 : 1);
    constexpr int kPaths = MODES ? MODES : 2;
    const bool builds = p.prefix_dump || p.trans_dump || p.trans2_dump; // (the tables are built on the modal path)
    if (!(kPaths & (mode == kDense ? 1 : 2)) || (builds && (mode != kModal || LAY >= 3))) return (int)hipErrorInvalidValue; // (see kLean)
    if constexpr ((kPaths & 2) != 0) {
        if (p.prefix_dump) {
            // the table is built by the packed one-column geometry with room for kDMax mean vectors
            if constexpr (LAY == 0 && CPL == 1 && G == NP + kDMax) {
                if (flavor == 0) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 0, true>);
                if (flavor == 1) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 1, true>);
                return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 2, true>);
            } else {
                return (int)hipErrorInvalidValue;
            }
        }
        if (p.trans_dump || p.trans2_dump) {
            // the transient / pair / state tables: the BUILD instantiation of the geometry (never the lean ones, see above, nor the
            // block layout, which does not jump)
            if constexpr (LAY == 0 || LAY == 2) {
                if (!p.prefix || p.no_jump) return (int)hipErrorInvalidValue;
                if (flavor == 0) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 0, false, true, true>);
                if (flavor == 1) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 1, false, true, true>);
                return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 2, false, true, true>);
            } else {
                return (int)hipErrorInvalidValue;
            }
        }
        if (mode == kModal && p.prefix && !p.no_jump) {
            if constexpr (LAY == 1) {
                return (int)hipErrorInvalidValue; // (the block layout runs frame by frame only: see BILD_GEOMETRIES)
            } else {
                if (flavor == 0) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 0, false, true>);
                if (flavor == 1) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 1, false, true>);
                return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 2, false, true>);
            }
        }
        if (mode == kModal) {
            if (flavor == 0) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 0>);
            if (flavor == 1) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 1>);
            return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kModal, 2>);
        }
    }
    if constexpr ((kPaths & 1) != 0) {
        if (flavor == 0) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kDense, 0>);
        if (flavor == 1) return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kDense, 1>);
        return go(logl_kernel<NP, CPL, G, W, OCC, LAY, kDense, 2>);
    }
    return (int)hipErrorInvalidValue;
}

// (id, rows, columns per lane, lanes per group, waves per workgroup, min waves per SIMD, paths);
// CPL * G >= NP + 1: a group carries min(3, CPL * G - NP) mean vectors (G = NP + 1 / + 2 serve chains of one /
// two dimensions -- d < 3, or localization errors that differ between dimensions -- with more tasks per wave).  W is chosen so that W * (64/G) group images + the dense tables fit in
// 160 KiB of LDS; OCC bounds the register allocation (512 / OCC VGPRs per lane).  The table
// may hold several geometries per NP, listed by increasing tasks per wave: geometry_for takes
// the first one whose waves are all resident at once, else the last (densest) one.
// Measured on MI355X (profiles/r01_geometry_sweep.txt):
//  * NP = 10: (CPL, G) = (3, 5) and (5, 3) -- fewer lanes per task, fewer instructions per
//    task -- lose to 2 columns per lane at every batch size: they run at one wave per SIMD
//    with a longer dependent chain per frame.  (2, 7) beats (2, 8): 9 instead of 8 tasks per
//    wave at the same instruction count (13 of 14 column slots used).
//    One column per lane (1, 13) at three waves per SIMD has the shortest frame latency
//    (0.28 us vs 0.46 us per frame for a lone wave) and wins up to ~12k tasks; (2, 7) beyond.
//  * NP = 16 / 20: one column per lane at two waves per SIMD beats 2 and 3 columns per lane (one
//    wave per SIMD) at every batch size from 3 000 to 160 000 tasks; forcing two waves per SIMD
//    onto the multi-column geometries spills inside the frame loop (4-6x slower).
//  * NP >= 24: the multi-column geometries spill in the frame loop even at one wave per SIMD
//    (10-20x slower); one column per lane (1-2 tasks per wave) does not.
//  * NP = 10 / 12, one column per lane, G = 16 (ids 15 / 16, only through BILD_GEOM): the block layout -- a
//    task is one 16-lane block of the f64 4x4x4 matrix instruction and S comes from block_sum16.  2-5 %
//    faster than the packed (1, 13) / (1, 15) at every batch size, 7 % with missing frames: the f64 matrix
//    and vector pipes share their FMA throughput, so only the redundancy of the per-lane S chain is saved.
//    Not selected automatically: its S is summed in another order, and with it the results of one profile
//    would differ in the last bits between batch sizes (all other geometries of an NP agree bit for bit).  Frame by frame
//    only: its jumping instantiation is neither compiled nor dispatched (launch_geom, geometry_for).  Forced onto split launches
//    it returned NaN for some rows; the cause is not known -- not the block sum (the f64 MFMA sums each 16-lane block
//    correctly under a partial EXEC mask, measured on MI355X), and the other layouts pass the same launches bit for bit.
//  * NP = 10 / 12, one column per lane, G = 16, row layout (ids 21 / 22): a task is one 16-lane row and every use of
//    (C w)_i reads lane i of the row by DPP row broadcast inside the FMA itself (v_fmac_f64_dpp ... row_newbcast) --
//    no LDS all-gather in the frame loop, 20 registers less.  Same operations in the same order as the packed
//    layouts, hence bit-identical results (checked: max |diff| = 0 against (1, 13) on every batch size tried).
//    10 000 x T=1000: 485 -> 448 us; a lone wave (3 000 tasks) 285 -> 237 us; with missing frames 522 -> 484 us
//    Id 23 is the same layout bounded for TWO waves per SIMD: the frame loop over the work lists of a split launch
//    (walk.hip), which is latency-bound -- a few hundred tasks, one per wave, the launch as long as its longest chain --
//    and gains 6-9 % from the larger register budget (no spills around the frame loop, the measurement vector in
//    registers instead of five LDS reads per frame: 63.6 -> 59.6 us at k = 4, 116 -> 105 us at k = 8); for whole batches
//    run frame by frame three waves per SIMD stay the better geometry (r02_occ2_again.txt).
//    (profiles/r02_row_layout.txt).  Listed before the packed geometry with the same number of tasks per wave, so the
//    modal path picks it whenever three mean vectors are needed; with fewer, (1, 11) / (1, 12) carry 5 tasks per wave.
// seventh field: layout (0 packed, 1 matrix-instruction block, 2 row; 3 / 4: row / packed for the frame loop over the work lists only); last field: which paths may select the geometry
// automatically (1 = dense, 2 = modal, 3 = both).
// The dense recursion is FMA-bound with one LDS operand feeding 2*CPL FMAs, so it wants several
// columns per lane where the modal one wants a single column.
#ifndef BILD_ROW_OCC
#define BILD_ROW_OCC 3
#endif
#define BILD_GEOMETRIES(X)     \
    X(0, 4, 1, 7, 4, 3, 0, 3)     \
    X(1, 4, 2, 4, 4, 2, 0, 3)     \
    X(17, 8, 1, 9, 4, 3, 0, 3)    \
    X(18, 8, 1, 10, 4, 3, 0, 3)   \
    X(2, 8, 1, 11, 4, 3, 0, 3)    \
    X(19, 10, 1, 11, 4, 3, 0, 3)  \
    X(20, 10, 1, 12, 4, 3, 0, 3)  \
    X(21, 10, 1, 16, 4, BILD_ROW_OCC, 2, 2)  \
    X(23, 10, 1, 16, 4, 2, 3, 0)  \
    X(3, 10, 1, 13, 4, 3, 0, 3)   \
    X(4, 10, 2, 7, 4, 2, 0, 3)    \
    X(22, 12, 1, 16, 4, 2, 2, 2)  \
    X(5, 12, 1, 15, 4, 2, 0, 3)   \
    X(6, 12, 2, 8, 4, 2, 0, 3)    \
    X(7, 16, 1, 19, 4, 2, 0, 2)   \
    X(24, 16, 1, 19, 4, 1, 4, 0)  \
    X(8, 16, 3, 7, 4, 1, 0, 1)    \
    X(9, 20, 1, 23, 4, 2, 0, 2)   \
    X(25, 20, 1, 23, 4, 1, 4, 0)  \
    X(10, 20, 2, 12, 4, 1, 0, 1)  \
    X(11, 20, 3, 8, 4, 1, 0, 1)   \
    X(12, 24, 1, 27, 4, 1, 0, 3)  \
    X(13, 28, 1, 31, 4, 1, 0, 3)  \
    X(14, 32, 1, 35, 4, 1, 0, 3)  \
    X(15, 10, 1, 16, 4, 3, 1, 0)  \
    X(16, 12, 1, 16, 4, 2, 1, 0)

constexpr Geometry kGeoms[] = {
#define X(ID, NP, CPL, G, W, OCC, LAY, MODES) {NP, CPL, G, W, OCC, ID, MODES, LAY},
    BILD_GEOMETRIES(X)
#undef X
};

} // namespace

int padded_rows(int n_rows)
{
    for (const Geometry &c : kGeoms)
        if (c.NP >= n_rows) return c.NP;
    return 0;
}

// BILD_GEOM=<id> (diagnostics and tests) forces geometry `id` onto every evaluating launch of the vector kernels that it fits:
// the same padded row count, room for `means` mean vectors, and a path its last field admits -- where that field is 0 (the
// geometries never picked automatically: the block layouts 15 / 16, the lean frame loops 23 / 24 / 25, all of them modal
// layouts) it counts as modal.  A launch it does not fit takes the automatic choice below (BILD_Q_LAST_GEOMETRY tells which
// geometry ran): the kernels of the other paths are not compiled, and launch_geom refuses them by the same rule.
// Launches that BUILD a table never take the forced geometry (`forced` = false: the transient and pair tables, whose builder
// launches go through launch_batch; the prefix table takes builder_geometry): the lean geometries cannot build one, and the
// tables of a set, with all the results read out of them, do not depend on the switch.
// A launch that may jump (`jumps`) never takes the block layout (LAY 1): see BILD_GEOMETRIES.
bool geometry_for(int NP, int mode, int64_t ntasks, int means, Geometry *g, bool forced, bool jumps)
{
    if (forced && bild::config().geom >= 0) {
        const int id = bild::config().geom;
        const int path = mode == kDense ? 1 : 2;
        for (const Geometry &c : kGeoms)
            if (c.id == id && c.NP == NP && c.mean_slots() >= means && ((c.modes ? c.modes : 2) & path) && !(jumps && c.lay == 1)) {
                *g = c;
                return true;
            }
    }
    // candidates are listed by increasing lanes per task, then increasing tasks per wave.  Of those with room
    // for `means` mean vectors, one column per lane and the fewest lanes come first; take the first one whose
    // waves are all resident at once (256 CUs x 4 SIMDs x OCC waves); if none is, the one with the smallest
    // (rounds of resident waves) x (cost of a frame ~ CPL + c0), c0 = per-frame overhead in units of
    // one column's work (dense: FMA-bound, ~0; modal: ~2)
    const Geometry *best = nullptr;
    int64_t best_cost = 0;
    for (const Geometry &c : kGeoms) {
        if (c.NP != NP || c.mean_slots() < means || !(c.modes & (mode == kDense ? 1 : 2))) continue;
        // of the one-column geometries only the tightest fit is a candidate (the wider ones idle lanes)
        if (best && best->CPL == 1 && c.CPL == 1) continue;
        const int64_t waves = (ntasks + c.tasks_per_wave() - 1) / c.tasks_per_wave();
        const int64_t slots = 1024 * (int64_t)c.OCC;
        if (waves <= slots) {
            best = &c;
            break;
        }
        const int64_t cost = ((waves + slots - 1) / slots) * (c.CPL + (mode == kDense ? 0 : 2));
        if (!best || cost < best_cost) {
            best = &c;
            best_cost = cost;
        }
    }
    if (!best) return false;
    *g = *best;
    return true;
}

// The frame loop over the work lists is latency-bound (a few hundred tasks, the launch as long as its longest chain): it
// takes the geometry of the chain length with the LARGEST register budget -- for 10 modes the row layout at two waves per SIMD
// (id 23), for 16 / 20 modes the packed layout at one wave per SIMD (ids 24 / 25: what spills to scratch memory at two waves
// per SIMD -- two reloads per frame, dozens per comparison -- stays in registers there).
bool listed_geometry(const Geometry &from, Geometry *g)
{
    if (bild::config().geom >= 0 || bild::config().no_listed_geometry) return false;
    const int to = from.id == 21 ? 23 : from.id == 7 ? 24 : from.id == 9 ? 25 : -1;
    for (const Geometry &c : kGeoms)
        if (c.id == to) {
            *g = c;
            return true;
        }
    return false;
}

bool builder_geometry(int NP, Geometry *g)
{
    for (const Geometry &c : kGeoms)
        if (c.NP == NP && c.CPL == 1 && c.G == NP + kDMax && c.id != 15 && c.id != 16 && c.id != 21 && c.id != 22 && c.id != 23) {
            *g = c;
            return true;
        }
    return false;
}

const char *kernel_name(const Geometry &, int mode) { return mode == kModal ? "logl_kernel<modal>" : "logl_kernel<dense>"; }

int launch_logl(const Geometry &g, int mode, const KParams &p, int grid, size_t lds, void *stream, void *ev_start, void *ev_stop)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t ev0 = reinterpret_cast<hipEvent_t>(ev_start), ev1 = reinterpret_cast<hipEvent_t>(ev_stop);
    switch (g.id) {
#define X(ID, NP, CPL, G, W, OCC, LAY, MODES) \
    case ID: return launch_geom<NP, CPL, G, W, OCC, LAY, MODES>(mode, p, grid, lds, st, ev0, ev1);
        BILD_GEOMETRIES(X)
#undef X
    default: return -1;
    }
}

int launch_validate(const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id, const int32_t *order, int64_t n,
                    int K1, int S, int n_traj, int *d_err, void *stream)
{
    const int bs = 256;
    hipLaunchKernelGGL(validate_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, reinterpret_cast<hipStream_t>(stream),
                       seg_start, seg_state, traj_id, order, n, K1, S, n_traj, d_err);
    return (int)hipGetLastError();
}

int launch_prefix_L(const TrajDesc *d_trajs, int n_traj, int S, int NP, int dstar_max, int Tmax, double *d_prefix, double *d_prefix_L, void *stream)
{
    const int64_t tasks = (int64_t)n_traj * dstar_max * S;
    if (tasks <= 0 || Tmax <= 0) return 0;
    const int bpt = (Tmax + 255) / 256;
    if (tasks * bpt >= ((int64_t)1 << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(prefix_L_kernel, dim3((unsigned)(tasks * bpt)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d_trajs, n_traj, S, NP,
                       dstar_max, bpt, d_prefix, d_prefix_L);
    return (int)hipGetLastError();
}

int launch_logl_one(const Geometry &g, const KParams &p, const WalkParams &w, int grid, size_t lds, void *stream, void *ev_start, void *ev_stop)
{
    if (g.id != 23 || w.K1 < 1 || w.K1 > kOneLaunchMaxK1 || !p.walk_lds || !p.prefix || p.no_jump || !p.trans || p.work) return (int)hipErrorInvalidValue;
    const int64_t ntasks = w.n * w.dstar_max;
    if (grid < 1 || (ntasks + grid - 1) / grid > kOneSlice) return (int)hipErrorInvalidValue;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipEvent_t ev0 = reinterpret_cast<hipEvent_t>(ev_start), ev1 = reinterpret_cast<hipEvent_t>(ev_stop);
    auto go = [&](auto k) -> int {
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) return (int)err;
        if (ev0 && ev1) hipExtLaunchKernelGGL(k, dim3(grid), dim3(256), (unsigned)lds, st, ev0, ev1, 0, p, w);
        else hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, st, p, w);
        return (int)hipGetLastError();
    };
    const int flavor = p.has_G ? 0 : (p.all_valid ? 2 : 1);
    if (flavor == 0) return go(logl_one_kernel<10, 1, 16, 4, 2, 3, 0>);
    if (flavor == 1) return go(logl_one_kernel<10, 1, 16, 4, 2, 3, 1>);
    return go(logl_one_kernel<10, 1, 16, 4, 2, 3, 2>);
}

int launch_reduce_partials(const double *partial, double *out, int64_t n, int dstar_max, void *stream)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int bs = 256;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, st, partial, out, n,
                       dstar_max);
    return (int)hipGetLastError();
}

} // namespace bild
