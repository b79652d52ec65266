// logl_body: the task loop of the vector likelihood kernels (kernels.hip: logl_kernel, logl_one_kernel) -- one device function,
// inlined into every kernel, that deals a task to a group of lanes, runs its prologue, starts it, runs its frame loop and writes its
// result.  Its parts, in the order they stand in the function (all lambdas that capture the task's values by reference):
//
//  * dealing a task: loop position -> (r, e, otask, handed), for one-launch layers, spread / snake work lists, packed lists and the
//    plain grid stride.
//  * the segment list: prefetched load, copy to LDS, cleaning in place, seg_start_of / seg_state_of, the wave-priority request (the
//    expected-frames rule itself is chain_work.h).  Owns nseg, seg, next_start.
//  * the filter of one task on one group of lanes -- load_state, fetch_wq, update, sandwich, sandwich_pair, pack / unpack, frame,
//    piece_value / reset_piece, mean_sum -- over col (PAIR: colh), wq, L, sgd, wown, accq, P, E, nv, s2_now.  Knows nothing of tables.
//  * the table side -- record_of, load_cols, start_from / start_run, begin_chain, the walk plan, land, compare_with_table -- over
//    t, t_check, extra, nrun, open_run, s, s_loaded, the trajectory pointers and the one-frame prefetch (xc / xn / pc / pn).  It
//    drives the filter.
//  * the frame loops: the lean one (kLean: the launch over the work lists) and the general one.
//
// Live from one frame to the next in the LEAN loop: the filter state (colh in the two-row frame, col otherwise; L, sgd, wq, accq,
// P, E, nv), t, t_event, next_start, t_check, seg, s, open_run, nrun, extra, the prefetched frame (xn, pn) and the trajectory
// pointers (px, pprobe).  s2 and the switch the segment began with are NOT: they live in the row's LDS constants (row_const), and
// whatever else a lambda captures costs registers across the loop -- two more cost the geometries short of them a round of spills.
//
// Code that runs only in table-building launches: write_record with dump (DUMP: the prefix table) and dump_state / dump_pair_state
// (BUILD: the state tables) in the general frame loop, and the transient / pair entry written in the epilogue (BUILD).  None of it
// is compiled into the lean loop.
//
// The LDS of a workgroup is laid out by LdsLayout (common.h), for this function, logl_one_kernel / walk_one and the host alike.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <limits.h>

#include "chain_work.h"
#include "config.h"
#include "common.h"
#include "frame_ops.h"

// ---- compile-time switches of this file (A/B and diagnostics builds: tools/ab.py) ------------------------------------------
#ifndef BILD_SNAKE
#define BILD_SNAKE 1 // (0: every layer of a spread work list in the same direction -- A/B builds)
#endif
#ifndef BILD_SPREAD_ALWAYS
#define BILD_SPREAD_ALWAYS 1 // (0: work lists longer than the grid has rows are packed, neighbouring slots to one wave)
#endif
// expected frames of a wave's busiest row from which it asks for issue priority 1 / 2 / 3 (logl_body, "wave priority")
#ifndef BILD_PRIO_T1
#define BILD_PRIO_T1 100
#endif
#ifndef BILD_PRIO_T2
#define BILD_PRIO_T2 130
#endif
#ifndef BILD_PRIO_T3
#define BILD_PRIO_T3 160
#endif
#ifndef BILD_JUMP_FIRST
#define BILD_JUMP_FIRST 24 // first comparison with the table this many frames behind a switch
#endif
// timing experiments only (wrong results), off unless defined: BILD_X_NOLOAD (what the trajectory loads cost),
// BILD_EXPERIMENT_NO_SANDWICH (what the basis change itself costs)
// BILD_TASK_CLOCK = 1 .. 4: the diagnostics builds of TaskClock below

namespace bild {
namespace {

// The task clock of the diagnostics builds (-DBILD_TASK_CLOCK=<mode>; decoded by tools/task_clock.py, tools/listed_clock.py): what
// a task writes to KParams::frames_task in place of the frames it ran.  Mode 1: the low 16 bits of the clock at the task's begin and
// end; 2: ticks inside looks at the table (and the jumps behind them) and their number; 3: ticks / 2 from the begin to the end of
// stage a (descriptor read, segment list cleaned), b (state vectors loaded, plan written) and c (tables walked), 10 bits each;
// 4: as 2 for basis changes.  Without the switch the type is empty, every call compiles to nothing and the word is the frame count.
#ifdef BILD_TASK_CLOCK
struct TaskClock {
    enum Event { kLook = 2, kBasisChange = 4 };
    unsigned long long begin = 0, a = 0, b = 0, c = 0, ev0 = 0, events = 0;
    int n_events = 0;
    __device__ __forceinline__ void task_begins() { begin = wall_clock64(); }
    __device__ __forceinline__ void stage_a() { if (BILD_TASK_CLOCK == 3) a = wall_clock64(); }
    __device__ __forceinline__ void stage_b() { if (BILD_TASK_CLOCK == 3) b = c = wall_clock64(); }
    __device__ __forceinline__ void stage_c() { if (BILD_TASK_CLOCK == 3) c = wall_clock64(); }
    __device__ __forceinline__ void event_begins(int kind)
    {
        if (kind == BILD_TASK_CLOCK) ev0 = wall_clock64();
    }
    __device__ __forceinline__ void event_ends(int kind)
    {
        if (kind == BILD_TASK_CLOCK) {
            events += wall_clock64() - ev0;
            ++n_events;
        }
    }
    __device__ __forceinline__ int32_t word(int) const
    {
        if (BILD_TASK_CLOCK == 3)
            return (int32_t)(((((a - begin) / 2) & 0x3ff) << 20) | ((((b - begin) / 2) & 0x3ff) << 10) | (((c - begin) / 2) & 0x3ff));
        if (BILD_TASK_CLOCK == 2 || BILD_TASK_CLOCK == 4) return (int32_t)(((events & 0xffffull) << 16) | (unsigned)n_events);
        return (int32_t)(((begin & 0xffffull) << 16) | (wall_clock64() & 0xffffull));
    }
};
#else
struct TaskClock {
    enum Event { kLook = 2, kBasisChange = 4 };
    __device__ __forceinline__ void task_begins() {}
    __device__ __forceinline__ void stage_a() {}
    __device__ __forceinline__ void stage_b() {}
    __device__ __forceinline__ void stage_c() {}
    __device__ __forceinline__ void event_begins(int) {}
    __device__ __forceinline__ void event_ends(int) {}
    __device__ __forceinline__ int32_t word(int nrun) const { return nrun; }
};
#endif

// FLAVOR selects what the frame loop has to carry:
//   0: external force (G != 0) and missing frames   1: missing frames   2: neither (every frame valid)
// LAY: 0 packed groups of G consecutive lanes; 1 a group is a 16-lane block of the f64 4x4x4 matrix instruction
// (S as a block sum on the matrix pipe); 2 a group is a 16-lane row, cross-lane operands by DPP row broadcast;
// 3 / 4: the row / the packed layout in the instantiation that serves the frame loop over the work lists only (kLean)
// DUMP: this instantiation builds the prefix table (one per chain length is compiled, see launch_geom)
// JUMP: this instantiation carries the machinery that takes frames out of the tables (convergence checks, transient table);
// the frame-by-frame instantiation stays lean (the jump code costs registers the frame loop then spills around)
// BUILD: the JUMP instantiation that builds the transient / pair / state tables (KParams::trans_dump, trans2_dump) -- and the only one
// that can: what a builder needs (entries, state records) stays out of the evaluating kernels, and what they need (tails, walk plan,
// landing on tables that do not exist yet) out of the builders.  (The tail code of round 4 cost the builders 70 % while it was
// compiled into both: configs[3] tables 234 -> 406 ms.)
// PAIR: the two-row frame of the listed loop (LAY 3 only, see logl_kernel): a task runs on a pair of rows, lane j of the even
// row holds the even entries of column j of [C | M], the odd row the odd ones -- half the predict, dot and rank-1 instructions of
// a frame.  The events work on the halves too: a basis change computes in each row the outputs that row keeps (sandwich_pair), a
// look at the table takes its maxima over the row's entries and exchanges them (compare_with_table) -- whole columns exist only as
// the input of a basis change, in the tail of a look and where a record is loaded.  Whatever decides a branch is exchanged first, so
// both rows hold the same bits there and take the same branches.
// ONE: the listed frame loop of the one-launch path (logl_one_kernel): the workgroup's own table walk (walk_one) has left its listed
// tasks in LDS (OneHand), dealt heaviest first, and the lists and plans of the first layer in the LDS areas of the rows that run
// them.  Such a task starts at the state vectors; one of a later layer (more tasks than rows) runs the whole prologue.
template <int NP, int CPL, int G, int W, int OCC, int LAY, int MODE, int FLAVOR, bool DUMP, bool JUMP, bool BUILD, bool PAIR = false,
          bool ONE = false>
__device__ __forceinline__ void logl_body(const KParams &p, const OneHand *hand = nullptr)
{
    constexpr bool HASG = FLAVOR == 0;
    constexpr bool ALLVALID = FLAVOR == 2;
    constexpr int kThreads = 64 * W;
    constexpr int kWaves = W;
    constexpr int GPW = 64 / G;          // groups (= tasks in flight) per wavefront
    // block layout: a group is one 16-lane block of the f64 4x4x4 matrix instruction (lanes that share
    // bits 2-3), so that S = s2 + w.(Cw) is a block sum on the matrix pipe
    constexpr bool BLK = LAY == 1;
    constexpr bool ROW = LAY == 2 || LAY == 3;
    // the frame loop over the work lists ONLY (geometries 23 / 24 / 25): never builds a table, so the instantiation carries none
    // of the builders' tests in its frame loop, and has a frame loop of its own (below)
    constexpr bool kLean = LAY == 3 || LAY == 4; // (4: the packed layout, likewise for the listed launch only)
    static_assert(!(BLK && JUMP), "the block layout runs frame by frame only (see BILD_GEOMETRIES)");
    static_assert(LAY == 0 || LAY == 4 || (G == 16 && CPL == 1), "block / row layouts: 16 lanes per task, one column per lane");
    constexpr int MS = table_stride(NP); // LDS matrix stride
    constexpr int SB = StateBlock::size(NP);
    static_assert(NP % 2 == 0, "rows are read in pairs");
    // mean columns a group has room for; the host only selects a geometry whose MC covers the largest
    // number of dimensions any covariance chain of the trajectory set carries (Geometry::mean_slots)
    constexpr int MC = (CPL * G - NP < kDMax) ? CPL * G - NP : kDMax;
    static_assert(MC >= 1, "not enough columns for [C | M]");

    extern __shared__ __align__(16) double smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int grp = BLK ? ((lane >> 2) & 3) : lane / G;
    const int gl = BLK ? ((lane & 3) | ((lane >> 4) << 2)) : lane - grp * G; // ROW: lane / 16, lane % 16
    static_assert(!PAIR || (LAY == 3 && CPL == 1 && JUMP && !DUMP && !BUILD), "the row pair serves the listed frame loop only");
    // tasks per wavefront, this lane's task among them, and its row of the pair (PAIR: each row keeps its own LDS areas)
    constexpr int TPW = PAIR ? GPW / 2 : GPW;
    const int tgrp = PAIR ? grp >> 1 : grp;
    const int odd = PAIR ? (grp & 1) : 0;
    const bool lead = gl == 0 && !odd; // the lane that writes the task's results

    // Work lists (walk.hip): this launch runs only the tasks the table walk handed on -- kWorkBuckets lists by expected
    // work, dealt out heaviest first.  Slot q of that order goes to (wave, row) so that the heaviest tasks get a wave
    // each while they fit (the other rows of the wave then idle: a row's events -- basis change, comparison, jump --
    // are paid by the whole wave), the next heaviest the second rows, and so on; lists longer than the grid has rows
    // are throughput-bound and tasks of similar work share a wave.
    static_assert(!ONE || (LAY == 3 && JUMP && !DUMP && !BUILD), "the one-launch path serves the listed frame loop only");
    const bool listed = JUMP && (ONE || p.work != nullptr);
    int64_t n_tasks = ONE ? hand->n : p.ntasks;
    if (listed && !ONE) {
        int64_t tot = 0;
        for (int bq = 0; bq < kWorkBuckets; ++bq) tot += p.work_counts[bq];
        n_tasks = tot;
        if ((int64_t)blockIdx.x * kWaves >= tot) return; // (all rows of this workgroup would idle)
    }

    // Matrix tables live in LDS for the whole kernel: the dense propagators are needed every frame,
    // and a modal basis change walks its matrix row by row in a dependent loop -- from L2 that was
    // ~500 cycles per row, 10 us per switch (measured: +89 % kernel time at k = 20).
    // (ONE: staged by logl_one_kernel, in front of the walk)
    constexpr int HDR = state_header_doubles(NP);
    const LdsLayout lay(NP, kWaves * GPW, p.tab_doubles, p.S);
    if constexpr (!ONE) {
        for (int i = tid; i < p.tab_doubles; i += kThreads) smem[i] = p.tab[i];
        // ... and so do the per-state vectors a state switch reloads (lam | wq | sig: the head of each state block)
        for (int i = tid; i < p.S * HDR; i += kThreads) smem[lay.hdr0 + i] = p.states[(size_t)(i / HDR) * StateBlock::size(NP) + i % HDR];
        __syncthreads();
    }
    // per-group scratch: image of X*A, NP + kDMax columns of NP doubles; its first NP doubles
    // double as the all-gather buffer of the update
    if (grp >= GPW) return; // lanes beyond the last whole group (64 % G != 0) idle
    const double *const lds_hdr = smem + lay.hdr0;
    double *const scratch = smem + lay.img0 + (size_t)(wv * GPW + grp) * group_image_doubles(NP);
    // the task's segment list (K1 <= kSegLds): a switch then costs two LDS reads instead of two dependent L2 round trips
    int32_t *const seg_lds = reinterpret_cast<int32_t *>(smem + lay.seg0) + (size_t)(wv * GPW + grp) * (2 * group_seg_doubles());
    // ... and the task's constants of the frame loop.  In a register such a value is live across the whole loop and the first
    // to be spilled -- the reload (scratch memory, vmcnt) then sits in every frame and waits for the trajectory prefetch too
    typedef __attribute__((address_space(3))) double lds_double_t;
    lds_double_t *const row_const = (lds_double_t *)reinterpret_cast<double *>(seg_lds + 2 * kSegLds);
    // walk plan (p.walk_lds): per switch of the task, what the tables hold for it -- see `land`
    lds_double_t *const walk = (lds_double_t *)(smem + lay.walk0) + (size_t)(wv * GPW + grp) * kWalkDoubles;

    int cidx[CPL];
    bool isC[CPL], hasImg[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
        cidx[q] = gl * CPL + q;
        isC[q] = cidx[q] < NP;
        hasImg[q] = cidx[q] < NP + MC; // spare columns have no LDS image (and stay zero)
    }

    const int S = p.S;
    const int d = p.d;
    const int K1 = p.K1;
    const int64_t gstride = (int64_t)gridDim.x * (kWaves * TPW);
    const int64_t n_waves = (int64_t)gridDim.x * kWaves, wave_id = (int64_t)blockIdx.x * kWaves + wv;
    // (listed, and the list fits the rows of the grid: spread -- row j of wave w takes slot j * n_waves + w, every second
    // layer in reverse: the waves that carry the heaviest tasks of one layer get the lightest of the next, or none)
    const bool spread = listed && (BILD_SPREAD_ALWAYS || n_tasks <= gstride);
    // (ONE: position q of the workgroup's deal runs on wave (q + rot) % W, row (pair) q / W of its layer -- the heaviest task of each
    // layer on wave `rot`; rot = residency index, so that the two workgroups of a CU do not put their heaviest tasks on one SIMD)
    const int one_wave = ONE ? (wv + kWaves - (int)(blockIdx.x / 256) % kWaves) % kWaves : 0;

    for (int64_t it = ONE ? 0 : spread ? (int64_t)tgrp : wave_id * TPW + tgrp;; it += ONE ? 1 : spread ? (int64_t)TPW : gstride) {
        int64_t task = it;
        if (ONE) { // `it` counts layers of kWaves * TPW positions
            task = (it * TPW + tgrp) * kWaves + one_wave;
            if (task >= n_tasks) break;
        } else if (spread) { // `it` counts layers of n_waves slots
            if (it * n_waves >= n_tasks) break;
            task = it * n_waves + (BILD_SNAKE && (it & 1) ? n_waves - 1 - wave_id : wave_id);
            if (task >= n_tasks) continue;
        } else if (task >= n_tasks) {
            break;
        }
        int64_t r, otask;
        int e;
        // (ONE: the first layer's list, plan and expected work are in the row's LDS areas already)
        const bool handed = ONE && it == 0;
        if (ONE) {
            otask = hand->task[task];
            r = otask / p.dstar_max;
            e = (int)(otask - r * p.dstar_max);
        } else if (listed) {
            // slot `task` of the buckets laid end to end, heaviest (last) bucket first
            int64_t q = task;
            int bq = kWorkBuckets - 1;
            for (; bq > 0; --bq) {
                const int c = p.work_counts[bq];
                if (q < c) break;
                q -= c;
            }
            otask = p.work[(int64_t)bq * p.work_cap + q];
            r = otask / p.dstar_max;
            e = (int)(otask - r * p.dstar_max);
        } else {
            const int64_t slot = task / p.dstar_max;
            e = (int)(task - slot * p.dstar_max);
            r = p.order ? p.order[slot] : slot; // launch order is a scheduling matter only
            otask = r * p.dstar_max + e;
        }
        TaskClock clk; // (diagnostics builds only: empty otherwise)
        clk.task_begins();
        // (the listed frame loop: a lone task's prologue is a string of dependent memory round trips -- the task's list is asked
        // for HERE, beside the trajectory descriptor, not behind it; lane i holds entry i, lists of up to kSegLds segments)
        int32_t pre_start = 0, pre_state = 0;
        if constexpr (kLean) {
            if (!handed && K1 <= kSegLds && gl < K1) {
                pre_start = p.seg_start[r * K1 + gl];
                pre_state = p.seg_state[r * K1 + gl];
            }
        }
        const int tj = p.traj_id ? p.traj_id[r] : 0;
        const TrajDesc *__restrict__ td = p.trajs + tj;
        if (e >= td->dstar) {
            if (lead) p.out[otask] = 0.0;
            continue;
        }
        const int T = td->T;
        const double s2 = td->s2[e];
        if (ROW) {
            if (gl == 0) row_const[0] = odd ? 0.0 : s2; // (PAIR: the S sum of the odd row starts from 0, see update)
            wave_lds_fence();
        }
        double s2_now = odd ? 0.0 : s2; // ROW: read again from LDS at the top of every frame (see row_const)
        const int nd = td->ndims[e];

        bool isM[CPL];
        int xoff[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int mi = cidx[q] - NP;
            isM[q] = (mi >= 0) && (mi < nd);
            xoff[q] = isM[q] ? td->dims[e][mi] : 0;
        }

        // Trajectory stream.  The pointers come out of memory: tell the compiler they are global,
        // or every load becomes a flat_load (which also ties up lgkmcnt).  Each own column walks
        // its own coordinate with a running pointer; columns that are not mean columns read a
        // zero word with stride 0, so that  e = w.col - x  is the innovation sign-flipped for a
        // mean column and plain Cw_j for a covariance column -- one formula, no selects.  The
        // device copy has one padding row per trajectory: fetching one frame ahead never leaves it.
        typedef const __attribute__((address_space(1))) double *gptr_t;
        gptr_t px[CPL];
        int xstep[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            px[q] = isM[q] ? (gptr_t)td->x + xoff[q] : (gptr_t)p.zeros;
            xstep[q] = isM[q] ? d : 0;
        }
        gptr_t pprobe = (gptr_t)td->x; // coordinate 0 is NaN <=> frame missing
        auto fetch = [&](double (&xv)[CPL], double &probe) {
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
#ifdef BILD_X_NOLOAD // timing experiment only (wrong results): what the trajectory loads cost
                xv[q] = 0.25;
#else
                xv[q] = *px[q];
#endif
                px[q] += xstep[q];
            }
            if (!ALLVALID) {
                probe = *pprobe;
                pprobe += d;
            } else {
                probe = 0.0;
            }
        };

        const int32_t *__restrict__ sst = p.seg_start + r * K1;
        const int32_t *__restrict__ ssv = p.seg_state + r * K1;
        // The segment list as given may hold boundaries that are no switches (a segment in the state of its predecessor),
        // empty segments (equal starts) and segments beyond the trajectory.  Lists of up to kSegLds segments are copied
        // to LDS and cleaned there, in place: what remains are the real switches inside the trajectory, strictly
        // increasing -- so that a result depends on the expanded profile only, not on how it was encoded, and a switch
        // costs two LDS reads instead of two dependent L2 round trips.  Longer lists are walked in global memory.
        const bool seg_in_lds = K1 <= kSegLds;
        int nseg = K1;
        if (handed) {
            nseg = __double2loint(walk[1]);
        } else if (seg_in_lds) {
            volatile int32_t *const sl = seg_lds;
            if constexpr (kLean && (BLK || ROW)) { // (16 lanes per task: one entry per lane, loaded at the top of the task)
                if (gl < K1) {
                    sl[gl] = pre_start;
                    sl[kSegLds + gl] = pre_state;
                }
            } else {
                for (int i = gl; i < K1; i += (BLK || ROW) ? 16 : G) {
                    sl[i] = sst[i];
                    sl[kSegLds + i] = ssv[i];
                }
            }
            wave_lds_fence();
            int cnt = 1, prev = sl[kSegLds];
            for (int i = 1; i < K1; ++i) {
                const int st0 = sl[i], sv = sl[kSegLds + i];
                const int end = (i + 1 < K1) ? sl[i + 1] : INT_MAX;
                if (st0 >= T) break;                    // starts are sorted: nothing behind this one is inside either
                if (end <= st0 || sv == prev) continue; // empty, or not a change of state
                sl[cnt] = st0;                          // cnt <= i: entries still to be read are not touched
                sl[kSegLds + cnt] = sv;
                prev = sv;
                ++cnt;
            }
            nseg = cnt;
            wave_lds_fence();
        }
        auto seg_start_of = [&](int i) { return seg_in_lds ? seg_lds[i] : sst[i]; };
        auto seg_state_of = [&](int i) { return seg_in_lds ? seg_lds[kSegLds + i] : ssv[i]; };
        // Wave priority.  The launch ends when its longest chain of short segments has been run, frame by frame, by ONE
        // row -- on a SIMD shared with two other waves that mostly have slack.  A wave that expects a long run asks the
        // issue arbiter for priority (frames to run estimated from the switch frames, as the host scheduler does: chain_work.h,
        // over the cleaned list in LDS):
        // 136 -> 119 us for the 10k batch in array order, 116 -> 114 us in the scheduler's order
        // (profiles/r02_wave_priority.txt).  A matter of speed only.
        if (JUMP && seg_in_lds && p.trans != nullptr) {
            ChainWork cw{p.m_typ, p.trans2 != nullptr};
            if (handed) cw.w = __double2hiint(walk[1]); // (the walk's estimate: the same rule on the same list)
            for (int i = 1; i < (handed ? 0 : nseg); ++i) {
                const int t1 = seg_lds[i];
                cw.add(t1, ((i + 1 < nseg) ? seg_lds[i + 1] : T) - t1);
            }
            const int w = cw.finish(T); // (handed: no chain is open, the estimate stays the walk's)
            if (__ballot(w >= BILD_PRIO_T3)) __builtin_amdgcn_s_setprio(3);
            else if (__ballot(w >= BILD_PRIO_T2)) __builtin_amdgcn_s_setprio(2);
            else if (__ballot(w >= BILD_PRIO_T1)) __builtin_amdgcn_s_setprio(1);
            else __builtin_amdgcn_s_setprio(0);
        }
        int seg = 0;
        int s = seg_state_of(0);
        clk.stage_a(); // descriptor read, segment list cleaned
        int next_start = (nseg > 1) ? seg_start_of(1) : INT_MAX;

        // ---- per-state registers -------------------------------------------------
        // measurement vector in the current basis.  Row layout, jump instantiation: NOT kept in registers -- the same for
        // all lanes of a row, it is read from the state header in LDS at the top of every update (five 16-byte reads, behind
        // the predict), and the twenty registers go to the event paths, which otherwise spill around the frame loop
        // (at two waves per SIMD -- the geometry of the frame loop over the work lists, id 23 -- there are registers enough:
        // a lone wave then does not wait for five LDS reads in front of every update)
        constexpr bool kWqFromLds = ROW && JUMP && OCC >= 3;
        double wq[NP];
        // modal predict  C'_ij <- lam_i lam_j C'_ij + sig_i delta_ij,  M'_i <- lam_i M'_i  as ONE
        // fma per entry: L[q][i] = lam_i * (lam_c or 1), sgd[i] = sig_c on the own diagonal entry
        // (row i == column c of column slot q = i % CPL) and 0 elsewhere.  Rebuilt at switches.
        Cols<NP, CPL> L;
        double sgd[NP];
        double wown = 0.0; // block layout: w_c of the own covariance column, 0 for the other lanes
        auto load_state = [&](int st) {
            const double *__restrict__ sb = lds_hdr + (size_t)st * HDR; // lam | wq | sig at the offsets of the state block
            if constexpr (PAIR) { // (the row's entries only: entry k of wq, L, sgd is entry 2k + odd)
                const double mu = isC[0] ? sb[StateBlock::lam(NP) + cidx[0]] : (hasImg[0] ? 1.0 : 0.0);
                const double sgc = isC[0] ? sb[StateBlock::sig(NP) + cidx[0]] : 0.0;
#pragma unroll
                for (int k = 0; k < NP / 2; ++k) {
                    const int i = 2 * k + odd;
                    wq[k] = sb[StateBlock::wq(NP) + i];
                    L.v[0][k] = sb[StateBlock::lam(NP) + i] * mu;
                    sgd[k] = (gl == i) ? sgc : 0.0;
                }
                return;
            }
            if constexpr (!kWqFromLds) {
#pragma unroll
                for (int i = 0; i < NP; ++i) wq[i] = sb[StateBlock::wq(NP) + i];
            }
            if (BLK) wown = isC[0] ? sb[StateBlock::wq(NP) + cidx[0]] : 0.0;
            if (MODE == kModal) {
                double mu[CPL], sgc[CPL];
#pragma unroll
                for (int q = 0; q < CPL; ++q) {
                    const int cc = isC[q] ? cidx[q] : 0;
                    mu[q] = isC[q] ? sb[StateBlock::lam(NP) + cc] : (hasImg[q] ? 1.0 : 0.0);
                    sgc[q] = isC[q] ? sb[StateBlock::sig(NP) + cc] : 0.0;
                }
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const double li = sb[StateBlock::lam(NP) + i];
#pragma unroll
                    for (int q = 0; q < CPL; ++q) L.v[q][i] = li * mu[q];
                    sgd[i] = (gl == i / CPL) ? sgc[i % CPL] : 0.0;
                }
            }
        };
        load_state(s);

        // ---- initial condition: steady state of state profile[0] (pyx:160-163) ----
        // (a task that starts from a table -- every task of the jump instantiation -- loads its state there: start_from)
        Cols<NP, CPL> col;
        // PAIR: the row's half of its column in the frame loop (entry k = entry 2k + odd of col); col itself is live at events only
        double colh[PAIR ? NP / 2 : 1];
        auto pack = [&]() {
            if constexpr (PAIR) {
#pragma unroll
                for (int k = 0; k < NP / 2; ++k) colh[k] = odd ? col.v[0][2 * k + 1] : col.v[0][2 * k];
            }
        };
        auto unpack = [&]() {
            if constexpr (PAIR) {
#pragma unroll
                for (int k = 0; k < NP / 2; ++k) pair_swap(colh[k], col.v[0][2 * k], col.v[0][2 * k + 1]);
            }
        };
        if (JUMP && p.prefix != nullptr && !p.no_jump) {
#pragma unroll
            for (int q = 0; q < CPL; ++q)
#pragma unroll
                for (int i = 0; i < NP; ++i) col.v[q][i] = 0.0;
        } else {
            const double *__restrict__ sb = p.states + (size_t)s * SB;
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const double *src = isC[q] ? sb + StateBlock::C0(NP) + cidx[q] * NP
                                           : sb + StateBlock::M0(NP) + xoff[q] * NP;
                const double live = (isC[q] || isM[q]) ? 1.0 : 0.0;
#pragma unroll
                for (int i = 0; i < NP; ++i) col.v[q][i] = live * src[i];
            }
        }

        pack(); // (PAIR: from here on the halves are the state)

        double accq[CPL]; // per own column: sum of e^2 / S (meaningful for mean columns)
#pragma unroll
        for (int q = 0; q < CPL; ++q) accq[q] = 0.0;
        double P = 1.0; // running product of S (mantissa), exponent in E
        int E = 0;
        int nv = 0;     // observed frames behind these accumulators

        // ---- Kalman update (pyx:19-90) ---------------------------------------------
        auto fetch_wq = [&]() { // (kWqFromLds) at the top of every update: issued behind the predict by the scheduler
            if constexpr (kWqFromLds) {
                typedef double __attribute__((ext_vector_type(2))) d2_t;
                typedef const __attribute__((address_space(3))) d2_t *wq_ptr_t; // (the address moves with s: nothing to hoist)
                const wq_ptr_t wp = (wq_ptr_t)(lds_hdr + (size_t)s * HDR + StateBlock::wq(NP));
#pragma unroll
                for (int i = 0; i < NP; i += 2) {
                    const d2_t w2 = wp[i / 2];
                    wq[i] = w2.x;
                    wq[i + 1] = w2.y;
                }
            }
        };
        auto update = [&](const double (&xv)[CPL]) {
            if constexpr (PAIR) {
                // the row's half of every sum, then the two halves added in the order of the one-row frame (even + odd)
                double a = 0.0;
#pragma unroll
                for (int k = 0; k < NP / 2; ++k) a = fma(wq[k], colh[k], a);
                double a0, a1;
                pair_swap(a, a0, a1);
                const double ev = (a0 + a1) - xv[0];
                double evs = odd_rows_shift(ev); // lane 2k of the row: (C w) entry 2k + odd
                dpp_ready(evs);
                double sr = s2_now; // (s2 in the even row, 0 in the odd one: row_const[0])
                PairOps<NP>::dot(sr, evs, wq);
                double sa, sb2;
                pair_swap(sr, sa, sb2);
                const double Sv = sa + sb2;
                double Sinv = __builtin_amdgcn_rcp(Sv);
                Sinv = fma(fma(-Sv, Sinv, 1.0), Sinv, Sinv);
                Sinv = fma(fma(-Sv, Sinv, 1.0), Sinv, Sinv);
                const double coef = ev * Sinv;
                accq[0] = fma(ev, coef, accq[0]);
                PairOps<NP>::rank1(colh, evs, -coef);
                int ex;
                P = frexp(P * Sv, &ex);
                E += ex;
                ++nv;
                return;
            }
            fetch_wq();
            double ev[CPL];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                double a0 = 0.0, a1 = 0.0;
#pragma unroll
                for (int i = 0; i < NP; i += 2) {
                    a0 = fma(wq[i], col.v[q][i], a0);
                    a1 = fma(wq[i + 1], col.v[q][i + 1], a1);
                }
                ev[q] = (a0 + a1) - xv[q]; // covariance column: (C w)_c ; mean column: -(x - w.M)
            }
            if constexpr (ROW) {
                // C w is never gathered: lane i of the row holds (C w)_i in ev and every use reads it by row broadcast
                dpp_ready(ev[0]);
                double sa = s2_now, sb2 = 0.0;
                RowOps<NP>::dot(sa, sb2, ev[0], wq);
                const double Sv = sa + sb2;
                double Sinv = __builtin_amdgcn_rcp(Sv);
                Sinv = fma(fma(-Sv, Sinv, 1.0), Sinv, Sinv);
                Sinv = fma(fma(-Sv, Sinv, 1.0), Sinv, Sinv);
                const double coef = ev[0] * Sinv;
                accq[0] = fma(ev[0], coef, accq[0]);
                RowOps<NP>::rank1(col.v[0], ev[0], -coef); // col[i] += (C w)_i * (-coef) = fma(-coef, cw[i], col[i])
                int ex;
                P = frexp(P * Sv, &ex);
                E += ex;
                ++nv;
                return;
            }
            // every lane publishes (no exec masking): mean / spare columns land behind the NP
            // gathered entries (cidx < CPL*G <= group image size)
#pragma unroll
            for (int q = 0; q < CPL; ++q) scratch[cidx[q]] = ev[q];
            wave_lds_fence();
            double cw[NP];
#pragma unroll
            for (int i = 0; i < NP; i += 2) {
                const double2 t2 = *reinterpret_cast<const double2 *>(scratch + i);
                cw[i] = t2.x;
                cw[i + 1] = t2.y;
            }
            wave_lds_fence();
            double Sv;
            if (BLK) {
                Sv = block_sum16(wown * ev[0], s2);
            } else {
                double sa = s2, sb2 = 0.0;
#pragma unroll
                for (int i = 0; i < NP; i += 2) {
                    sa = fma(wq[i], cw[i], sa);
                    sb2 = fma(wq[i + 1], cw[i + 1], sb2);
                }
                Sv = sa + sb2;
            }
            // 1/S: hardware reciprocal seed + two Newton steps (full double precision for the
            // normal, positive S a covariance produces; NaN/Inf/0 propagate as such)
            double Sinv = __builtin_amdgcn_rcp(Sv);
            Sinv = fma(fma(-Sv, Sinv, 1.0), Sinv, Sinv);
            Sinv = fma(fma(-Sv, Sinv, 1.0), Sinv, Sinv);
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const double coef = ev[q] * Sinv; // K_c * S for a covariance column, -nu/S for a mean column
                accq[q] = fma(ev[q], coef, accq[q]); // e^2 / S
#pragma unroll
                for (int i = 0; i < NP; ++i) col.v[q][i] = fma(-coef, cw[i], col.v[q][i]);
            }
            int ex;
            P = frexp(P * Sv, &ex);
            E += ex;
            ++nv;
        };

        // A <- X A for all columns, then C <- C X^T for the covariance part: two lane-local
        // multiplies, each streamed through the group's LDS image; the covariance columns are
        // read back TRANSPOSED after the first one (row c of X*C is column c of (X*C)^T, and
        // X (X C)^T = (X C X^T)^T = X C X^T).  Used for the dense predict (X = B_s) and the
        // modal basis change (X = R).  `after_left` runs on the mean columns between the
        // two multiplies (adds G in the dense predict).
        auto sandwich = [&](auto X, auto &&after_left) {
            matvec_to_lds<NP, CPL, (JUMP && ((ROW && OCC <= 2) || kLean))>(X, col, scratch, cidx, hasImg);
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                // covariance: walk row c of the image; mean: own column; spare: anything in range
                // (tried: storing the covariance block ACROSS the image, so that this transposed read becomes five 16-byte
                // reads and one wait instead of ten 8-byte reads each waited for -- the basis change gained 0.1 us and the
                // frame loop, re-allocated by the compiler, lost 0.04 us per frame: 53.7 -> 56.9 us at k = 4; dropped)
                const int c = isC[q] ? cidx[q] : (hasImg[q] ? cidx[q] * NP : 0);
                const int st = isC[q] ? NP : 1;
                const double keep = hasImg[q] ? 1.0 : 0.0;
                if constexpr (JUMP && ((ROW && OCC <= 2) || kLean)) {
                    // (all reads in flight, ONE wait: the compiler's own order is read, wait, multiply, ten times over)
                    double tmp[NP];
#pragma unroll
                    for (int i = 0; i < NP; ++i) tmp[i] = scratch[c + i * st];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < NP; ++i) col.v[q][i] = keep * tmp[i];
                } else {
#pragma unroll
                    for (int i = 0; i < NP; ++i) col.v[q][i] = keep * scratch[c + i * st];
                }
            }
            wave_lds_fence();
            after_left();
            matvec_to_lds<NP, CPL, (JUMP && ((ROW && OCC <= 2) || kLean))>(X, col, scratch, cidx, isC);
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q < CPL; ++q)
                if (isC[q]) {
#pragma unroll
                    for (int i = 0; i < NP; i += 2) {
                        const double2 t2 = *reinterpret_cast<const double2 *>(scratch + cidx[q] * NP + i);
                        col.v[q][i] = t2.x;
                        col.v[q][i + 1] = t2.y;
                    }
                }
            wave_lds_fence();
        };

        // The basis change of a PAIR, split over its rows: both products need whole columns as input (unpacked once, in front),
        // but each row computes only the outputs it keeps -- entries 2k + odd.  Left product: a mean column's outputs are its new
        // colh already; the covariance columns' go to ONE image shared by the pair (the even row's area), from which row c is read
        // back transposed, whole.  Right product: its outputs ARE colh -- no second image, no second read-back, no pack().  Half
        // the FMAs and half the matrix reads of `sandwich` per lane, and every output sees the operands of the one-row frame in
        // the same order.  (A spare column is zero and stays zero.)
        auto sandwich_pair = [&](auto X) {
            if constexpr (PAIR) {
                constexpr int H = NP / 2;
                double *const img = scratch - odd * group_image_doubles(NP);
                unpack();
                double left[H], right[H];
                matvec_pair<NP, true>(X + odd * NP, col.v[0], left, img + cidx[0] * NP + odd, isC[0]);
                wave_lds_fence();
                {
                    const int c = isC[0] ? cidx[0] : 0; // (the other lanes: anything in range, their product is not kept)
                    double tmp[NP];
#pragma unroll
                    for (int i = 0; i < NP; ++i) tmp[i] = img[c + i * NP];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < NP; ++i) col.v[0][i] = tmp[i];
                }
                matvec_pair<NP, false>(X + odd * NP, col.v[0], right, nullptr, false);
#pragma unroll
                for (int k = 0; k < H; ++k) colh[k] = isC[0] ? right[k] : (hasImg[0] ? left[k] : 0.0);
                wave_lds_fence(); // (the image is read: the next writer of the area may come)
            }
        };

        constexpr int kJumpFirst = BILD_JUMP_FIRST; // first comparison this many frames behind a switch
        int t_check = 0; // frame index (frames < t_check are processed) at which the next convergence check is due
        int s_loaded = s; // state whose vectors (wq, L, sgd) are in registers
        // the switch the current segment began with -- its frame, and the state in front of it (first-order tail) -- lives in the
        // task's second LDS constant: two registers live across the frame loop cost the geometries that are short of them
        // another round of spills (the pair table's builder, (2, 7): 420 -> 700 us when they were registers)
        // (the word's upper half, bits 16 and up of the hi word: the switch the task's current chain began with -- begin_chain, read
        // by the switch tail of a look; a switch inside the chain carries it on, one LDS read at an event, nothing in a frame)
        auto note_switch = [&](int s_from, int t_seg) {
            row_const[1] = __hiloint2double(s_from, t_seg);
        };
        constexpr int kNoteState = 0xffff;
        static_assert(kSegLds < (1 << 14), "a switch index fits the upper half of the noted word");
        note_switch(s, 0);
        // frame t is the first of a new segment: state bookkeeping, and the basis change of a real switch
        auto enter_segment = [&](int t) {
            {
                do {
                    ++seg;
                    next_start = (seg + 1 < nseg) ? seg_start_of(seg + 1) : INT_MAX;
                } while (t >= next_start); // (never loops on a cleaned list)
                const int sn = seg_state_of(seg);
                if (sn != s) {
                    if (MODE == kModal) {
                        // basis change: one matrix R[sn][s], or -- many states -- out of the old basis (Q[s]) and
                        // into the new one (Q[sn]^T)
                        const int steps = p.tab_factored ? 2 : 1;
                        clk.event_begins(TaskClock::kBasisChange);
                        for (int st = 0; st < steps; ++st) {
                            const int slot = p.tab_factored ? (st == 0 ? s : S + sn) : sn * S + s;
#ifndef BILD_EXPERIMENT_NO_SANDWICH // timing experiment only (wrong results): what the basis change itself costs
                            if constexpr (PAIR) sandwich_pair(const_cast<const double *>(smem) + (size_t)slot * MS);
                            else sandwich(const_cast<const double *>(smem) + (size_t)slot * MS, [] {});
#endif
                        }
                        clk.event_ends(TaskClock::kBasisChange);
                    }
                    int carried = 0;
                    if constexpr (JUMP && !BUILD) carried = __double2hiint(row_const[1]) & ~kNoteState;
                    note_switch(s | carried, t);
                    s = sn;
                    load_state(s);
                    s_loaded = s;
                    t_check = t + kJumpFirst;
                }
            }
        };
        // one frame t >= 1: predict (pyx:206-241), masked update (pyx:244-248)
        auto frame = [&](const double (&xv)[CPL], double probe) {
            if (ROW && kLean) {
                // (issued HERE: the scheduler sinks the read to just in front of the S sum it starts, and every frame then waits
                // for LDS between its two dot products -- in front of the predict the latency hides behind ten FMAs)
                s2_now = row_const[0];
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (PAIR) {
#pragma unroll
                for (int k = 0; k < NP / 2; ++k) colh[k] = fma(L.v[0][k], colh[k], sgd[k]);
                if (HASG && isM[0]) {
                    const double *__restrict__ gb = p.states + (size_t)s * SB + StateBlock::G(NP) + xoff[0] * NP + odd;
#pragma unroll
                    for (int k = 0; k < NP / 2; ++k) colh[k] += gb[2 * k];
                }
            } else if (MODE == kModal) {
#pragma unroll
                for (int q = 0; q < CPL; ++q)
#pragma unroll
                    for (int i = 0; i < NP; ++i)
                        col.v[q][i] = (q == i % CPL) ? fma(L.v[q][i], col.v[q][i], sgd[i]) : L.v[q][i] * col.v[q][i];
                if (HASG) {
                    const double *__restrict__ gb = p.states + (size_t)s * SB + StateBlock::G(NP);
#pragma unroll
                    for (int q = 0; q < CPL; ++q)
                        if (isM[q]) {
#pragma unroll
                            for (int i = 0; i < NP; ++i) col.v[q][i] += gb[xoff[q] * NP + i];
                        }
                }
            } else {
                const double *__restrict__ sb = p.states + (size_t)s * SB;
                constexpr bool has_G = HASG;
                sandwich(const_cast<const double *>(smem) + (size_t)s * MS, [&] {
                    if (has_G) {
#pragma unroll
                        for (int q = 0; q < CPL; ++q)
                            if (isM[q]) {
#pragma unroll
                                for (int i = 0; i < NP; ++i) col.v[q][i] += sb[StateBlock::G(NP) + xoff[q] * NP + i];
                            }
                    }
                });
                // + Sig[:, c] (symmetric: row c of the LDS copy)
                const double *__restrict__ sg = smem + (size_t)(S + s) * MS;
#pragma unroll
                for (int q = 0; q < CPL; ++q)
                    if (isC[q]) {
#pragma unroll
                        for (int i = 0; i < NP; i += 2) {
                            const double2 t2 = *reinterpret_cast<const double2 *>(sg + cidx[q] * NP + i);
                            col.v[q][i] += t2.x;
                            col.v[q][i + 1] += t2.y;
                        }
                    }
            }
            if (ALLVALID || !isnan(probe)) update(xv);
        };

        // ---- which frames to run at all ------------------------------------------------------------------------------
        // Without tables: frame 0 is an update on the steady state without a predict (pyx:186-190), then every frame.
        // With the tables of the trajectory set (common.h), a task runs only where its filter differs from the switch-free
        // filter of its current state:
        //  * the part in front of its first switch is a difference of the running log-likelihood L_s(t) of that filter;
        //  * behind a switch the filter forgets where it came from at a geometric rate (a few tens of frames for a Rouse
        //    chain).  From kJumpFirst frames behind the switch on -- and then after as many frames as the measured deviation
        //    still needs at the usual rate of decay -- the task compares its whole state [C | M] with the table's record of
        //    the same frame and state.  Equal states, same propagator and same data give equal futures: once they agree to
        //    kJumpTol (relative to the largest entry of each column), the rest of the segment is again a difference of
        //    L_s(t), and the task is back at a "synchronised point" in front of its next switch.  No stationarity is
        //    assumed: a task that never converges (long gaps, slow modes) simply runs every frame;
        //  * a transient that starts at a synchronised point depends on (trajectory, chain, frame, old state, new state)
        //    only -- not on the candidate.  The TRANSIENT TABLE holds, for every such switch, how many frames m it takes to
        //    converge and what it adds to the log-likelihood beyond the table's own sums.  A task whose next switch is at
        //    least m frames away takes that entry and runs nothing.
        // The pieces are sums of O(1e4) numbers taken apart and put together again: a result deviates from the
        // frame-by-frame one by ~1e-11 (BILD_NO_JUMP runs every frame behind the first switch, bit-identical to
        // BILD_NO_PREFIX).  Rows of a wavefront are independent: each has its own frame counter and trajectory pointers.
        constexpr int NC = NP + kDMax;
        constexpr int REC = prefix_record_doubles(NP);
        constexpr int kRecP = NC * NP + kDMax, kRecE = kRecP + 1, kRecL = kRecP + 2, kRecNv = kRecP + 3;
        constexpr double kJumpTol = 1.1368683772161603e-13; // 2^-43
        const bool restore = !DUMP && p.prefix != nullptr;
        const bool jumping = JUMP && restore && !p.no_jump;
        // (launch_geom: a BUILD instantiation is launched when, and only when, p.trans_dump or p.trans2_dump is set -- with the prefix
        // table in place and jumps allowed)
        constexpr bool building_transients = BUILD;
        const bool use_transients = jumping && p.trans != nullptr && !building_transients;
        auto record_of = [&](int st, int t) { return p.prefix + (td->prefix_rec0 + ((int64_t)e * S + st) * T + t) * REC; };
        auto record = [&](int t) { return record_of(s, t); };
        auto load_cols = [&](const double *__restrict__ rec) {
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const double keep = (isC[q] || isM[q]) ? 1.0 : 0.0;
                const double *src = rec + (hasImg[q] ? cidx[q] : 0) * NP;
#pragma unroll
                for (int i = 0; i < NP; i += 2) {
                    const double2 t2 = *reinterpret_cast<const double2 *>(src + i);
                    col.v[q][i] = keep * t2.x;
                    col.v[q][i + 1] = keep * t2.y;
                }
            }
            // (PAIR: whole columns in both rows, five 16-byte loads, then the row's half by selects.  Loading the halves directly --
            // five 8-byte loads per row -- was slower: DESIGN.md section 4)
            pack();
        };
        // lanes of this task, as a mask over the wavefront (for the row-wide verdict of a comparison)
        unsigned long long group_mask;
        if (BLK) group_mask = 0x000F000F000F000Full << (4 * grp);
        else group_mask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << (grp * G);
        // log-likelihood of the frames behind the accumulators (pyx:88, 251-256), the same in every lane of the task
        // sum over the task's mean columns of one value per column, in column order (the same in every lane of the task).  The
        // order must not depend on how columns are dealt to lanes: a lane of a three-column geometry holds two mean columns, and
        // adding those on the lane first made geometry 11 differ from geometry 10 in the last bits at NP = 20.
        auto mean_sum = [&](const double (&v)[CPL]) {
#pragma unroll
            for (int q = 0; q < CPL; ++q)
                if (!isC[q] && hasImg[q]) scratch[cidx[q]] = isM[q] ? v[q] : 0.0;
            wave_lds_fence();
            double tot = 0.0;
#pragma unroll
            for (int m = 0; m < MC; ++m) tot += scratch[NP + m];
            wave_lds_fence();
            return tot;
        };
        auto piece_value = [&]() { return piece_from_sums(mean_sum(accq), P, E, nv, nd); };
        auto reset_piece = [&]() {
#pragma unroll
            for (int q = 0; q < CPL; ++q) accq[q] = 0.0;
            P = 1.0;
            E = 0;
            nv = 0;
        };

        int t = 1;
        int nrun = 0; // frames run: minus the first frame of the open run while it lasts, plus its last frame + 1 when it ends
        double extra = 0.0; // finished pieces: table differences, transient entries, own pieces that have ended
        // the accumulators hold a piece that is not in `extra` yet (lean: an int -- a loop-carried bool of divergent lanes is a lane
        // mask in scalar registers, merged at the bottom of EVERY frame)
        typename std::conditional<kLean, int, bool>::type open_run = 1;
        double xc[CPL], xn[CPL], pc, pn;
        // start a run of own frames at frame t0 from the table's state in front of it; the trajectory pointers stand at
        // frame t_ptr (0 at the start of a task, t + 1 inside the frame loop)
        auto start_from = [&](const double *__restrict__ rec, int t0, bool cumulative, int t_ptr) {
            load_cols(rec);
            if (cumulative) { // accumulators continue the table's (BILD_NO_JUMP: bit-identical to the run from frame 0)
#pragma unroll
                for (int q = 0; q < CPL; ++q) accq[q] = isM[q] ? rec[NC * NP + (cidx[q] - NP)] : 0.0;
                P = rec[kRecP];
                E = (int)rec[kRecE];
                nv = (int)rec[kRecNv];
            } else {
                reset_piece();
            }
            if (s_loaded != s) {
                load_state(s);
                s_loaded = s;
            }
#pragma unroll
            for (int q = 0; q < CPL; ++q) px[q] += (int64_t)xstep[q] * (t0 - t_ptr);
            if (!ALLVALID) pprobe += (int64_t)d * (t0 - t_ptr);
            fetch(xn, pn); // frame t0 (or the first padding row)
            nrun -= t0;
            t_check = t0 + 8; // (a switch at t0 sets its own; lists too long to be cleaned may hold boundaries that switch nothing)
            open_run = 1;
        };
        auto start_run = [&](int t0, bool cumulative, int t_ptr) { start_from(record(t0 - 1), t0, cumulative, t_ptr); };
        // A chain of close switches begins at the synchronised point in front of frame t (the start of segment seg + 1).  With
        // the transient state table (common.h) it begins at its SECOND switch instead: the state the first transient has
        // reached there, accumulators included, is a record of the table -- written by the candidate that built the transient
        // table's entry for this switch, which ran the very same frames from the very same record.
        // (the walk plan, below: the task's table entries are in LDS, lane by lane)
        const bool planned = use_transients && p.walk_lds != 0 && seg_in_lds;
        auto begin_chain = [&](int t_ptr) {
            // the chain's first switch is the one into segment seg + 1, whichever record the chain physically starts from
            const int chain0 = (JUMP && !BUILD) ? (seg + 1 <= kSegLds ? seg + 1 : kSegLds) << 16 : 0;
            if constexpr (JUMP) {
                if (p.strans != nullptr && seg_in_lds && seg + 2 < nseg) {
                    const int sn = seg_state_of(seg + 1), t2 = seg_start_of(seg + 2), g1 = t2 - t;
                    if (sn != s && g1 >= 1 && g1 < p.sgap) {
                        // the table keeps every `sstride`-th gap (g = 1, 1 + sstride, ...): the chain starts from the last
                        // record at or in front of its second switch and runs the frames in between itself (at most
                        // sstride - 1 of them, in the state of the gap) -- the frames the candidate would have run anyway
                        const int q = (g1 - 1) / p.sstride, g0 = 1 + q * p.sstride;
                        const int64_t entry = (((int64_t)e * S + s) * (S - 1) + (sn - (sn > s ? 1 : 0))) * T + t;
                        const double *__restrict__ rec = p.strans + ((td->strans0 + entry) * p.snq + q) * REC;
                        // (the switch the run begins behind, the state it runs in, its next switch and its first frame)
                        int links = 1, s_from = s, t_from = t, s_to = sn, t_next = t2, t_go = t + g0;
                        // With the pair state table (common.h) it begins at its THIRD switch, where the task's prologue has found
                        // that it may (below: "pair state starts"): the plan then holds -1 in place of the pair entry's frame
                        // count, and the record and the frame to go on at in place of its value -- two LDS reads and the same
                        // start, no index arithmetic beside the values the frame loop carries
                        if constexpr (!BUILD) {
                            if (planned && __double2hiint(walk[3 * (seg + 1) + 2]) == -1) {
                                const double at = walk[3 * (seg + 1) + 1];
                                rec = p.pstrans + (int64_t)__double2hiint(at) * REC;
                                links = 2;
                                s_from = sn;
                                t_from = t2;
                                s_to = seg_state_of(seg + 2);
                                t_next = seg_start_of(seg + 3);
                                t_go = __double2loint(at);
                            }
                        }
                        seg += links; // the segment of sn (sm): the frame at t2 (t3) moves on to the next one
                        note_switch(s_from | chain0, t_from);
                        s = s_to;
                        next_start = t_next;
                        t = t_go;
                        start_from(rec, t, true, t_ptr);
                        return;
                    }
                }
            }
            if constexpr (JUMP && !BUILD) {
                const double noted = row_const[1];
                row_const[1] = __hiloint2double((__double2hiint(noted) & kNoteState) | chain0, __double2loint(noted));
            }
            start_run(t, false, t_ptr);
        };
        // The walk plan.  Which table entries a task may need is known from its (cleaned) segment list alone: for the switch
        // into segment i, the transient entry of (state i-1 -> state i, frame start_i) and, where segment i is shorter than the
        // pair table's range, the pair entry of (state i-1 -> i -> i+1, start_i, length of segment i) -- each with the running
        // sums of the new state's filter up to the switch behind.  Lane i - 1 of the task fetches those of switch i, all at
        // once, and leaves the two sums and the two frame counts in LDS; `land` then walks from switch to switch without
        // waiting for memory (four switches: 6.6 -> ~2 us of a task's life; the same numbers, added in the same order).
        if (planned && !handed) {
            for (int i = 1 + gl; i < nseg; i += (BLK || ROW) ? 16 : G) {
                const int ti = seg_lds[i], s0 = seg_lds[kSegLds + i - 1], s1 = seg_lds[kSegLds + i];
                const int n2 = (i + 1 < nseg) ? seg_lds[i + 1] : INT_MAX;
                const int t3 = n2 < T ? n2 : T;
                const TransEntry en = p.trans[td->trans0 + (((int64_t)e * S + s0) * S + s1) * T + ti];
                const double la = record_of(s1, ti - 1)[kRecL], lb = record_of(s1, t3 - 1)[kRecL];
                double v2 = 0.0;
                int m2 = 0;
                if constexpr (kLean) {
                    // every load of the plan in ONE round trip: the pair entry and its running sums are asked for
                    // unconditionally, with indices of entry 0 where there is no pair (walk.hip does the same)
                    const bool pair_ok = p.trans2 != nullptr && n2 < T && n2 - ti < p.gap_max;
                    const int sm = pair_ok ? seg_lds[kSegLds + i + 1] : 0;
                    const int n4 = (pair_ok && i + 2 < nseg) ? seg_lds[i + 2] : INT_MAX;
                    const int t4 = n4 < T ? n4 : T;
                    const TransEntry *tab2 = p.trans2 != nullptr ? p.trans2 : p.trans;
                    const int64_t i2 = pair_ok ? (td->trans0 * S + ((((int64_t)e * S + s0) * S + s1) * S + sm) * T + ti) * p.gap_max + (n2 - ti) : td->trans0;
                    const TransEntry e2 = tab2[i2];
                    const double l4 = record_of(sm, t4 - 1)[kRecL], l2 = record_of(sm, ti - 1)[kRecL];
                    if (pair_ok) {
                        v2 = e2.c + (l4 - l2);
                        m2 = e2.m;
                    }
                } else if (p.trans2 != nullptr && n2 < T && n2 - ti < p.gap_max) {
                    const int sm = seg_lds[kSegLds + i + 1];
                    const int n4 = (i + 2 < nseg) ? seg_lds[i + 2] : INT_MAX;
                    const int t4 = n4 < T ? n4 : T;
                    const TransEntry e2 =
                        p.trans2[(td->trans0 * S + ((((int64_t)e * S + s0) * S + s1) * S + sm) * T + ti) * p.gap_max + (n2 - ti)];
                    v2 = e2.c + (record_of(sm, t4 - 1)[kRecL] - record_of(sm, ti - 1)[kRecL]);
                    m2 = e2.m;
                }
                walk[3 * i] = en.c + (lb - la);
                walk[3 * i + 1] = v2;
                walk[3 * i + 2] = __hiloint2double(m2, en.m);
            }
            // ... and, by the task's last lane (slot 0 belongs to no switch), the running sum in front of the first switch
            if (gl == ((BLK || ROW) ? 15 : G - 1)) {
                const int t1 = (nseg > 1 && seg_lds[1] < T) ? seg_lds[1] : T;
                walk[0] = record_of(seg_lds[kSegLds], t1 - 1)[kRecL];
            }
            wave_lds_fence();
        }
        // Pair state starts.  With the pair state table (common.h) a chain of three and more close switches t1 < t2 < t3 begins at
        // its THIRD switch: the candidate that built the pair entry (t1, g1 = t2 - t1) ran the frames of the gap t2 .. from the
        // same record, through the same code, and left its state behind every pstride-th of them.  Lane i - 1 decides for a
        // chain that begins at switch i -- out of line of the frame loop, from the list and the plan in LDS alone -- and taken
        // it is only where this candidate, started at its second switch, would run EVERY frame up to t3 and end no piece there:
        //  (a) a record exists: g1 inside the pair table (and the first level's gaps), g2 = t3 - t2 inside the covered gaps;
        //  (b) t3 - t1 < m_pair, the pair entry's frame count (hi word of the plan's third slot).  The builder's first look that
        //      converged was the one at frame t1 + m_pair (m_pair = T - t1: none did), and it had written the records of all
        //      frames up to there.  Its looks are this candidate's looks -- same states, same records, same schedule --, so none
        //      of them at a frame <= t3 converges by the full criterion; equality is left out: a look AT t3 comes in front of
        //      the switch.  (`land` cannot take the pair entry either: it would need t1 + m_pair <= t3);
        //  (c) none of them takes a first-order tail: compare_with_table takes one only if t3 - t2 >= m_ref + tail_margin, m_ref > 0
        //      the single entry of the switch at t2 (lo word of switch i + 1's third slot).
        // The looks in the gap then do nothing but schedule the next look, and the switch at t3 schedules its own.  Where all
        // hold, the plan's pair slots of switch i change their meaning: frame count -1 (`land` reads: no pair entry to take), and
        // in place of the value the record (hi word; ensure_pairs keeps their number below 2^31) and the frame to go on at.
        if constexpr (JUMP && !BUILD) {
            if (planned && p.pstrans != nullptr && p.strans != nullptr) { // (begin_chain: a branch of the first level's start)
                for (int i = 1 + gl; i + 2 < nseg; i += (BLK || ROW) ? 16 : G) {
                    const int s0 = seg_lds[kSegLds + i - 1], sn = seg_lds[kSegLds + i], sm = seg_lds[kSegLds + i + 1];
                    const int t1 = seg_lds[i], t2 = seg_lds[i + 1], t3 = seg_lds[i + 2];
                    const int g1 = t2 - t1, g2 = t3 - t2;
                    const double mm = walk[3 * i + 2];
                    const int m_pair = __double2hiint(mm), m_ref = __double2loint(walk[3 * (i + 1) + 2]);
                    const int q2 = (g2 - 1) / p.pstride;
                    if (t1 >= 1 && sn != s0 && sm != sn && g1 >= 1 && g1 < p.gap_max && g1 < p.sgap && g2 >= 1 && g2 < p.pgap && q2 < p.pnq && g1 + g2 < m_pair &&
                        (m_ref <= 0 || g2 < m_ref + p.tail_margin)) {
                        const int64_t rec = pair_state_record(td->pstrans0, S, T, p.gap_max, p.pnq, e, s0, sn, sm, t1, g1, q2);
                        walk[3 * i + 1] = __hiloint2double((int)rec, t2 + 1 + q2 * p.pstride);
                        walk[3 * i + 2] = __hiloint2double(-1, __double2loint(mm));
                    }
                }
                wave_lds_fence();
            }
        }
        // at a synchronised point in front of frame t (== next_start, or T): take whatever the tables hold
        auto land = [&]() {
            while (planned && t < T) { // t == start of segment seg + 1
                const int i = seg + 1;
                const double v1 = walk[3 * i], v2 = walk[3 * i + 1], mm = walk[3 * i + 2];
                const int m1 = __double2loint(mm), m2 = __double2hiint(mm);
                const int nn = (seg + 2 < nseg) ? seg_start_of(seg + 2) : INT_MAX;
                const int t3 = nn < T ? nn : T;
                if (m1 > 0 && t + m1 <= t3) {
                    extra += v1;
                    ++seg;
                    s = seg_state_of(seg);
                    next_start = nn;
                    t = t3;
                    continue;
                }
                if (m2 <= 0) break;
                const int n4 = (seg + 3 < nseg) ? seg_start_of(seg + 3) : INT_MAX;
                const int t4 = n4 < T ? n4 : T;
                if (t + m2 > t4) break;
                extra += v2;
                seg += 2;
                s = seg_state_of(seg);
                next_start = n4;
                t = t4;
            }
            while (!planned && t < T && use_transients) {
                const int sn = seg_state_of(seg + 1);
                if (sn == s) break; // (uncleaned list) not a switch: run on
                const int nn = (seg + 2 < nseg) ? seg_start_of(seg + 2) : INT_MAX;
                const int t3 = nn < T ? nn : T;
                const TransEntry en = p.trans[td->trans0 + (((int64_t)e * S + s) * S + sn) * T + t];
                const double la = record_of(sn, t - 1)[kRecL], lb = record_of(sn, t3 - 1)[kRecL];
                if (en.m > 0 && t + en.m <= t3) {
                    extra += en.c + (lb - la);
                    ++seg;
                    s = sn;
                    next_start = nn;
                    t = t3;
                    continue;
                }
                // the transient reaches into the next switch: the two together may be in the pair table
                if (p.trans2 == nullptr || nn >= T || nn - t >= p.gap_max || nn <= t) break;
                const int sm = seg_state_of(seg + 2);
                if (sm == sn) break; // (uncleaned list)
                const int n4 = (seg + 3 < nseg) ? seg_start_of(seg + 3) : INT_MAX;
                const int t4 = n4 < T ? n4 : T;
                const TransEntry e2 =
                    p.trans2[(td->trans0 * S + ((((int64_t)e * S + s) * S + sn) * S + sm) * T + t) * p.gap_max + (nn - t)];
                if (e2.m <= 0 || t + e2.m > t4) break; // a chain of three or more: run it
                extra += e2.c + (record_of(sm, t4 - 1)[kRecL] - record_of(sm, t - 1)[kRecL]);
                seg += 2;
                s = sm;
                next_start = n4;
                t = t4;
            }
        };
        clk.stage_b(); // state vectors loaded, lambdas set up
        if (jumping) {
            open_run = 0;
            t = next_start < 1 ? 1 : (next_start < T ? next_start : T); // first switch (>= 1: segment 0 owns frame 0), or T
            if (!building_transients) {
                extra = planned ? (double)walk[0] : record(t - 1)[kRecL];
                land();
            }
            clk.stage_c(); // tables walked
            if (t < T) begin_chain(0);
        } else if (restore) {
            t = next_start < 1 ? 1 : (next_start < T ? next_start : T);
            start_run(t, true, 0);
        } else {
            nrun = -1; // the run starts at frame 1
            fetch(xc, pc); // frame 0
            fetch(xn, pn); // frame 1 (or the first padding row)
            if (ALLVALID || !isnan(pc)) update(xc);
        }
        // ---- table-building launches only: the state and the sums of the open piece go to a record (common.h: the record layout
        // of the prefix table and of the state table)
        auto write_record = [&](double *__restrict__ rec) {
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                if (hasImg[q]) {
#pragma unroll
                    for (int i = 0; i < NP; i += 2)
                        *reinterpret_cast<double2 *>(rec + cidx[q] * NP + i) = make_double2(col.v[q][i], col.v[q][i + 1]);
                }
                if (isM[q]) rec[NC * NP + (cidx[q] - NP)] = accq[q];
            }
            // (the running log-likelihood of the switch-free filter, kRecL and its dense copy, is filled in behind this launch from
            // the sums stored here -- prefix_L_kernel, one thread per record: computed here it was a logarithm and an LDS round
            // trip in every frame of a launch that is two wavefronts per trajectory, a quarter of the builder's 0.94 us per frame)
            if (gl == 0) {
                rec[kRecP] = P;
                rec[kRecE] = (double)E;
                rec[kRecNv] = (double)nv;
            }
        };
        // this launch builds the prefix table: the state after every frame goes to its record (tasks have K1 = 1, s is fixed)
        auto dump = [&](int tt) { write_record(p.prefix_dump + (td->prefix_rec0 + ((int64_t)e * S + s) * T + tt) * REC); };
        // this launch builds the transient table and, beside it, the transient state table (common.h): the state after
        // every frame of the transient goes to its record (tasks have two segments: the switch is at sst[1])
        const bool dump_states = JUMP && !kLean && building_transients && p.strans_dump != nullptr && K1 == 2 && nseg == 2;
        const int t_switch = dump_states ? seg_start_of(1) : 0;
        const int64_t state_rec0 = dump_states ? (td->strans0 + (((int64_t)e * S + seg_state_of(0)) * (S - 1) +
                                                                 (seg_state_of(1) - (seg_state_of(1) > seg_state_of(0) ? 1 : 0))) * T + t_switch) * p.snq
                                               : 0;
        auto dump_state = [&](int g) { write_record(p.strans_dump + (state_rec0 + g) * REC); };
        // this launch builds the pair table and, beside it, the pair state table (common.h): tasks have three segments, the state
        // after every pstride-th frame behind the second switch goes to its record.  Everything is read from the list in LDS at
        // the frame of a record: nothing of it lives across the frame loop (see note_switch)
        auto dump_pair_state = [&](int tt) {
            if constexpr (BUILD && !kLean) {
                if (p.pstrans_dump == nullptr || K1 != 3 || nseg != 3 || !seg_in_lds || tt >= T) return;
                const int t1 = seg_start_of(1), t2 = seg_start_of(2), g1 = t2 - t1, g2 = tt - t2;
                if (g2 < 1 || g2 >= p.pgap || (g2 - 1) % p.pstride != 0) return;
                const int q2 = (g2 - 1) / p.pstride;
                const int s0 = seg_state_of(0), sn = seg_state_of(1), sm = seg_state_of(2);
                if (g1 < 1 || g1 >= p.gap_max || q2 >= p.pnq || sn == s0 || sm == sn) return;
                write_record(p.pstrans_dump + pair_state_record(td->pstrans0, S, T, p.gap_max, p.pnq, e, s0, sn, sm, t1, g1, q2) * REC);
            }
        };
        if constexpr (DUMP) dump(0);
        // A comparison with the table is due at frame t (the state after frame t - 1 against the table's record): either the
        // next look is scheduled, or the own piece ends here and the task goes on at its next synchronised point.
        // Returns true when the task is finished with its frames (a table-building launch whose transient has converged).
        auto compare_with_table = [&]() -> bool {
            clk.event_begins(TaskClock::kLook);
            const double *__restrict__ rec = record(t - 1);
            // per lane: largest deviation of the own column(s) from the table's, in units of the tolerance
            double excess = 0.0;
            bool same = true;
            // first-order tail (tail.hip): the covariance columns must have converged as before; a mean column may still be
            // kTailTol = 2^-20 away -- what that deviation does to every later frame is a dot product with the table's g
            const double kTailTol = p.tail_tol;  // (2^-20 unless BILD_TAIL_TOL_BITS says otherwise: tools/tail_tolerance.py)
            const int kTailMargin = p.tail_margin; // frames beyond the table's own transient before the next switch may come (8)
            const bool tails = JUMP && p.tail_g != nullptr && !building_transients;
            bool near = true;
            // (the listed frame loop: every load of the look in flight, then ONE wait, as in `sandwich` -- the compiler's own order
            // is load, wait, compare, five times over, for the 80 bytes of one column.  With them the two running sums a look that
            // converges adds afterwards: the frame it goes on at is known before the comparison.)
            constexpr bool kBatchLook = kLean && CPL == 1;
            double look[kBatchLook ? NP : 1], look_L = 0.0, look_L2 = 0.0;
            if constexpr (kBatchLook) {
                if (hasImg[0]) {
                    if constexpr (PAIR) {
#pragma unroll
                        for (int k = 0; k < NP / 2; ++k) look[k] = rec[cidx[0] * NP + 2 * k + odd];
                    } else {
#pragma unroll
                        for (int i = 0; i < NP; i += 2) {
                            const double2 r2 = *reinterpret_cast<const double2 *>(rec + cidx[0] * NP + i);
                            look[i] = r2.x;
                            look[i + 1] = r2.y;
                        }
                    }
                }
                if (!building_transients) {
                    look_L = rec[kRecL];
                    look_L2 = record((next_start < T ? next_start : T) - 1)[kRecL];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                if (!hasImg[q]) continue;
                // (mean columns: the floor is the scale of the DATA as far as the model can explain it -- for data drawn
                // from the model the largest coordinate itself, 4-5 standard deviations of the innovation; for data the model
                // did not produce (an offset, outliers) the innovations e grow with the data, the log-likelihood error of a
                // deviation d is ~ 20 |e| d / S, and the floor must not grow with them: TrajDesc::mscale)
                double dev = 0.0, ref = isM[q] ? td->mscale[e] : 0.0;
                if constexpr (PAIR) {
                    // each row over its entries, then the larger of the two: a maximum (fmax: of the operands that are numbers)
                    // does not depend on the order it is taken in, so both rows hold what the whole column gives
                    double devh = 0.0, refh = ref;
#pragma unroll
                    for (int k = 0; k < NP / 2; ++k) {
                        double rk;
                        if constexpr (kBatchLook) rk = look[k];
                        else rk = rec[cidx[q] * NP + 2 * k + odd];
                        devh = fmax(devh, fabs(colh[k] - rk));
                        refh = fmax(refh, fabs(rk));
                    }
                    double d0, d1, r0, r1;
                    pair_swap(devh, d0, d1);
                    pair_swap(refh, r0, r1);
                    dev = fmax(d0, d1);
                    ref = fmax(r0, r1);
                } else {
#pragma unroll
                    for (int i = 0; i < NP; i += 2) {
                        double2 r2;
                        if constexpr (kBatchLook) r2 = make_double2(look[i], look[i + 1]);
                        else r2 = *reinterpret_cast<const double2 *>(rec + cidx[q] * NP + i);
                        dev = fmax(dev, fmax(fabs(col.v[q][i] - r2.x), fabs(col.v[q][i + 1] - r2.y)));
                        ref = fmax(ref, fmax(fabs(r2.x), fabs(r2.y)));
                    }
                }
                const double bar = kJumpTol * ref;
                same = same && (dev <= bar); // a NaN anywhere never compares equal
                excess = fmax(excess, dev > bar ? dev / fmax(bar, 1e-300) : 0.0);
                const double bar_t = isM[q] ? kTailTol * ref : bar;
                near = near && (dev <= bar_t);
            }
            const unsigned long long agree = __ballot(same);
            bool converged = (agree & group_mask) == group_mask;
            double tail_term = 0.0;
            if (tails && !converged) {
                // (The comparisons stay where the table BUILDERS made theirs -- the next look is scheduled by the full criterion,
                // tails or not: a transient must never be found converged at a frame its builder did not look at, or a chain
                // that starts from the state table -- which skips the frames in front of its second switch, comparisons
                // included -- and the same chain run from its first switch would part ways by a tolerance.)
                if ((__ballot(near) & group_mask) == group_mask) {
                    // may the rest of the segment come out of the table?  Only if the means will have converged by the next
                    // switch: the table knows how long a transient from a synchronised start takes at this very place (the
                    // entry of the switch this segment began with), a chain's last transient gets kTailMargin frames more
                    const int t2 = next_start < T ? next_start : T;
                    bool far = t2 >= T;
                    wave_lds_fence();
                    const double noted = row_const[1];
                    const int t_seg = __double2loint(noted), s_from = __double2hiint(noted) & kNoteState;
                    // (the vectors of the dot product: the table's own tail, or -- below -- the tail through the next switch)
                    const double *__restrict__ g_at = p.tail_g + (td->prefix_rec0 + ((int64_t)e * S + s) * T + (t - 1)) * (kDMax * NP);
                    if (!far && p.trans != nullptr && t_seg >= 1) {
                        const int m_ref = p.trans[td->trans0 + (((int64_t)e * S + s_from) * S + s) * T + t_seg].m;
                        // ... and by what the means still have to lose: `excess` is their deviation in units of the full
                        // tolerance; a transient from a synchronised start lost ~30 bits (a deviation of 2^-13 of the scale
                        // down to 2^-43) in m_ref frames, so `bits` more take bits * m_ref / 30 frames -- a chain's last
                        // transient starts further off than a single switch's and is asked for more (soak: 3-state chains)
                        int bits = 40;
                        if (!(__ballot(excess >= 0x1p36) & group_mask)) bits = 36;
                        if (!(__ballot(excess >= 0x1p32) & group_mask)) bits = 32;
                        if (!(__ballot(excess >= 0x1p28) & group_mask)) bits = 28;
                        if (!(__ballot(excess >= 0x1p24) & group_mask)) bits = 24;
                        if (!(__ballot(excess >= 0x1p20) & group_mask)) bits = 20;
                        if (!(__ballot(excess >= 0x1p16) & group_mask)) bits = 16;
                        if (!(__ballot(excess >= 0x1p12) & group_mask)) bits = 12;
                        if (!(__ballot(excess >= 0x1p8) & group_mask)) bits = 8;
                        far = m_ref > 0 && t2 - t_seg >= m_ref + kTailMargin && t2 - t >= (bits * m_ref + 29) / 30 + 4;
                        // The switch tail (tail.hip).  The next switch is too close for the table's own tail -- whose vector is the
                        // adjoint of the switch-free filter --, but the adjoint along the path this candidate has in front of it
                        // (state s up to t2 - 1, the switch, the transient from a synchronised start, the new state's filter) is
                        // in a table too, and `land` at t2 does the zeroth order.  Taken where
                        //  (a) the table has the entry: t2 - t < J;  (b) the switch at t2 has a transient entry m1 (the lo word of
                        //  its third plan slot, which the pair-state rewrite leaves intact);  (c) the switch behind t2 leaves that
                        //  transient the room this look would ask of its own, so that `land` takes exactly that entry;
                        //  (d) the look lies behind the chain's THIRD switch: a chain started from a state table skips the looks of
                        //  its first and second gap, and the same chain run from its first switch must not end at one of them.
                        if constexpr (!BUILD) {
                            if (!far && m_ref > 0 && p.stail != nullptr && seg_in_lds && seg + 1 < nseg && t2 - t < p.stail_J &&
                                seg - (__double2hiint(noted) >> 16) >= 2) {
                                const int sn = seg_state_of(seg + 1);
                                const int m1 = planned ? __double2loint(walk[3 * (seg + 1) + 2])
                                                       : p.trans[td->trans0 + (((int64_t)e * S + s) * S + sn) * T + t2].m;
                                const int n3 = (seg + 2 < nseg) ? seg_start_of(seg + 2) : INT_MAX;
                                const int room = (n3 < T ? n3 : T) - t2;
                                // (t2 + m1 < T: an entry of T - t2 frames is a transient that ran into the trajectory's end without
                                // converging -- the table holds no vectors for it; only BILD_TAIL_MARGIN=0 lets one come this far)
                                if (sn != s && m1 > 0 && m1 <= kSwitchTailMaxM && t2 + m1 < T && room >= m1 + kTailMargin &&
                                    room >= (bits * m1 + 29) / 30 + 4) {
                                    far = true;
                                    const int64_t entry = td->strans0 + (((int64_t)e * S + s) * (S - 1) + (sn - (sn > s ? 1 : 0))) * T + t2;
                                    g_at = p.stail + (entry * p.stail_J + (t2 - t)) * (kDMax * NP);
                                }
                            }
                        }
                    }
                    if (far) {
                        converged = true;
                        // (PAIR: the one place of a look that needs whole columns -- g . (M - M_table) is a chain of NP FMAs
                        // per lane whose order is part of the result; a chain takes at most one tail)
                        if constexpr (PAIR) unpack();
                        double mine[CPL];
#pragma unroll
                        for (int q = 0; q < CPL; ++q) {
                            mine[q] = 0.0;
                            if (isM[q]) {
                                const double *__restrict__ gq = g_at + (cidx[q] - NP) * NP;
                                double acc = 0.0;
#pragma unroll
                                for (int i = 0; i < NP; ++i) acc = fma(gq[i], col.v[q][i] - rec[cidx[q] * NP + i], acc);
                                mine[q] = acc;
                            }
                        }
                        tail_term = mean_sum(mine);
                    }
                }
            }
            if (!converged) {
                // not yet: the deviation shrinks geometrically (the default Rouse model: 0.73 bits per frame), so the
                // next look comes after about the frames the worst column still needs at 1.3 frames per bit -- by the
                // lower edge of its bucket, i.e. rather too early than too late; a slower filter is simply asked again
                int wait = 4;
                if (__ballot(excess >= 0x1p4) & group_mask) wait = 8;
                if (__ballot(excess >= 0x1p8) & group_mask) wait = 12;
                if (__ballot(excess >= 0x1p16) & group_mask) wait = 24;
                if (__ballot(excess >= 0x1p24) & group_mask) wait = 32;
                if (__ballot(excess >= 0x1p32) & group_mask) wait = 44;
                if (__ballot(!(excess < 0x1p60)) & group_mask) wait = 64; // far off, or not a number
                t_check = t + wait;
            } else {
                // converged at frame t: the own piece ends here (with what the remaining deviation of the means still adds)
                extra += piece_value();
                extra += tail_term;
                open_run = 0;
                nrun += t;
                if (building_transients) return true;
                // (the lean loop has asked for frame t + 1 already, the other one has not)
                const int t_ptr = kLean ? t + 2 : t + 1;
                const int t2 = next_start < T ? next_start : T;
                if constexpr (kBatchLook) extra += look_L2 - look_L;
                else extra += record(t2 - 1)[kRecL] - rec[kRecL];
                t = t2;
                land();
                if (t < T) {
                    begin_chain(t_ptr); // leaves frame t in xn
                    if constexpr (kLean) {
#pragma unroll
                        for (int q = 0; q < CPL; ++q) xc[q] = xn[q];
                        pc = pn;
                        fetch(xn, pn);
                    }
                }
            }
            clk.event_ends(TaskClock::kLook);
            return false;
        };
        if constexpr (kLean) {
            // The frame loop of the launch over the work lists.  A lone wave -- the chains that end a launch -- pays for every
            // instruction around the frame: ONE test per frame for everything that is not a frame (`t_event`: the next frame at
            // which a segment begins or a comparison is due), no tests of the table builders, no loop-carried flag in the scalar
            // masks: 53 -> 48 us for the 10k x k = 4 launch, 97 -> 85 us at k = 8.  (The same structure costs the geometries that
            // are short of registers more spills than it saves instructions -- (16, 1, 19) went from two reloads per frame to
            // seven, 3x slower --, so they keep the loop below.)
            auto next_event = [&]() {
                const int tc = (jumping && t_check > t) ? t_check : INT_MAX;
                return next_start < tc ? next_start : tc;
            };
            int t_event = next_event();
            while (t < T) {
                // invariant: xn holds frame t, the pointers stand at frame t + 1.  The next frame's data are asked for FIRST, in
                // front of the branch: in one basic block with the frame the scheduler sinks the load behind the last use of the
                // current frame's data (same register), and the delivery below then waits for L2 in every frame
#pragma unroll
                for (int q = 0; q < CPL; ++q) xc[q] = xn[q];
                pc = pn;
                fetch(xn, pn);
                if (t >= t_event) { // (PAIR: the events work on the halves, each row on its own)
                    if (jumping && t == t_check) {
                        (void)compare_with_table();
                        if (t >= T) break;
                    }
                    if (t >= next_start) enter_segment(t);
                    t_event = next_event();
                }
                frame(xc, pc);
                ++t;
                // The next frame's data were asked for at the top of this one: take delivery HERE, a whole frame later, and
                // not where the register allocator happens to copy them (mid-frame: a wave with the SIMD to itself -- the
                // long chains that end a launch -- then waited for L2 in every frame: 0.45 us per frame instead of 0.24)
#pragma unroll
                for (int q = 0; q < CPL; ++q) asm volatile("" : "+v"(xn[q]));
            }
        } else {
            while (t < T) {
                // invariant: xn holds frame t, the pointers stand at frame t + 1
#pragma unroll
                for (int q = 0; q < CPL; ++q) xc[q] = xn[q];
                pc = pn;
                fetch(xn, pn);
                if (ROW) s2_now = row_const[0];
                if (t >= next_start) enter_segment(t);
                frame(xc, pc);
                if constexpr (DUMP) dump(t);
                ++t;
                if constexpr (JUMP) {
#pragma unroll
                    for (int q = 0; q < CPL; ++q) asm volatile("" : "+v"(xn[q])); // (delivery of the next frame's data: see above)
                }
                if constexpr (JUMP) {
                    if (dump_states && t < T && t - t_switch < p.sgap && (t - t_switch - 1) % p.sstride == 0)
                        dump_state((t - t_switch - 1) / p.sstride);
                    dump_pair_state(t);
                }
                if (JUMP && jumping && t == t_check && t < T) {
                    if (compare_with_table()) break;
                }
            }
        }
        if (open_run != 0) {
            extra += piece_value(); // a run that reached the end of the trajectory (all of it, without tables)
            nrun += t;
        }
        if (building_transients) {
            // what this transient adds beyond the running sums of the new state's own filter over the same frames, and how
            // many frames it took (frames < t are processed; it started at the switch, frame t0)
            // (the descriptor as given: a second switch behind the trajectory's end has been cleaned away, its entry is void)
            const int t0 = sst[1], s_old = ssv[0], tb = t < T ? t : T;
            const bool all_switched = nseg == K1 && seg == nseg - 1; // converged (or ended) behind the LAST switch
            const double c = extra - (record_of(s, tb - 1)[kRecL] - record_of(s, t0 - 1)[kRecL]);
            if (gl == 0) {
                TransEntry en;
                en.c = all_switched ? c : 0.0;
                en.m = all_switched ? tb - t0 : 0;
                en.pad = 0;
                if (p.trans2_dump)
                    p.trans2_dump[(td->trans0 * S + ((((int64_t)e * S + s_old) * S + ssv[1]) * S + ssv[2]) * T + t0) * p.gap_max +
                                  (sst[2] - t0)] = en;
                else
                    p.trans_dump[td->trans0 + (((int64_t)e * S + s_old) * S + ssv[1]) * T + t0] = en;
                p.out[otask] = 0.0;
            }
        } else if (lead) {
            p.out[otask] = extra;
        }
        // bench accounting: one of kFrameCounters words per workgroup slot (a single word would serialise ten thousand
        // atomics that all arrive at the end of a short launch)
        if (p.frames_run && lead) atomicAdd(p.frames_run + (blockIdx.x % kFrameCounters), (unsigned long long)nrun);
        if (p.frames_task && lead) p.frames_task[otask] = clk.word(nrun);
        wave_lds_fence();
    }
}

} // namespace
} // namespace bild
