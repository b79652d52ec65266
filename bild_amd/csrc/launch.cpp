// Launches: one batch of candidates on a stream (launch_batch: the table walk, the frame loop, the reduction of partial
// results), the launch order of the host and the device scheduler, and the kernel timing of bench.py.
#include <climits>
#include <queue>
#include <utility>

#include "chain_work.h"
#include "likelihood.h"

namespace {

// kernel timing (bench.py roofline leg)
std::atomic<int32_t *> g_frames_task{nullptr}; // diagnostics: bild_debug_frames_per_task
std::mutex g_time_mu;
int g_time_on = 0; // 0: off; p >= 1: every p-th launch is bracketed by events (sampling keeps the events out of most steps)
uint64_t g_time_count = 0;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_time_events;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_walk_events; // the table walk in front of a split launch (walk.hip)
std::string g_time_name;

// the milliseconds between the events of `list` (g_time_events or g_walk_events), summed; the list is emptied
int drain(std::vector<std::pair<hipEvent_t, hipEvent_t>> &list, double *total_ms, int64_t *launches, std::string *name = nullptr)
{
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    {
        std::lock_guard<std::mutex> lk(g_time_mu);
        ev.swap(list);
        if (name) *name = g_time_name;
    }
    double tot = 0.0;
    for (auto &pr : ev) {
        HIP_TRY(hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        tot += ms;
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    *total_ms = tot;
    *launches = (int64_t)ev.size();
    return BILD_OK;
}

constexpr size_t kWorkHeader = 128; // two sets of work-list counters
static_assert(kWorkHeader >= 2 * kWorkBuckets * sizeof(int32_t), "header holds the counters");

} // namespace

namespace bild {

int launch_batch(const bild_model &m, const bild_trajset &ts, int64_t n, int K1, const int32_t *d_seg_start,
                 const int32_t *d_seg_state, const int32_t *d_traj_id, const int32_t *d_order, unsigned flags,
                 hipStream_t st, double *d_out, const LaunchIn &in)
{
    int mode;
    int rc = pick_mode(m, flags, &mode);
    if (rc) return rc;
    const LaunchIn::Fill building = in.fill;
    const bool st_in = in.d_ss != nullptr;
    if (st_in && K1 > kSplitMaxK1) return fail(BILD_ERR_INVALID, "internal: (s, theta) input with %d segments", K1);
    // which kernel family serves this model and path:
    //   kWide       41-128 modes, LDS-resident state (wide.hip)                      modal path only
    //   kModalTiles 33-40 modes, modal recursion on tile registers (modal_mfma.hip)  modal path only
    //   kDenseTiles dense recursion on the matrix pipe (dense_mfma.hip): symmetric models of up to 24 modes
    //               (BILD_DENSE_VALU=1: the LDS-fed vector formulation instead)
    //   kVector     the register-resident vector kernels of kernels.hip, geometry chosen per batch
    enum Family { kVector, kDenseTiles, kModalTiles, kWide };
    Family fam = kVector;
    if (m.wide || m.mid) {
        if (mode != kModal)
            return fail(BILD_ERR_UNSUPPORTED, "chains of more than %d effective modes (here %d) run on the modal path only%s%s", kMaxNP,
                        m.n, m.modal_ok ? "" : ", which is unavailable: ", m.modal_ok ? "" : m.modal_why.c_str());
        fam = m.wide ? kWide : kModalTiles;
    } else if (mode == kDense && m.symmetric && dense_mfma_supported(m.NPm[kDense]) && !config().dense_valu) {
        fam = kDenseTiles;
    }
    const int64_t ntasks = n * ts.dstar_max;
    // A split launch (below) sends only its chains of close switches through the frame loop -- a few per cent of a batch
    // with few switches per candidate, a third at k = 8 -- and deals them out itself, heaviest first.  What it needs
    // beyond this: the transient table, and room for the walk plan.
    const bool splittable = fam == kVector && mode == kModal && K1 <= kSplitMaxK1 && !building && !config().no_split &&
                            !(flags & BILD_NO_SPLIT) && ntasks <= (int64_t)INT_MAX;
    // room for the walk plan (the table entries of all switches of a task, fetched at once) where it does not cost occupancy
    // (a CU holds OCC waves per SIMD = 4 OCC / W workgroups of a geometry, and 160 KiB of LDS for them)
    auto walk_bytes = [](const Geometry &g) { return LdsLayout(g.NP, g.W * (64 / g.G), 0, 0).walk_bytes(); };
    auto walk_fits = [&](const Geometry &g, size_t lds) {
        return K1 <= kSegLds && !config().no_walk_plan &&
               lds + walk_bytes(g) <= (size_t)160 * 1024 / (size_t)std::max(1, (4 * g.OCC + g.W - 1) / g.W);
    };
    Geometry geom{};
    size_t lds = 0;
    if (fam == kVector) {
        // (the tables are there already, so the launch will split: a launch that takes the geometry of the listed frame loop
        // and then runs the WHOLE batch with it would run at one or two waves per SIMD)
        const bool may_split = splittable && !(flags & (BILD_NO_JUMP | BILD_NO_PREFIX)) && ts.trans_state == 1 && !config().no_walk_plan;
        // (the first geometry of the chain length: fewest tasks per wave, and the one whose LDS leaves room for the walk plan)
        const int64_t tasks_for_geometry = may_split ? 1 : ntasks;
        // (the frame loop over the work lists is latency-bound: the row layout -- three mean slots, the shortest frame for a lone
        // wave -- also where fewer mean vectors would allow more tasks per wave; all geometries of a chain length agree bit for bit)
        const int means_for_geometry = may_split ? std::max(ts.means_max, (int)kDMax) : ts.means_max;
        // (a launch that builds a table takes the automatic geometry whatever BILD_GEOM says, a launch that may jump never the
        // block layout: see geometry_for; a forced geometry is held to the mean vectors the set needs, not to the three slots a
        // split launch prefers)
        const bool forced = !building && config().geom >= 0;
        const bool jumps = mode == kModal && K1 > 0 && !(flags & (BILD_NO_PREFIX | BILD_NO_JUMP)) && !config().no_prefix && !config().no_jump;
        if (!(forced && geometry_for(m.NPm[mode], mode, tasks_for_geometry, ts.means_max, &geom, true, jumps) && geom.id == config().geom) &&
            !geometry_for(m.NPm[mode], mode, tasks_for_geometry, means_for_geometry, &geom, !building, jumps) &&
            !geometry_for(m.NPm[mode], mode, tasks_for_geometry, ts.means_max, &geom, !building, jumps))
            return fail(BILD_ERR_UNSUPPORTED, "no kernel for %d rows", m.NPm[mode]);
        Geometry lg{};
        // (... including the room for the walk plan in the workgroup's share of the LDS)
        if (may_split && listed_geometry(geom, &lg) && walk_fits(lg, lds_bytes(m, lg, mode))) {
            // (Rounds 2-3 took a geometry at ONE wave per SIMD only while the estimated list fitted the chip once.  Since the lean
            // frame loop -- no spills at 16 / 20 modes, against 270 / 600 spilled registers of the batch geometries -- it wins at
            // every list length measured: chains of 32 / 40 beads, 10 000 ... 100 000 candidates, k = 4 / 8: 1.3-2.0x / 2.5x;
            // BASELINE configs[3] at k = 8: 335 -> 196 us.  tools/listed_rule.py, BILD_NO_LISTED_GEOMETRY for the comparison.)
            geom = lg;
        }
        lds = lds_bytes(m, geom, mode);
        if (lds > 160 * 1024)
            return fail(BILD_ERR_UNSUPPORTED, "model tables need %zu bytes of LDS (> 160 KiB): too many states (%d) for chain length %d", lds, m.S, m.n);
    }

    bool timing; // this launch is bracketed by events (bild_kernel_timing: every p-th one) and counts the frames it runs
    {
        std::lock_guard<std::mutex> lk(g_time_mu);
        timing = g_time_on > 0 && !building && (g_time_count++ % (uint64_t)g_time_on) == 0;
    }
    KParams p{};
    fill_params(m, ts, mode, p);
    p.ntasks = ntasks;
    p.K1 = K1;
    p.seg_start = d_seg_start;
    p.seg_state = d_seg_state;
    p.traj_id = d_traj_id;
    if (fam == kVector) {
        p.order = d_order;
        p.no_jump = (flags & BILD_NO_JUMP) || config().no_jump ? 1 : 0;
        if (mode == kModal && K1 > 0 && !(flags & BILD_NO_PREFIX)) {
            // the tables of the set are built at its first evaluation: results never depend on what was evaluated before (a
            // call that runs frame by frame and a later one that uses the tables would differ by ~1e-12)
            if (ts.prefix_state == 0) ensure_prefix(m, ts, st);
            if (ts.prefix_state == 1) p.prefix = ts.d_prefix;
            if (ts.prefix_state == 1 && !building && !(flags & BILD_NO_TAIL)) p.tail_g = ts.d_tail_g;
            p.tail_tol = std::ldexp(1.0, -std::max(8, std::min(config().tail_tol_bits, 43)));
            p.tail_margin = std::max(0, config().tail_margin);
            const bool read_states = !config().no_states && !(flags & BILD_NO_STATES);
            bool states = false; // the launch fills or reads the transient state table
            bool pair_states = false; // ... the pair state table (BILD_NO_STATES and the flag switch both levels off)
            if (building == LaunchIn::kFillTransients) {
                p.trans_dump = ts.d_trans;
                p.strans_dump = ts.d_strans;
                states = true;
            } else if (building == LaunchIn::kFillPairs) {
                p.trans2_dump = ts.d_trans2;
                p.gap_max = ts.gap_max;
                if (read_states) p.strans = ts.d_strans;
                states = read_states;
                p.pstrans_dump = ts.d_pstrans;
                pair_states = ts.d_pstrans != nullptr;
            } else if (p.prefix && !p.no_jump) {
                // (the state table as it was when the launch began: one that ensure_transients builds below is read from the next on)
                states = read_states && ts.trans_state == 1;
                if (states) p.strans = ts.d_strans;
                pair_states = read_states && ts.trans2_state == 1;
                if (ts.trans_state == 0) ensure_transients(m, ts, st);
                if (ts.trans_state == 1) {
                    p.trans = ts.d_trans;
                    p.m_typ = ts.trans_m_typ;
                    if (ts.trans2_state == 0) ensure_pairs(m, ts, st);
                    if (ts.stail_state == 0) ensure_switch_tails(m, ts, st);
                    if (ts.stail_state == 1 && p.tail_g != nullptr && !(flags & BILD_NO_SWITCH_TAIL)) {
                        p.stail = ts.d_stail;
                        p.stail_J = ts.stail_J;
                    }
                    if (ts.trans2_state == 1) {
                        p.trans2 = ts.d_trans2;
                        p.gap_max = ts.gap_max;
                    }
                    // (as above: the table as it was when the launch began)
                    if (pair_states && p.trans2 && !config().no_pair_states) p.pstrans = ts.d_pstrans;
                    pair_states = p.pstrans != nullptr;
                    if (walk_fits(geom, lds)) {
                        p.walk_lds = 1;
                        lds += walk_bytes(geom);
                    }
                }
            }
            if (states) {
                p.sgap = ts.sgap;
                p.sstride = ts.sstride;
                p.snq = ts.snq;
            }
            if (pair_states) {
                p.pgap = ts.pgap;
                p.pstride = ts.pstride;
                p.pnq = ts.pnq;
            }
        }
        if (timing) p.frames_run = m.d_frames;
        p.frames_task = g_frames_task.load();
    }

    // ---- the table walk in front of the frame loop (walk.hip) -----------------------------------------------------
    // With all tables in place a task is a handful of lookups unless it holds a chain of three or more close switches:
    // one lane per task walks the tables and writes the result, or hands the task on through the work lists; the frame
    // loop then runs the listed tasks only.  Same numbers added in the same order: bit-identical to the single launch
    // (BILD_NO_SPLIT=1).  Also the place where (s, theta) input becomes segment lists.
    const bool split = splittable && p.walk_lds;
    const bool walk = split || st_in;
    // lists of <= 3 segments hold at most two switches: on a set whose tables cover every such candidate the walk finishes
    // the whole batch, and the frame loop -- which would find its lists empty -- is not launched
    const bool frame_loop = !(split && K1 <= 3 && ts.two_switch_covered && p.trans2 != nullptr && !config().no_fused_launch);
    // ... and where the listed frame loop runs on geometry 23 and the batch is small, walk and frame loop share ONE launch
    // (kernels.hip: logl_one_kernel): each workgroup walks a slice of at most kOneSlice tasks and runs what it listed itself,
    // handed over in LDS -- no work lists, no second dispatch, no prologue that repeats the walk.  Bit-identical to the two
    // kernels (BILD_NO_ONE_LAUNCH) and to BILD_NO_SPLIT.  The bound: DESIGN.md section 4 (profiles/r05_one_launch_ab.txt).
    const int64_t one_grid = std::min<int64_t>(ntasks, 256 * (int64_t)std::max(geom.OCC, 1));
    const bool one = split && frame_loop && fam == kVector && geom.id == 23 && geom.lay == 3 && K1 <= kOneLaunchMaxK1 && ntasks >= 1 &&
                     ntasks <= kOneLaunchMaxTasks && (ntasks + one_grid - 1) / one_grid <= kOneSlice && !config().no_one_launch &&
                     lds + LdsLayout::hand_bytes() <= (size_t)160 * 1024 / (size_t)std::max(1, (4 * geom.OCC + geom.W - 1) / geom.W);

    // What this call allocates and creates for itself, released by whatever path it returns: the frees are stream-ordered
    // behind everything the call enqueued, the events are destroyed unless they were handed to the timing lists.
    struct Own {
        hipStream_t st;
        double *partials = nullptr;
        int32_t *work = nullptr, *lists = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr, w0 = nullptr, w1 = nullptr;
        ~Own()
        {
            for (void *b : {(void *)partials, (void *)work, (void *)lists})
                if (b) (void)hipFreeAsync(b, st);
            for (hipEvent_t e : {e0, e1, w0, w1})
                if (e) (void)hipEventDestroy(e);
        }
    } own{st};
    if (timing) {
        HIP_TRY(hipEventCreate(&own.e0));
        HIP_TRY(hipEventCreate(&own.e1));
        if (walk && !one) { // (the one launch carries the frame loop's events only: the walk has no dispatch of its own)
            HIP_TRY(hipEventCreate(&own.w0));
            HIP_TRY(hipEventCreate(&own.w1));
        }
    }
    // d* > 1: one partial result per (sample, covariance chain), summed by a second kernel.  The buffer belongs to
    // THIS call (stream-ordered allocation, released behind the reduction): launches of one model on different
    // streams, or a host-buffer call beside a device-buffer call, share nothing.
    double *target = d_out;
    if (ts.dstar_max > 1) {
        HIP_TRY(hipMallocAsync((void **)&own.partials, (size_t)p.ntasks * sizeof(double), st));
        target = own.partials;
    }
    p.out = target;

    std::unique_lock<std::mutex> slot_order; // (WorkSlot::launch_mu: released when this function returns, by whatever path)
    if (st_in && (!d_seg_start || !d_seg_state)) {
        // (s, theta) rows resident in HBM and no room given for the lists the frame loop reads: the model's block on the
        // stream that owns it, else an allocation of this call
        const size_t bytes = 2 * (size_t)n * K1 * sizeof(int32_t);
        int32_t *lists = nullptr;
        {
            std::lock_guard<std::mutex> lk(m.mu);
            bild_model::WorkSlot *slot = m.slot_for(st);
            if (slot && slot->ws_lists.reserve(bytes) == BILD_OK) lists = (int32_t *)slot->ws_lists.ptr;
        }
        if (!lists) {
            if (hipMallocAsync((void **)&own.lists, bytes, st) != hipSuccess) return fail(BILD_ERR_NOMEM, "segment lists: out of device memory");
            lists = own.lists;
        }
        d_seg_start = lists;
        d_seg_state = lists + (size_t)n * K1;
        p.seg_start = d_seg_start;
        p.seg_state = d_seg_state;
    }
    WalkParams w{};
    if (walk) {
        w.trajs = ts.d_descs;
        w.S = m.S;
        w.dstar_max = ts.dstar_max;
        w.K1 = K1;
        w.n = n;
        w.traj_id = d_traj_id;
        if (st_in) {
            w.ss = in.d_ss;
            w.thetas = in.d_thetas;
            w.seg_out_start = const_cast<int32_t *>(d_seg_start);
            w.seg_out_state = const_cast<int32_t *>(d_seg_state);
            w.status = in.status;
        } else {
            w.seg_start = d_seg_start;
            w.seg_state = d_seg_state;
        }
        w.convert_all = split ? 0 : 1;
        w.no_lists = frame_loop ? 0 : 1;
        if (one) {
            // (no work lists: the counter sets of the persistent block stay as they are -- the walk of the next split launch zeroes
            // the set after the one it takes, and a flip here would hand that launch a set nobody zeroed)
            w.Lc = ts.d_prefix_L;
            w.trans = p.trans;
            w.trans2 = p.trans2;
            w.gap_max = p.gap_max;
            w.m_typ = p.m_typ;
            w.out = target;
            w.frames_task = p.frames_task;
            if (config().walk_debug) w.debug = config().walk_debug;
            p.order = nullptr;
        }
        bild_model::WorkSlot *flipped = nullptr; // the persistent work-list block this launch alternates the counter set of
        if (split && !one) {
            int32_t *d_work = nullptr, *d_lists = nullptr;
            const size_t list_bytes = (size_t)kWorkBuckets * (size_t)p.ntasks * sizeof(int32_t);
            {
                bild_model::WorkSlot *slot;
                {
                    std::lock_guard<std::mutex> lk(m.mu);
                    slot = m.slot_for(st);
                }
                if (slot) slot_order = std::unique_lock<std::mutex>(slot->launch_mu); // (never taken under m.mu: no lock order to get wrong)
                std::lock_guard<std::mutex> lk(m.mu);
                if (slot) {
                    DeviceBuf &ws_work = slot->ws_work;
                    if (ws_work.cap < kWorkHeader + list_bytes) {
                        // (hipFree inside waits for the device: nothing still reads the old block)
                        // (the memset on the launch's own stream: a plain hipMemset is not ordered against a non-blocking stream)
                        if (ws_work.reserve(kWorkHeader + list_bytes) != BILD_OK || hipMemsetAsync(ws_work.ptr, 0, kWorkHeader, st) != hipSuccess)
                            return fail(BILD_ERR_NOMEM, "work lists: allocation of %zu bytes failed", kWorkHeader + list_bytes);
                    }
                    d_work = (int32_t *)ws_work.ptr + kWorkBuckets * slot->work_set;
                    w.work_counts_next = (int32_t *)ws_work.ptr + kWorkBuckets * (1 - slot->work_set);
                    slot->work_set = 1 - slot->work_set;
                    flipped = slot;
                    d_lists = (int32_t *)((char *)ws_work.ptr + kWorkHeader);
                }
            }
            if (!d_work) {
                hipError_t he = hipMallocAsync((void **)&own.work, kWorkHeader + list_bytes, st);
                if (he == hipSuccess) he = hipMemsetAsync(own.work, 0, kWorkHeader, st);
                if (he != hipSuccess) return fail(BILD_ERR_NOMEM, "work lists: %s", hipGetErrorString(he));
                d_work = own.work;
                d_lists = (int32_t *)((char *)own.work + kWorkHeader);
            }
            w.Lc = ts.d_prefix_L;
            w.trans = p.trans;
            w.trans2 = p.trans2;
            w.gap_max = p.gap_max;
            w.m_typ = p.m_typ;
            w.out = target;
            w.work_counts = d_work;
            w.work = d_lists;
            w.work_cap = p.ntasks;
            w.frames_task = p.frames_task;
            p.work_counts = w.work_counts;
            p.work = w.work;
            p.work_cap = w.work_cap;
            p.order = nullptr; // the work lists ARE the launch order
        }
        const int wrc = one ? 0 : launch_walk(w, (void *)st, (void *)own.w0, (void *)own.w1); // (timed: the events ride on the dispatch)
        if (wrc != 0) {
            if (flipped) { // the walk never ran: the other counter set was not zeroed -- the next launch must not take it
                std::lock_guard<std::mutex> lk(m.mu);
                flipped->work_set = 1 - flipped->work_set;
            }
            return fail(BILD_ERR_HIP, "walk kernel launch failed: %s", hipGetErrorString((hipError_t)wrc));
        }
        if (timing && !one) {
            std::lock_guard<std::mutex> lk(g_time_mu);
            g_walk_events.emplace_back(own.w0, own.w1);
            own.w0 = own.w1 = nullptr;
        }
    }

    // tasks per workgroup (the tile kernels size their own grid: 4 waves x 4 tasks)
    const int64_t tasks_per_block = fam == kWide ? 1 : fam != kVector ? 16 : (int64_t)geom.W * geom.tasks_per_wave();
    int64_t blocks = (p.ntasks + tasks_per_block - 1) / tasks_per_block;
    // (work lists: one residency of the chip at most -- most of the tasks never reach the frame loop)
    const int64_t max_blocks = split ? 256 * std::max(geom.OCC, 1) : 256 * 16;
    const int grid = one ? (int)one_grid : (int)std::min<int64_t>(std::max<int64_t>(blocks, 1), max_blocks);
    // timed launches of the vector kernels carry their events on the dispatch (start / end of the kernel itself); the tile
    // kernels are bracketed by recorded events (milliseconds long: the brackets' own latency does not matter there)
    const bool ride = fam == kVector;
    if (timing && !ride) HIP_TRY(hipEventRecord(own.e0, st));
    int lrc = !frame_loop          ? 0
              : one                ? launch_logl_one(geom, p, w, grid, lds + LdsLayout::hand_bytes(), (void *)st, timing ? (void *)own.e0 : nullptr,
                                                     timing ? (void *)own.e1 : nullptr)
              : fam == kWide       ? launch_logl_wide(m.NP, p, grid, (void *)st)
              : fam == kModalTiles ? launch_logl_modal_mfma(m.NPm[kModal], p, (void *)st)
              : fam == kDenseTiles ? launch_logl_dense_mfma(m.NPm[kDense], p, (void *)st)
                                   : launch_logl(geom, mode, p, grid, lds, (void *)st, timing ? (void *)own.e0 : nullptr, timing ? (void *)own.e1 : nullptr);
    if (lrc != 0) return fail(BILD_ERR_HIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
    if (!building) m.last_geom = fam == kVector && frame_loop ? geom.id : -1;
    if (timing) {
        if (!frame_loop) HIP_TRY(hipEventRecord(own.e0, st)); // (no dispatch for the events to ride on: an empty bracket)
        if (!ride || !frame_loop) HIP_TRY(hipEventRecord(own.e1, st));
        std::lock_guard<std::mutex> lk(g_time_mu);
        g_time_events.emplace_back(own.e0, own.e1);
        own.e0 = own.e1 = nullptr;
        g_time_name = fam == kWide ? "logl_wide_kernel" : fam == kModalTiles ? "logl_modal_mfma_kernel" : fam == kDenseTiles ? "logl_dense_mfma_kernel" : one ? "logl_one_kernel<modal>" : kernel_name(geom, mode);
    }
    if (ts.dstar_max > 1) {
        lrc = launch_reduce_partials(target, d_out, n, ts.dstar_max, (void *)st);
        if (lrc != 0) return fail(BILD_ERR_HIP, "reduce launch failed: %s", hipGetErrorString((hipError_t)lrc));
    }
    if (st_in && !split) {
        // every row went through the frame loop, the refused ones with a marked list of no switch: NaN for them, as in a split
        // launch (entries that leave their results on the device cannot refuse a row otherwise)
        lrc = launch_mark_refused_rows(d_seg_start, K1, n, d_out, (void *)st);
        if (lrc != 0) return fail(BILD_ERR_HIP, "launch failed: %s", hipGetErrorString((hipError_t)lrc));
    }
    return BILD_OK;
}

// Launch order of a batch (vector kernels, modal path, tables in use).  Candidates differ in the number of frames they run
// themselves; the four (or so) tasks of a wavefront are independent rows of one instruction stream, so the wave lives as long
// as its busiest row.
//  1. sort by the work a candidate will do, most first: a wave's rows then finish together, and long work is dispatched
//     first.  The work is estimated from the candidate's switches and the transient table's frames-to-convergence (with
//     BILD_NO_JUMP: the remaining length behind the first switch);
//  2. when the whole grid is resident at once -- at most OCC workgroups per CU -- nothing is ever re-balanced at run time:
//     the dispatcher deals workgroups to the 256 CUs round-robin (workgroups b, b + 256, b + 512 share a CU;
//     measured: profiles/r02_placement.txt), so the sorted workgroups are dealt to CUs longest-processing-time-first
//     with the CU's number of workgroups as capacity, and written out in that dealing order.
// Purely a matter of speed: results do not depend on the order, and nothing relies on the dispatcher behaving so.
// order[slot] = sample.  Returns false when the identity is as good (nothing written).
bool schedule(const bild_model &m, const bild_trajset &ts, int64_t n, int K1, const int32_t *seg_start, const int32_t *seg_state,
              const int32_t *traj_id, unsigned flags, int32_t *order, bool inside_a_call)
{
    int mode;
    if (n < 2 || K1 < 2 || n > INT_MAX || pick_mode(m, flags, &mode) || mode != kModal || m.wide || m.mid) return false;
    if ((flags & BILD_NO_PREFIX) || ts.prefix_state < 0 || config().no_prefix || config().no_schedule) return false;
    const bool jumps = !(flags & BILD_NO_JUMP) && !config().no_jump;
    // with jumps but without a transient table every switch costs about the same wherever it is: nothing to sort by
    if (jumps && ts.trans_state != 1) return false;
    // Measured on the 10k batch (profiles/r02_transients.txt): with the tables the order is worth 22 us of kernel time and
    // costs 62 us of host time -- inside a host-buffer call it does not pay; a caller with resident candidates computes
    // it once (bild_schedule_segments) and reuses it.
    if (jumps && inside_a_call) return false;
    Geometry geom{};
    if (!geometry_for(m.NPm[mode], mode, n * ts.dstar_max, ts.means_max, &geom)) return false;
    const int Tmax = ts.Tmax, m_typ = ts.trans_m_typ;
    const bool pairs = ts.trans2_state == 1;
    std::vector<int32_t> count((size_t)Tmax + 2, 0), work((size_t)n);
    for (int64_t r = 0; r < n; ++r) {
        const TrajDesc &td = ts.descs[traj_id ? traj_id[r] : 0];
        const int T = td.T;
        const int32_t *a = seg_start + r * K1;
        int w = 0;
        if (!jumps) {
            int t0 = a[1];
            t0 = t0 < 1 ? 1 : (t0 > T ? T : t0);
            w = T - t0;
        } else {
            // Frames the candidate will run itself, estimated from its switch frames alone (chain_work.h), over the list as
            // given.  (Boundaries that switch nothing are rare and only blur the estimate.)
            ChainWork cw{m_typ, pairs};
            for (int i = 1; i < K1; ++i) {
                const int t = a[i];
                if (t >= T) break;
                cw.add(t, ((i + 1 < K1 && a[i + 1] < T) ? a[i + 1] : T) - t);
            }
            w = cw.finish(T);
            w = w > Tmax ? Tmax : w;
        }
        w = w < 0 ? 0 : w; // (a row of decreasing starts can make the estimate negative; host entries reject such rows beforehand)
        work[r] = w;
        ++count[Tmax - w + 1];
    }
    for (int i = 1; i <= Tmax + 1; ++i) count[i] += count[i - 1];
    std::vector<int32_t> sorted((size_t)n);
    for (int64_t r = 0; r < n; ++r) sorted[count[Tmax - work[r]]++] = (int32_t)r;
    if (jumps) {
        // Most candidates of a batch run no frame at all, a few run hundreds, and the rows of a wave share one instruction
        // stream: every event of a row (basis change, comparison, jump) is paid by the whole wave.  So the busy candidates
        // are SPREAD: the heaviest go one per wave, the next heaviest fill the second rows, and so on -- a wave then holds
        // one long row and light ones instead of four long rows whose events add up.
        const int64_t rpw = geom.tasks_per_wave() % ts.dstar_max == 0 ? geom.tasks_per_wave() / ts.dstar_max : 1;
        // ... round by round: the waves the chip holds at once (256 CUs x OCC workgroups x W waves) take the heaviest
        // candidates that fit into them, spread as above; the next round the next heaviest, and so on.  A batch that fits
        // the chip once is one round (plain spreading: the 10k batch, latency-bound by its longest chain); a batch many
        // times that size with few busy candidates has them all in its first round.
        // A batch of several rounds with more busy candidates than one round has waves is throughput-bound whatever the
        // order: then candidates of equal work share a wave (the sorted order as it is), heaviest waves first
        // (`profiles/r02_launch_order.txt`: 80 000 candidates 220 -> 157 us, configs[2]'s 256 000 1.77 -> 0.92 ms; a batch
        // that fits the chip once is better off spread even when every wave has busy rows: 10 000 x k = 8, 123 vs 152 us).
        const int64_t slots = (int64_t)256 * geom.OCC * geom.W * rpw;
        int64_t busy = 0;
        while (busy < n && work[sorted[busy]] > 0) ++busy;
        const bool packed = n > slots && busy > slots / rpw;
        if (packed) {
            std::copy(sorted.begin(), sorted.end(), order);
            return true;
        }
        const int64_t round = std::max<int64_t>(slots, rpw);
        for (int64_t base = 0; base < n; base += round) {
            const int64_t cnt = std::min(round, n - base), nw = cnt / rpw, n_full = nw * rpw;
            for (int64_t w = 0; w < nw; ++w)
                for (int64_t j = 0; j < rpw; ++j) order[base + w * rpw + j] = sorted[base + j * nw + w];
            for (int64_t i = n_full; i < cnt; ++i) order[base + i] = sorted[base + i]; // the lightest few: a last, partial wave
        }
        return true;
    }
    const int64_t per_block = std::max<int64_t>(1, (int64_t)geom.W * geom.tasks_per_wave() / ts.dstar_max);
    const int64_t nb = (n + per_block - 1) / per_block;
    const int kCUs = 256;
    if (nb <= kCUs || nb > (int64_t)kCUs * geom.OCC || (int64_t)geom.W * geom.tasks_per_wave() % ts.dstar_max != 0) {
        std::copy(sorted.begin(), sorted.end(), order);
        return true;
    }
    // blocks of the sorted list, longest first; block length = its first (longest) sample
    const int rounds = (int)((nb + kCUs - 1) / kCUs);
    const int extra = (int)(nb - (int64_t)(rounds - 1) * kCUs); // CUs 0 .. extra-1 take `rounds` workgroups, the others one less
    typedef std::pair<int64_t, int> Load; // (work so far, CU)
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> heap;
    for (int c = 0; c < kCUs; ++c) heap.push(Load(0, c));
    std::vector<int> filled(kCUs, 0);
    std::vector<int64_t> at((size_t)nb, -1); // launch position -> block of the sorted list
    for (int64_t b = 0; b < nb; ++b) {
        const Load top = heap.top();
        heap.pop();
        const int c = top.second;
        at[(size_t)c + (size_t)kCUs * filled[c]] = b;
        ++filled[c];
        const int cap = c < extra ? rounds : rounds - 1;
        if (filled[c] < cap) heap.push(Load(top.first + work[sorted[b * per_block]] + 1, c));
    }
    // only the last block of the sorted list can be short: it goes to the last position, so that blocks of samples and
    // workgroups stay aligned
    for (int64_t pos = 0; pos < nb; ++pos)
        if (at[(size_t)pos] == nb - 1) {
            std::swap(at[(size_t)pos], at[(size_t)nb - 1]);
            break;
        }
    int64_t w = 0;
    for (int64_t pos = 0; pos < nb; ++pos) {
        const int64_t b = at[(size_t)pos];
        const int64_t lo = b * per_block, hi = std::min(n, lo + per_block);
        for (int64_t i = lo; i < hi; ++i) order[w++] = sorted[i];
    }
    return true;
}

// Launch order for a host-buffer call, computed on the device behind the upload (schedule.hip): only where it pays -- a
// batch of several rounds on a trajectory set whose tables exist (from its second evaluation on); 1: no order (array order)
int device_order(const bild_model &m, const bild_trajset &ts, int64_t n, int K1, const int32_t *d_start, const int32_t *d_tid,
                 unsigned flags, hipStream_t st, const int32_t **d_order)
{
    if (n < 2 || K1 < 2 || n > INT_MAX || m.wide || m.mid || !m.modal_ok) return 1;
    const unsigned path = flags & 0xFu;
    if (path != BILD_PATH_AUTO && path != BILD_PATH_MODAL) return 1;
    if ((flags & (BILD_NO_PREFIX | BILD_NO_JUMP)) || config().no_prefix || config().no_jump || config().no_schedule) return 1;
    if (ts.prefix_state != 1 || ts.trans_state != 1) return 1;
    // a split launch orders its frame loop itself (work lists by expected work)
    if (K1 <= kSplitMaxK1 && !config().no_split) return 1;
    Geometry geom{};
    if (!geometry_for(m.NPm[kModal], kModal, n * ts.dstar_max, ts.means_max, &geom)) return 1;
    if (geom.tasks_per_wave() % ts.dstar_max != 0) return 1;
    const int rpw = geom.tasks_per_wave() / ts.dstar_max;
    const int64_t slots = (int64_t)256 * geom.OCC * geom.W * rpw;
    if (n <= slots) return 1; // one round: the order does not matter (10k batch: 80 vs 81 us)
    const size_t bytes = device_schedule_bytes(n);
    {
        std::lock_guard<std::mutex> lk(m.mu);
        if (m.ws_sched.reserve(bytes)) return 1;
    }
    return device_schedule(d_start, d_tid, ts.d_descs, K1, n, ts.trans_m_typ, ts.trans2_state == 1 ? 1 : 0, ts.Tmax, rpw, slots, m.ws_sched.ptr,
                           m.ws_sched.cap, d_order, (void *)st);
}

} // namespace bild

extern "C" {

int bild_debug_frames_per_task(int32_t *d_buffer)
{
    g_frames_task.store(d_buffer);
    return BILD_OK;
}

int bild_kernel_timing_read_walk(double *total_ms, int64_t *launches)
{
    if (!total_ms || !launches) return fail(BILD_ERR_INVALID, "NULL argument");
    return drain(g_walk_events, total_ms, launches);
}

int bild_kernel_timing(int enable)
{
    std::lock_guard<std::mutex> lk(g_time_mu);
    g_time_on = enable < 0 ? 0 : enable;
    g_time_count = 0;
    return BILD_OK;
}

int bild_kernel_timing_read(double *total_ms, int64_t *launches, char *name, int name_len)
{
    if (!total_ms || !launches) return fail(BILD_ERR_INVALID, "NULL argument");
    std::string nm;
    if (int rc = drain(g_time_events, total_ms, launches, &nm)) return rc;
    if (name && name_len > 0) std::snprintf(name, (size_t)name_len, "%s", nm.c_str());
    return BILD_OK;
}

} // extern "C"
