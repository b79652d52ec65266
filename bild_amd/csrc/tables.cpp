// The trajectory sets behind bild_trajset handles: their upload, and the tables built for them at their first evaluation
// (prefix table with its first-order tails, transient and state tables, pair table), in memory recycled by a cache that
// nothing outside this file knows of.
#include <map>
#include <new>
#include <unordered_map>

#include "likelihood.h"

namespace {

constexpr int kZeroPad = 8;
// bild_trajset_expect: below these many declared evaluations the prefix (+ transient) tables / the pair and state tables are not built
constexpr int64_t kExpectPrefix = 300, kExpectPairs = 3000;

// Table memory is recycled.  hipFree of a block of two megabytes or more unmaps it -- 0.22 ms a piece, whatever its size: 0.9 ms per
// trajectory set between the scratch of its builders and its three large tables, a tenth of what `sample` spends on an ordinary
// trajectory when they come one after the other (rocprofv3 --hip-trace of tools/first_call.py).  Blocks of 128 KiB and more are therefore
// rounded up to a size class (powers of two in quarter steps) and kept for the next trajectory set when they are released -- up to
// BILD_TABLE_CACHE_BYTES (default 4 GB; 0: every block goes back to the driver at once).  A request that cannot be met flushes the cache
// and asks again.  Nothing is returned at process exit (the runtime may be gone by then).
// One rule orders the cache against the device: a block goes back to it (tab_free) only after the stream that used it has
// been synchronised -- on every path, failure paths included.  tab_malloc hands a block straight on, and a memset, copy or
// kernel still queued behind its last user would write into its next one.  The builders keep to the rule through TabScratch,
// bild_trajset_destroy by synchronising the device.
struct TableCache {
    std::mutex mu;
    std::multimap<size_t, void *> idle;         // size class -> block
    std::unordered_map<void *, size_t> classes; // every block handed out or idle that came from here
    size_t held = 0;
    static size_t size_class(size_t bytes)
    {
        size_t c = (size_t)128 << 10;
        while (c < bytes) {
            const size_t q = c / 4;
            for (int k = 1; k <= 4 && c < bytes; ++k) c += q; // c, 1.25 c, 1.5 c, 1.75 c, 2 c
        }
        return c;
    }
    void flush_locked()
    {
        for (auto &kv : idle) {
            classes.erase(kv.second);
            (void)hipFree(kv.second);
        }
        idle.clear();
        held = 0;
    }
};
TableCache g_tables;

hipError_t tab_malloc(void **out, size_t bytes)
{
    *out = nullptr;
    const int64_t cap = config().table_cache_bytes;
    if (cap <= 0 || bytes < ((size_t)128 << 10)) return hipMalloc(out, bytes);
    int dev = 0;
    (void)hipGetDevice(&dev);
    const size_t bytes_cls = TableCache::size_class(bytes);
    const size_t cls = bytes_cls | ((size_t)dev << 56); // (blocks stay on the device they were made on)
    std::lock_guard<std::mutex> lk(g_tables.mu);
    auto it = g_tables.idle.find(cls);
    if (it != g_tables.idle.end()) {
        *out = it->second;
        g_tables.held -= bytes_cls;
        g_tables.idle.erase(it);
        return hipSuccess;
    }
    hipError_t e = hipMalloc(out, bytes_cls);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_tables.flush_locked();
        e = hipMalloc(out, bytes_cls);
    }
    if (e == hipSuccess) g_tables.classes[*out] = cls;
    return e;
}

void tab_free(void *ptr)
{
    if (!ptr) return;
    std::unique_lock<std::mutex> lk(g_tables.mu);
    auto it = g_tables.classes.find(ptr);
    if (it == g_tables.classes.end()) { // (a small block, or the cache is off)
        lk.unlock();
        (void)hipFree(ptr);
        return;
    }
    const size_t cls = it->second, bytes_cls = cls & (((size_t)1 << 56) - 1);
    const int64_t cap = config().table_cache_bytes;
    if (cap > 0 && g_tables.held + bytes_cls <= (size_t)cap) {
        g_tables.idle.emplace(cls, ptr);
        g_tables.held += bytes_cls;
        return;
    }
    g_tables.classes.erase(it);
    lk.unlock();
    (void)hipFree(ptr);
}

// Table memory of one build on stream `st`, and the steps the build runs there.  What is not kept goes back to the cache when
// the build is over, by whatever path, after `st` has been synchronised (the rule above): run() ends with a synchronisation,
// and what was enqueued outside run() -- before it, by a build that gave up half way -- is waited for here.  A failed step
// leaves its error behind, but a table is an optimisation and its build nobody's error: that is cleared here as well.
class TabScratch {
public:
    explicit TabScratch(hipStream_t st) : st_(st) {}
    ~TabScratch()
    {
        if (!blocks_.empty() && !idle_) (void)hipStreamSynchronize(st_);
        for (void *b : blocks_) tab_free(b);
        if (e0_) (void)hipEventDestroy(e0_);
        if (e1_) (void)hipEventDestroy(e1_);
        (void)hipGetLastError();
    }
    template <typename T> bool alloc(T **out, size_t bytes)
    {
        void *b = nullptr;
        *out = nullptr;
        if (tab_malloc(&b, bytes) != hipSuccess) return false;
        blocks_.push_back(b);
        *out = (T *)b;
        return true;
    }
    // the block has become a table of the set: it stays
    template <typename T> T *keep(T *b)
    {
        auto it = std::find(blocks_.begin(), blocks_.end(), (void *)b);
        if (it != blocks_.end()) blocks_.erase(it);
        return b;
    }
    // `enqueue` (true: all of it enqueued) on `st`, then a synchronisation of `st`, also when enqueueing failed half way.  With
    // `ms`: between two events, whose elapsed milliseconds are added to *ms on success.
    template <typename F> bool run(F &&enqueue, double *ms = nullptr)
    {
        if (ms && !e0_ && (hipEventCreate(&e0_) != hipSuccess || hipEventCreate(&e1_) != hipSuccess)) return false;
        if (ms) (void)hipEventRecord(e0_, st_);
        bool ok = enqueue();
        if (ms) (void)hipEventRecord(e1_, st_);
        idle_ = hipStreamSynchronize(st_) == hipSuccess;
        ok = ok && idle_;
        float t = 0.f;
        if (ok && ms && hipEventElapsedTime(&t, e0_, e1_) == hipSuccess) *ms += t;
        return ok;
    }

private:
    hipStream_t st_;
    std::vector<void *> blocks_;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
    bool idle_ = false; // the last thing the build did on st_ was a run() that synchronised it
};

// the first-order tails beside the prefix table (tail.hip): one backward pass per (trajectory, chain, state)
void build_tails(const bild_model &m, const bild_trajset &ts, hipStream_t st)
{
    const int S = m.S, NP = m.NPm[kModal];
    const size_t gbytes = (size_t)ts.prefix_records * kDMax * NP * sizeof(double);
    std::vector<int64_t> first((size_t)ts.n_traj + 1, 0); // blocks of the parallel phase, trajectory by trajectory
    for (int j = 0; j < ts.n_traj; ++j) first[(size_t)j + 1] = first[j] + (int64_t)ts.dstar_max * S * ts.descs[j].T;
    TabScratch scratch(st);
    double *d_g, *d_gain;
    int64_t *d_first;
    const bool ok = first.back() == ts.prefix_records && first.back() < ((int64_t)1 << 31) && scratch.alloc(&d_g, gbytes) &&
                    scratch.alloc(&d_gain, (size_t)ts.prefix_records * (NP + 4) * sizeof(double)) &&
                    scratch.alloc(&d_first, first.size() * sizeof(int64_t)) &&
                    hipMemcpy(d_first, first.data(), first.size() * sizeof(int64_t), hipMemcpyHostToDevice) == hipSuccess &&
                    scratch.run([&] {
                        return launch_tail(ts.d_descs, ts.n_traj, S, NP, m.d, ts.dstar_max, m.d_states[kModal], ts.d_prefix, d_first,
                                           first.back(), d_gain, d_g, (void *)st) == 0;
                    }, &ts.prefix_build_ms);
    if (ok) ts.d_tail_g = scratch.keep(d_g);
}

} // namespace

namespace bild {

// The prefix table of a trajectory set (common.h), built once: the likelihood kernel itself runs one task per
// (trajectory, covariance chain, initial state) with a profile that never switches and stores its state after every
// frame.  Synchronous (the one-time cost of a set, like its upload); afterwards any stream may read the table.
int ensure_prefix(const bild_model &m, const bild_trajset &ts, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(ts.prefix_mu);
    if (ts.prefix_state != 0) return BILD_OK;
    ts.prefix_state = -1;
    if (config().no_prefix) return BILD_OK;
    if (ts.expected_evals >= 0 && ts.expected_evals < kExpectPrefix) return BILD_OK; // a few hundred evaluations: cheaper frame by frame
    const int NP = m.NPm[kModal];
    Geometry geom{};
    if (!builder_geometry(NP, &geom)) return BILD_OK;
    const size_t lds = lds_bytes(m, geom, kModal);
    if (lds > 160 * 1024) return BILD_OK;
    const size_t bytes = (size_t)ts.prefix_records * prefix_record_doubles(NP) * sizeof(double);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return BILD_OK;
    if (bytes > free_b / 4 || bytes > ((size_t)16 << 30)) return BILD_OK; // the table is an optimisation, not a requirement
    const int S = m.S;
    const int64_t nb = (int64_t)ts.n_traj * S;
    std::vector<int32_t> host((size_t)3 * nb);
    for (int j = 0; j < ts.n_traj; ++j)
        for (int s = 0; s < S; ++s) {
            host[(size_t)j * S + s] = 0;                 // seg_start
            host[(size_t)nb + (size_t)j * S + s] = s;    // seg_state
            host[(size_t)2 * nb + (size_t)j * S + s] = j; // traj_id
        }
    {
        TabScratch scratch(st);
        int32_t *d_desc;
        double *d_tab, *d_sink, *d_L;
        const bool ok = scratch.alloc(&d_desc, host.size() * sizeof(int32_t)) &&
                        scratch.alloc(&d_sink, (size_t)nb * ts.dstar_max * sizeof(double)) && scratch.alloc(&d_tab, bytes) &&
                        scratch.alloc(&d_L, (size_t)ts.prefix_records * sizeof(double)) &&
                        hipMemsetAsync(d_L, 0, (size_t)ts.prefix_records * sizeof(double), st) == hipSuccess &&
                        hipMemcpy(d_desc, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
                        scratch.run([&] {
                            KParams p{};
                            fill_params(m, ts, kModal, p);
                            p.ntasks = nb * ts.dstar_max;
                            p.K1 = 1;
                            p.seg_start = d_desc;
                            p.seg_state = d_desc + nb;
                            p.traj_id = d_desc + 2 * nb;
                            p.out = d_sink;
                            p.prefix_dump = d_tab;
                            p.prefix_L_dump = d_L;
                            const int64_t tpb = (int64_t)geom.W * geom.tasks_per_wave();
                            const int grid = (int)std::min<int64_t>(std::max<int64_t>((p.ntasks + tpb - 1) / tpb, 1), 256 * 16);
                            return launch_logl(geom, kModal, p, grid, lds, (void *)st) == 0 &&
                                   launch_prefix_L(ts.d_descs, ts.n_traj, S, NP, ts.dstar_max, ts.Tmax, d_tab, d_L, (void *)st) == 0; // (the records' running log-likelihoods)
                        }, &ts.prefix_build_ms);
        if (!ok) return BILD_OK;
        ts.d_prefix = scratch.keep(d_tab);
        ts.d_prefix_L = scratch.keep(d_L);
    }
    if (!m.has_G && !config().no_tail) build_tails(m, ts, st);
    ts.prefix_state = 1;
    return BILD_OK;
}

// The transient table of a trajectory set (common.h: TransEntry), built once behind the prefix table: one ordinary
// two-segment candidate per (trajectory, old state, new state, switch frame), evaluated by the likelihood kernel in its
// table-building mode (it stops at the first successful convergence check and writes the entry instead of a result).
int ensure_transients(const bild_model &m, const bild_trajset &ts, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(ts.prefix_mu);
    if (ts.trans_state != 0) return BILD_OK;
    ts.trans_state = -1;
    if (ts.prefix_state != 1 || config().no_transients || config().no_jump || m.S < 2) return BILD_OK;
    const int S = m.S;
    int64_t nb = 0;
    for (const TrajDesc &td : ts.descs) nb += (int64_t)std::max(td.T - 1, 0) * S * (S - 1);
    // the table is an optimisation: not for models with so many states that building it costs more than it can save
    if (nb == 0 || nb > ((int64_t)4 << 20)) return BILD_OK;
    const size_t bytes = (size_t)ts.trans_entries * sizeof(TransEntry);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 4) return BILD_OK;
    std::vector<int32_t> host((size_t)5 * nb); // seg_start (2 per sample) | seg_state (2 per sample) | traj_id
    int64_t r = 0;
    for (int j = 0; j < ts.n_traj; ++j)
        for (int s = 0; s < S; ++s)
            for (int sn = 0; sn < S; ++sn) {
                if (sn == s) continue;
                for (int t = 1; t < ts.descs[j].T; ++t, ++r) {
                    host[(size_t)2 * r] = 0;
                    host[(size_t)2 * r + 1] = t;
                    host[(size_t)2 * nb + 2 * r] = s;
                    host[(size_t)2 * nb + 2 * r + 1] = sn;
                    host[(size_t)4 * nb + r] = j;
                }
            }
    TabScratch scratch(st);
    int32_t *d_desc;
    double *d_sink, *d_states = nullptr;
    TransEntry *d_tab;
    // First launch: the entries alone.  How long transients last is not known before it has run, and the state table beside
    // the entries (common.h: a chain of close switches starts at its second switch) needs a record for every gap a chain can
    // START with -- gaps shorter than the first switch's transient, i.e. up to the longest converged transient of THIS set,
    // not a compile-time 64: the default model's longest is 45 frames (141 -> ~100 MB per 1000-frame trajectory).
    auto build_pass = [&](double *states) {
        ts.d_trans = d_tab; // launch_batch passes it on as the table to FILL (trans_state is still -1)
        ts.d_strans = states;
        LaunchIn in;
        in.fill = LaunchIn::kFillTransients;
        const bool good = scratch.run([&] {
            return launch_batch(m, ts, nb, 2, d_desc, d_desc + 2 * nb, d_desc + 4 * nb, nullptr, BILD_PATH_MODAL, st, d_sink, in) == BILD_OK;
        }, &ts.trans_build_ms);
        ts.d_trans = nullptr;
        ts.d_strans = nullptr;
        return good;
    };
    const bool ok = scratch.alloc(&d_desc, host.size() * sizeof(int32_t)) && scratch.alloc(&d_sink, (size_t)nb * sizeof(double)) &&
                    scratch.alloc(&d_tab, bytes) && hipMemsetAsync(d_tab, 0, bytes, st) == hipSuccess &&
                    hipMemcpy(d_desc, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess && build_pass(nullptr);
    if (!ok) return BILD_OK;
    std::vector<TransEntry> all((size_t)ts.trans_entries);
    if (hipMemcpy(all.data(), d_tab, bytes, hipMemcpyDeviceToHost) != hipSuccess) return BILD_OK;
    std::vector<int32_t> ms;
    for (const TransEntry &en : all)
        if (en.m > 0) ms.push_back(en.m);
    // longest transient that converged (entries that ran into the trajectory's end say nothing about the filter)
    {
        int64_t i0 = 0;
        for (const TrajDesc &td : ts.descs) {
            const int64_t cnt = (int64_t)td.T * S * S * ts.dstar_max;
            for (int64_t i = 0; i < cnt; ++i) {
                const TransEntry &en = all[(size_t)(i0 + i)];
                const int t = (int)(i % td.T);
                if (en.m > 0 && t + en.m < td.T) ts.trans_m_max = std::max(ts.trans_m_max, (int)en.m);
            }
            i0 += cnt;
        }
    }
    if (!ms.empty()) {
        std::nth_element(ms.begin(), ms.begin() + ms.size() * 9 / 10, ms.end());
        ts.trans_m_typ = ms[ms.size() * 9 / 10];
    }
    // Second launch: the same candidates once more, now leaving their states -- an optimisation with a budget.  The table
    // costs what its allocation and its fill cost (tens of GB per second: 26 GB, 0.8 s, for the 256 trajectories of BASELINE
    // configs[2]) and saves ~10 us per launch on the chains of close switches: worth it for sets of a few trajectories that
    // see batch after batch (one trajectory: 2 ms against 9 us per AMIS step), not for hundreds of them.  4 GB unless the
    // caller has declared >= 1e8 evaluations on the set (then 64 GB) or BILD_STATES_MAX_BYTES says otherwise; always at most
    // a third of the free memory.  Which tables exist depends on the set and that declaration alone (reproducibility).
    if (!config().no_states && !(ts.expected_evals >= 0 && ts.expected_evals < kExpectPairs) && ts.trans_m_max >= 2) {
        int sgap = std::min<int>(std::max(2, std::min(config().states_max_gap, 255)), ts.trans_m_max + 1);
        const int sstride = std::max(1, std::min(config().states_stride, 8));
        int snq = (sgap - 2) / sstride + 1; // records for g = 1, 1 + sstride, ... <= sgap - 1
        const size_t per_q = (size_t)ts.strans_entries * prefix_record_doubles(m.NPm[kModal]) * sizeof(double);
        size_t budget = (size_t)std::max<int64_t>(config().states_max_bytes, 0);
        if (config().states_max_bytes < 0) budget = ts.expected_evals >= (int64_t)100000000 ? ((size_t)64 << 30) : ((size_t)4 << 30);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 3);
        else budget = 0;
        // a table that would not fit covers the SHORT gaps (every chain saves its basis change, the frames saved grow with the
        // gap): as many records per switch as the budget holds, none below gaps of ~16 -- for sets of up to 32 trajectories:
        // what the table saves is the latency of a launch's longest chain, which does not grow with the number of
        // trajectories, while its cost does (configs[2], 256 trajectories: -11 % per step for 8.7 GB and 0.3 s)
        if ((size_t)snq * per_q > budget && per_q > 0) {
            snq = ts.n_traj <= 32 ? (int)(budget / per_q) : 0;
            sgap = snq * sstride + 1;
            if (snq * sstride < 16) snq = 0;
        }
        const size_t sbytes = (size_t)snq * per_q;
        if (snq > 0 && scratch.alloc(&d_states, sbytes)) {
            ts.sgap = sgap;
            ts.sstride = sstride;
            ts.snq = snq;
            ts.strans_records = ts.strans_entries * snq;
            if (!build_pass(d_states)) { // (the entries are complete; only the state table is lost)
                d_states = nullptr;
                ts.strans_records = 0;
            }
        }
    }
    ts.d_trans = scratch.keep(d_tab);
    ts.d_strans = scratch.keep(d_states);
    ts.trans_state = 1;
    return BILD_OK;
}

// The pair table (common.h): two switches closer together than the first one's transient, as one entry.  Built like the
// transient table, by the kernel itself, from candidates with two switches: one per (trajectory, s -> sn -> sm, frame, gap).
// Only for trajectory sets where it can pay: the build is a launch of (T - 1) (gap_max - 1) S (S-1)^2 short tasks per
// trajectory, worth it for sets that see batch after batch of candidates (one trajectory, ten thousand candidates per AMIS
// step), not for hundreds of trajectories with a few candidates each -- decided by the size of the build alone, so that a
// result never depends on what was evaluated before.
int ensure_pairs(const bild_model &m, const bild_trajset &ts, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(ts.prefix_mu);
    if (ts.trans2_state != 0) return BILD_OK;
    ts.trans2_state = -1;
    if (ts.trans_state != 1 || config().no_pairs || m.S < 2) return BILD_OK;
    if (ts.expected_evals >= 0 && ts.expected_evals < kExpectPairs) return BILD_OK; // (the second-level tables pay from a few thousand evaluations on)
    // gaps the table covers: up to the longest converged transient of the single table, 128 at most (BILD_PAIRS_MAX_GAP: another cap --
    // slow chains, whose transients last longer, leave more pairs to the frame loop)
    const int gap_cap = config().pairs_max_gap;
    const int S = m.S, G = std::min(gap_cap, ts.trans_m_max);
    if (G < 2) return BILD_OK;
    int64_t nb = 0;
    for (const TrajDesc &td : ts.descs) nb += (int64_t)std::max(td.T - 1, 0) * (G - 1) * S * (S - 1) * (S - 1);
    // (BILD_PAIRS_MAX_TASKS=<n>: another budget, for sets of many trajectories that will see hundreds of batches)
    const int64_t budget = config().pairs_max_tasks;
    if (nb == 0 || nb > budget) return BILD_OK;
    const int64_t entries = ts.trans_entries * S * G;
    const size_t bytes = (size_t)entries * sizeof(TransEntry);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 4) return BILD_OK;
    // the build candidates -- seg_start (3 per task) | seg_state (3 per task) | traj_id -- are written on the device
    // (schedule.hip: pair_tasks_kernel): up to tens of millions of them, nothing the host should fill and send
    std::vector<int64_t> first((size_t)ts.n_traj + 1, 0);
    for (int j = 0; j < ts.n_traj; ++j)
        first[(size_t)j + 1] = first[j] + (int64_t)std::max(ts.descs[j].T - 1, 0) * (G - 1) * S * (S - 1) * (S - 1);
    TabScratch scratch(st);
    int32_t *d_desc;
    int64_t *d_first;
    double *d_sink;
    TransEntry *d_tab;
    LaunchIn in;
    in.fill = LaunchIn::kFillPairs;
    // The pair state table (common.h), filled by the same launch: the second level of the state table, gated like the first and
    // from the same byte budget (ensure_transients), of which the first level has taken its share.  It is built whole or not at
    // all: what it saves is the second gap of a launch's longest chain, and short gaps alone do not shorten that chain.
    double *d_pstates = nullptr;
    int pgap = 0, pnq = 0;
    const int pstride = std::max(1, std::min(config().pair_states_stride, 8));
    if (!config().no_states && !config().no_pair_states && ts.d_strans != nullptr) {
        const size_t rec_bytes = (size_t)prefix_record_doubles(m.NPm[kModal]) * sizeof(double);
        pgap = std::min<int>(std::max(2, std::min(config().states_max_gap, 255)), ts.trans_m_max + 1);
        pnq = (pgap - 2) / pstride + 1; // records for g2 = 1, 1 + pstride, ... <= pgap - 1
        const size_t pbytes = pair_state_records(ts.prefix_records, S, G, pnq) * rec_bytes;
        size_t budget = (size_t)std::max<int64_t>(config().states_max_bytes, 0);
        if (config().states_max_bytes < 0) budget = ts.expected_evals >= (int64_t)100000000 ? ((size_t)64 << 30) : ((size_t)4 << 30);
        const size_t first_level = (size_t)ts.strans_records * rec_bytes;
        budget = budget > first_level ? budget - first_level : 0;
        budget = std::min(budget, (free_b > bytes ? free_b - bytes : 0) / 3);
        // (the walk plan holds a record's number in 32 bits: logl_body.h, "pair state starts")
        const bool fits = pbytes <= budget && pair_state_records(ts.prefix_records, S, G, pnq) < ((int64_t)1 << 31);
        if (!fits || !scratch.alloc(&d_pstates, pbytes)) d_pstates = nullptr;
    }
    const bool ok = scratch.alloc(&d_desc, (size_t)7 * nb * sizeof(int32_t)) && scratch.alloc(&d_first, first.size() * sizeof(int64_t)) &&
                    scratch.alloc(&d_sink, (size_t)nb * sizeof(double)) && scratch.alloc(&d_tab, bytes) &&
                    hipMemsetAsync(d_tab, 0, bytes, st) == hipSuccess &&
                    hipMemcpyAsync(d_first, first.data(), first.size() * sizeof(int64_t), hipMemcpyHostToDevice, st) == hipSuccess &&
                    launch_pair_tasks(d_first, ts.n_traj, ts.d_descs, S, G, nb, d_desc, d_desc + 3 * nb, d_desc + 6 * nb, (void *)st) == 0 &&
                    scratch.run([&] {
                        ts.d_trans2 = d_tab; // launch_batch passes it on as the table to FILL (trans2_state is still -1)
                        ts.gap_max = G;
                        ts.d_pstrans = d_pstates; // (likewise; null: the entries alone)
                        ts.pgap = pgap;
                        ts.pstride = pstride;
                        ts.pnq = pnq;
                        return launch_batch(m, ts, nb, 3, d_desc, d_desc + 3 * nb, d_desc + 6 * nb, nullptr, BILD_PATH_MODAL, st, d_sink, in) == BILD_OK;
                    }, &ts.trans2_build_ms);
    ts.d_trans2 = nullptr;
    ts.d_pstrans = nullptr;
    if (!ok) return BILD_OK; // (`first` is read by an asynchronous copy: declared before `scratch`, it outlives its synchronisation)
    // do the tables cover every candidate of at most two switches?  (schedule.hip: two_switch_cover_kernel)
    std::vector<int64_t> ent((size_t)ts.n_traj + 1, 0);
    for (int j = 0; j < ts.n_traj; ++j)
        ent[(size_t)j + 1] = ent[j] + (int64_t)ts.descs[j].dstar * S * (S - 1) * std::max(ts.descs[j].T - 1, 0);
    int64_t *d_ent;
    int *d_cov;
    int cov = 1;
    const bool good = scratch.alloc(&d_ent, ent.size() * sizeof(int64_t)) && scratch.alloc(&d_cov, sizeof(int)) &&
                      hipMemcpy(d_ent, ent.data(), ent.size() * sizeof(int64_t), hipMemcpyHostToDevice) == hipSuccess &&
                      hipMemcpy(d_cov, &cov, sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
                      scratch.run([&] { return launch_two_switch_cover(ts.d_descs, d_ent, ent.back(), ts.n_traj, S, ts.d_trans, d_tab, G, d_cov, (void *)st) == 0; }) &&
                      hipMemcpy(&cov, d_cov, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    ts.two_switch_covered = good && cov == 1 ? 1 : 0;
    ts.d_trans2 = scratch.keep(d_tab);
    ts.d_pstrans = scratch.keep(d_pstates);
    ts.pstrans_records = d_pstates ? pair_state_records(ts.prefix_records, S, G, pnq) : 0;
    ts.trans2_entries = entries;
    ts.trans2_state = 1;
    return BILD_OK;
}

// The switch tails of a trajectory set (tail.hip): for every switch of the transient table with a converged transient, what a
// deviation of the means in front of it does to everything behind it -- J vectors per switch, one for every frame a look that the
// ordinary tail refuses for closeness can stand at.  Behind the pair table, from the byte budget of the state tables after both of
// their levels, whole or not at all: which tables exist is a property of the set (and its declaration) alone.
// (Unlike the state tables this one changes results, by ~1e-11: its state leaves 0 only when the build is over, under the mutex, so
// that a second thread evaluating the set meanwhile waits here and then reads the same table -- never a launch without it.)
static bool build_switch_tails(const bild_model &m, const bild_trajset &ts, hipStream_t st);
int ensure_switch_tails(const bild_model &m, const bild_trajset &ts, hipStream_t st)
{
    std::lock_guard<std::mutex> lk(ts.prefix_mu);
    if (ts.stail_state != 0) return BILD_OK;
    const bool built = build_switch_tails(m, ts, st);
    ts.stail_state = built ? 1 : -1;
    return BILD_OK;
}

static bool build_switch_tails(const bild_model &m, const bild_trajset &ts, hipStream_t st)
{
    if (ts.prefix_state != 1 || ts.trans_state != 1 || ts.d_tail_g == nullptr || m.has_G || m.S < 2) return false;
    if (config().no_tail || config().no_switch_tail || ts.trans_m_max < 1) return false;
    if (ts.expected_evals >= 0 && ts.expected_evals < kExpectPairs) return false;
    const int S = m.S, NP = m.NPm[kModal];
    if (NP > kMaxNP) return false;
    // every look the ordinary tail refuses because the next switch is too close: fewer than (40 m_ref + 29) / 30 + 4 frames in
    // front of it (the most `bits` can ask for), or a segment shorter than m_ref + margin (the look is >= 24 frames into it)
    const int mm = std::min(ts.trans_m_max, kSwitchTailMaxM);
    const int J = std::max((40 * mm + 29) / 30 + 4, mm + std::max(0, config().tail_margin));
    const int64_t entries = ts.prefix_records * (S - 1);
    const size_t bytes = (size_t)entries * J * kDMax * NP * sizeof(double);
    const size_t rec_bytes = (size_t)prefix_record_doubles(NP) * sizeof(double);
    size_t budget = (size_t)std::max<int64_t>(config().states_max_bytes, 0);
    if (config().states_max_bytes < 0) budget = ts.expected_evals >= (int64_t)100000000 ? ((size_t)64 << 30) : ((size_t)4 << 30);
    const size_t levels = (size_t)(ts.d_strans ? ts.strans_records : 0) * rec_bytes + (size_t)(ts.d_pstrans ? ts.pstrans_records : 0) * rec_bytes;
    budget = budget > levels ? budget - levels : 0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    budget = std::min(budget, free_b / 3);
    if (bytes == 0 || bytes > budget || entries >= ((int64_t)1 << 31)) return false;
    std::vector<int64_t> first((size_t)ts.n_traj + 1, 0);
    for (int j = 0; j < ts.n_traj; ++j) first[(size_t)j + 1] = first[j] + (int64_t)ts.dstar_max * S * ts.descs[j].T;
    if (first.back() != ts.prefix_records) return false;
    TabScratch scratch(st);
    double *d_tab, *d_gain;
    int64_t *d_first;
    const bool ok = scratch.alloc(&d_tab, bytes) && scratch.alloc(&d_gain, (size_t)ts.prefix_records * (NP + 4) * sizeof(double)) &&
                    scratch.alloc(&d_first, first.size() * sizeof(int64_t)) &&
                    hipMemcpy(d_first, first.data(), first.size() * sizeof(int64_t), hipMemcpyHostToDevice) == hipSuccess &&
                    scratch.run([&] {
                        return hipMemsetAsync(d_tab, 0, bytes, st) == hipSuccess &&
                               launch_switch_tail(ts.d_descs, ts.n_traj, S, NP, m.d, ts.dstar_max, m.d_states[kModal], m.d_tab[kModal],
                                                  m.tab_factored ? 1 : 0, ts.d_prefix, ts.d_tail_g, ts.d_trans, d_first, first.back(), J, d_gain,
                                                  d_tab, (void *)st) == 0;
                    }, &ts.stail_build_ms);
    if (!ok) return false;
    ts.d_stail = scratch.keep(d_tab);
    ts.stail_J = J;
    ts.stail_bytes = (int64_t)bytes;
    return true;
}

} // namespace bild

extern "C" {

int bild_trajset_create(const bild_model *m, int n_traj, const int32_t *T, const double *x, const double *loc_err,
                        bild_trajset **out)
{
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!m || !T || !x || !loc_err) return fail(BILD_ERR_INVALID, "NULL argument");
    if (n_traj < 1) return fail(BILD_ERR_INVALID, "need at least one trajectory");
    const int d = m->d;
    int64_t total = 0;
    for (int j = 0; j < n_traj; ++j) {
        if (T[j] < 1) return fail(BILD_ERR_INVALID, "trajectory %d has length %d < 1", j, T[j]);
        total += T[j];
    }
    for (int64_t i = 0; i < (int64_t)n_traj * d; ++i)
        if (!(loc_err[i] >= 0.0) || !std::isfinite(loc_err[i]))
            return fail(BILD_ERR_INVALID, "localization error must be finite and >= 0");

    int rc = ensure_device(*m);
    if (rc) return rc;

    bild_trajset *ts = new (std::nothrow) bild_trajset;
    if (!ts) return fail(BILD_ERR_NOMEM, "out of memory");
    ts->model = m;
    ts->n_traj = n_traj;
    ts->d = d;
    ts->device = m->device;
    ts->descs.resize(n_traj);

    // device copy of the data: a frame with any NaN coordinate is missing (pyx:178) -> all NaN
    // layout: per trajectory T rows + kPadRows padding rows (the kernels fetch up to kPadRows frames ahead), then zeros
    std::vector<double> xd((size_t)(total + (int64_t)kPadRows * n_traj) * d + kZeroPad, 0.0);
    const double qnan = std::nan("");
    int64_t off = 0;
    auto cleanup = [&](int code) {
        if (ts->d_x) (void)hipFree(ts->d_x);
        if (ts->d_descs) (void)hipFree(ts->d_descs);
        delete ts;
        return code;
    };
    // the largest steady-state variance of the observable w.x over the states: with s2 the scale of an innovation
    double wCw_max = 0.0;
    {
        const int N = m->N;
        for (int s_ = 0; s_ < m->S; ++s_) {
            const double *C0 = m->C0.data() + (size_t)s_ * N * N;
            double q = 0.0;
            for (int i = 0; i < N; ++i)
                for (int jj = 0; jj < N; ++jj) q += m->w[i] * C0[(size_t)i * N + jj] * m->w[jj];
            wCw_max = std::max(wCw_max, q);
        }
    }
    std::vector<double> xscales((size_t)n_traj, 0.0);
    hipError_t he = hipMalloc((void **)&ts->d_x, xd.size() * sizeof(double));
    if (he != hipSuccess) return cleanup(fail(BILD_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he)));
    ts->d_zeros = ts->d_x + (size_t)(total + (int64_t)kPadRows * n_traj) * d;
    for (int j = 0; j < n_traj; ++j) {
        TrajDesc &td = ts->descs[j];
        std::memset(&td, 0, sizeof td);
        td.T = T[j];
        const int64_t doff = off + (int64_t)kPadRows * j; // device row offset: the padding rows of trajectories 0..j-1 precede
        td.x = ts->d_x + doff * d;
        int nvalid = 0;
        double xscale = 0.0;
        for (int t = 0; t < T[j]; ++t) {
            bool valid = true;
            for (int k = 0; k < d; ++k) valid &= !std::isnan(x[(off + t) * d + k]);
            for (int k = 0; k < d; ++k) {
                xd[(doff + t) * d + k] = valid ? x[(off + t) * d + k] : qnan;
                if (valid && std::isfinite(x[(off + t) * d + k])) xscale = std::max(xscale, std::fabs(x[(off + t) * d + k]));
            }
            nvalid += valid;
        }
        td.nvalid = nvalid;
        td.xscale = xscale;
        xscales[(size_t)j] = xscale;
        ts->all_valid = ts->all_valid && nvalid == T[j];
        // np.unique(err, return_inverse=True): sorted unique values (pyx:145)
        double uniq[kDStore];
        int nu = 0;
        for (int k = 0; k < d; ++k) {
            const double e = loc_err[(size_t)j * d + k];
            bool seen = false;
            for (int u = 0; u < nu; ++u) seen |= uniq[u] == e;
            if (!seen) uniq[nu++] = e;
        }
        std::sort(uniq, uniq + nu);
        // one covariance chain per distinct error; a task carries at most kDMax mean vectors, so an error shared by
        // more dimensions than that gets several chains (the covariance recursion is simply repeated)
        int nchains = 0;
        for (int u = 0; u < nu; ++u) {
            int in_chain = kDMax; // forces a new chain at the first dimension
            for (int k = 0; k < d; ++k) {
                if (loc_err[(size_t)j * d + k] != uniq[u]) continue;
                if (in_chain == kDMax) {
                    td.s2[nchains] = uniq[u] * uniq[u];
                    td.ndims[nchains] = 0;
                    ++nchains;
                    in_chain = 0;
                }
                td.dims[nchains - 1][td.ndims[nchains - 1]++] = k;
                ++in_chain;
            }
        }
        td.dstar = nchains;
        td.nuniq = nu;
        for (int u = 0; u < nchains; ++u) td.mscale[u] = std::min(xscales[(size_t)j], 6.0 * std::sqrt(td.s2[u] + wCw_max));
        nu = nchains;
        ts->dstar_max = std::max(ts->dstar_max, nu);
        for (int u = 0; u < nu; ++u) ts->means_max = std::max(ts->means_max, (int)td.ndims[u]);
        ts->Tmax = std::max(ts->Tmax, (int)T[j]);
        off += T[j];
    }
    {
        int64_t rec = 0;
        for (int j = 0; j < n_traj; ++j) {
            ts->descs[j].prefix_rec0 = rec;
            ts->descs[j].trans0 = rec * m->S; // S entries (one per new state) for every prefix record
            ts->descs[j].strans0 = rec * (m->S - 1); // S - 1 switches (one per OTHER state) for every prefix record
            ts->descs[j].pstrans0 = rec * (m->S - 1) * (m->S - 1); // ... and S - 1 second switches for each of them
            rec += (int64_t)T[j] * m->S * ts->dstar_max;
        }
        ts->strans_entries = rec * (m->S - 1);
        ts->strans_records = 0;
        ts->prefix_records = rec;
        ts->trans_entries = rec * m->S;
    }
    he = hipMemcpy(ts->d_x, xd.data(), xd.size() * sizeof(double), hipMemcpyHostToDevice);
    if (he != hipSuccess) return cleanup(fail(BILD_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(he)));
    he = hipMalloc((void **)&ts->d_descs, (size_t)n_traj * sizeof(TrajDesc));
    if (he != hipSuccess) return cleanup(fail(BILD_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(he)));
    he = hipMemcpy(ts->d_descs, ts->descs.data(), (size_t)n_traj * sizeof(TrajDesc), hipMemcpyHostToDevice);
    if (he != hipSuccess) return cleanup(fail(BILD_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(he)));
    *out = ts;
    return BILD_OK;
}

int bild_trajset_expect(bild_trajset *ts, int64_t evaluations)
{
    if (!ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (evaluations < 0) return fail(BILD_ERR_INVALID, "a negative number of expected evaluations");
    if (ts->prefix_state != 0) return fail(BILD_ERR_INVALID, "the trajectory set has been evaluated on already: declare the expected use first");
    ts->expected_evals = evaluations;
    return BILD_OK;
}

int bild_trajset_destroy(bild_trajset *ts)
{
    if (!ts) return BILD_OK;
    (void)hipDeviceSynchronize(); // (the tables go back to the cache, which hands them straight on: nothing may read them still)
    if (ts->d_x) (void)hipFree(ts->d_x);
    if (ts->d_descs) (void)hipFree(ts->d_descs);
    tab_free(ts->d_prefix);
    tab_free(ts->d_prefix_L);
    tab_free(ts->d_tail_g);
    tab_free(ts->d_trans);
    tab_free(ts->d_trans2);
    tab_free(ts->d_strans);
    tab_free(ts->d_pstrans);
    tab_free(ts->d_stail);
    delete ts;
    return BILD_OK;
}

int bild_prefix_info(const bild_trajset *ts, int64_t *bytes, double *build_ms)
{
    if (!ts) return fail(BILD_ERR_INVALID, "NULL handle");
    const bool built = ts->prefix_state == 1, trans = ts->trans_state == 1, pairs = ts->trans2_state == 1;
    if (bytes)
        *bytes = (built ? ts->prefix_records * prefix_record_doubles(ts->model->NPm[kModal]) * (int64_t)sizeof(double) : 0) +
                 (trans ? ts->trans_entries * (int64_t)sizeof(TransEntry) : 0) +
                 (pairs ? ts->trans2_entries * (int64_t)sizeof(TransEntry) : 0) +
                 (trans && ts->d_strans ? ts->strans_records * prefix_record_doubles(ts->model->NPm[kModal]) * (int64_t)sizeof(double) : 0) +
                 (pairs && ts->d_pstrans ? ts->pstrans_records * prefix_record_doubles(ts->model->NPm[kModal]) * (int64_t)sizeof(double) : 0) +
                 (ts->stail_state == 1 ? ts->stail_bytes : 0);
    if (build_ms)
        *build_ms = (built ? ts->prefix_build_ms : 0.0) + (trans ? ts->trans_build_ms : 0.0) + (pairs ? ts->trans2_build_ms : 0.0) +
                    (ts->stail_state == 1 ? ts->stail_build_ms : 0.0);
    return BILD_OK;
}

} // extern "C"
