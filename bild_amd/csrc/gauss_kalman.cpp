// Per-frame moments and posterior tracks of GenericGaussianModel profiles: the C ABI bild_gauss_kalman_segments and
// bild_gauss_kalman_mixture (include/bild_amd.h), the windows of a call as de-duplicated jobs, and the chunking of the
// factorisations and of the outputs.  Kernels: gauss_kalman.hip; DESIGN.md section 16.
//
// A candidate's intervals are those of gauss_sens.cpp.  Per dimension, interval [t0, t1) of state s has the window of
// the likelihood (its valid frames from a = t0 - 1 on, a = 0 for the first interval) and the missing frames of [t0, t1)
// that the window fills: all of them for ss_order 0, those behind the window's first valid frame for ss_order 1.  A window
// is a job (trajectory, dimension, state, rank of its first valid frame, entries, centred, first missing frame, missing
// frames).  A job without missing frames has consecutive valid frames, so it runs against a leading block of the shared
// Toeplitz factor of its (state, dimension); the others factor their own covariance.  The records of all jobs stay on
// the device while the per-frame outputs are scattered from them in chunks of whole candidates.
#include <algorithm>
#include <limits>
#include <unordered_map>

#include "gauss_kalman.h"
#include "gauss_windows.h"
#include "sim_host.h"

namespace {

using namespace bild;

struct JobKey {
    int traj, dim, state, rank, n, centred, miss, nmiss;
    bool operator==(const JobKey &o) const
    {
        return traj == o.traj && dim == o.dim && state == o.state && rank == o.rank && n == o.n && centred == o.centred &&
               miss == o.miss && nmiss == o.nmiss;
    }
};

struct JobKeyHash {
    size_t operator()(const JobKey &k) const
    {
        uint64_t h = 1469598103934665603ull;
        for (int v : {k.traj, k.dim, k.state, k.rank, k.n, k.centred, k.miss, k.nmiss}) h = (h ^ (uint32_t)v) * 1099511628211ull;
        return (size_t)h;
    }
};

int64_t budget_doubles(int64_t scratch_bytes)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    return sim_scratch_bytes(scratch_bytes, free_b) / 8;
}

// One call: the candidates' windows as jobs, their records on the device, and the scatter of chunks of candidates.
struct GaussKalCall {
    const bild_gauss_model &m;
    SimBufs bufs;
    std::vector<GaussKalRef> refs;
    std::vector<int64_t> ref_off;       // per candidate: its first ref
    GaussKalSet *d_sets = nullptr;
    GaussKalRef *d_refs = nullptr;
    double *d_rec = nullptr;
    int Tout = 0;

    explicit GaussKalCall(const bild_gauss_model &m_) : m(m_) {}

    // candidates n x K1 (traj_id may be null); outputs of Tout frames.  Runs every job; waits for nothing.
    int plan(int n_traj, const int32_t *T, const double *x, int64_t n, int K1, const int32_t *seg_start, const int32_t *seg_state,
             const int32_t *traj_id, int Tout_, int64_t scratch_bytes)
    {
        HIP_TRY(hipStreamCreateWithFlags(&bufs.stream, hipStreamNonBlocking));
        Tout = Tout_;
        const int S = m.S, d = m.d, L1 = m.L + 1;
        // per (trajectory, dimension): valid frames and their values, missing frames, the rank of every frame (T + 1)
        std::vector<int64_t> toff(n_traj + 1, 0);
        for (int j = 0; j < n_traj; ++j) toff[j + 1] = toff[j] + T[j];
        std::vector<int32_t> vidx((size_t)toff[n_traj] * d), midx(vidx.size()), rank((size_t)(toff[n_traj] + n_traj) * d);
        std::vector<double> xv(vidx.size());
        auto vbase = [&](int j, int k) { return (size_t)(toff[j] * d + (int64_t)k * T[j]); };
        auto rbase = [&](int j, int k) { return (size_t)((toff[j] + j) * d + (int64_t)k * (T[j] + 1)); };
        for (int j = 0; j < n_traj; ++j)
            for (int k = 0; k < d; ++k) {
                int v = 0;
                const size_t vb = vbase(j, k), rb = rbase(j, k);
                for (int t = 0; t < T[j]; ++t) {
                    rank[rb + t] = v;
                    const double val = x[(size_t)(toff[j] + t) * d + k];
                    if (!std::isnan(val)) {
                        vidx[vb + v] = t;
                        xv[vb + v] = val;
                        ++v;
                    } else {
                        midx[vb + (t - v)] = t;
                    }
                }
                rank[rb + T[j]] = v;
            }

        // the windows of every candidate -> refs (per candidate, interval, dimension) and jobs (de-duplicated)
        std::unordered_map<JobKey, int, JobKeyHash> job_of;
        std::vector<JobKey> keys;
        std::vector<int> ref_job;
        std::unordered_map<int64_t, int> set_of;
        std::vector<int64_t> set_key;
        auto set_index = [&](int j, int k, int s) {
            const int64_t key = ((int64_t)j * d + k) * S + s;
            auto it = set_of.find(key);
            if (it == set_of.end()) {
                it = set_of.emplace(key, (int)set_key.size()).first;
                set_key.push_back(key);
            }
            return it->second;
        };
        ref_off.assign(n + 1, 0);
        for (int64_t r = 0; r < n; ++r) {
            const int j = traj_id ? traj_id[r] : 0;
            for_each_interval(seg_start + r * K1, seg_state + r * K1, K1, T[j], [&](int a, int b, int s, bool first) {
                const int t0 = first ? 0 : a + 1;
                for (int k = 0; k < d; ++k) {
                    const int o = m.order[(size_t)s * d + k];
                    const int32_t *rk = &rank[rbase(j, k)];
                    const int r0 = first ? 0 : rk[a], cnt = rk[b] - r0;
                    GaussKalRef ref{};
                    ref.cand = r;
                    ref.set = set_index(j, k, s);
                    ref.k = k;
                    ref.t0 = t0;
                    ref.t1 = b;
                    ref.t2 = b == T[j] ? Tout : b;
                    ref.rank = r0;
                    ref.n = o == 0 ? cnt : std::max(cnt - 1, 0);
                    ref.skip = (o == 0 && !first) ? 1 : 0;
                    ref.nan = (o == 0 && !first && cnt == 0) ? 1 : 0;
                    // the missing frames the window fills: from t0 (ss_order 0) or behind its first valid frame (ss_order 1)
                    int mstart = b;
                    if (o == 0) mstart = t0;
                    else if (cnt > 0) mstart = std::max(t0, vidx[vbase(j, k) + r0] + 1);
                    mstart = std::min(mstart, b);
                    ref.miss = mstart - rk[mstart];
                    const int nmiss = (b - mstart) - (rk[b] - rk[mstart]);
                    int q = -1;
                    if (!ref.nan && (nmiss > 0 || ref.n > ref.skip)) {
                        const JobKey key{j, k, s, r0, ref.n, (o == 0 && first) ? 1 : 0, ref.miss, nmiss};
                        auto it = job_of.find(key);
                        if (it == job_of.end()) {
                            it = job_of.emplace(key, (int)keys.size()).first;
                            keys.push_back(key);
                        }
                        q = it->second;
                    }
                    refs.push_back(ref);
                    ref_job.push_back(q);
                }
            });
            ref_off[r + 1] = (int64_t)refs.size();
        }
        const int njobs = (int)keys.size();

        // jobs: records one after the other; gap-free ones against the shared factors, the others factored alone
        std::vector<int64_t> rec_off(njobs + 1, 0);
        for (int q = 0; q < njobs; ++q) rec_off[q + 1] = rec_off[q] + 2 * (int64_t)(keys[q].n + keys[q].nmiss);
        for (size_t e = 0; e < refs.size(); ++e) refs[e].rec = ref_job[e] >= 0 ? rec_off[ref_job[e]] : -1;
        std::vector<int> shared_n((size_t)S * d, 0);
        std::vector<GaussKalJob> solve, fact;
        for (int q = 0; q < njobs; ++q) {
            const JobKey &kk = keys[q];
            const int o = m.order[(size_t)kk.state * d + kk.dim];
            const int32_t *u = &vidx[vbase(kk.traj, kk.dim)] + kk.rank;
            const int last = o == 0 ? kk.n - 1 : kk.n;
            const GaussKalJob job{set_index(kk.traj, kk.dim, kk.state), kk.rank, kk.n, kk.centred, kk.miss, kk.nmiss, 0, rec_off[q]};
            if (kk.nmiss == 0 && kk.n > 0 && u[last] - u[0] == last) {
                int &sn = shared_n[(size_t)kk.state * d + kk.dim];
                sn = std::max(sn, kk.n);
                solve.push_back(job);
            } else {
                fact.push_back(job);
            }
        }

        double *d_msd, *d_xv;
        int32_t *d_vidx, *d_midx, *d_rank, *d_iota;
        BILD_TRY(bufs.put(&d_msd, m.msd.data(), m.msd.size()));
        BILD_TRY(bufs.put(&d_vidx, vidx.data(), vidx.size()));
        BILD_TRY(bufs.put(&d_midx, midx.data(), midx.size()));
        BILD_TRY(bufs.put(&d_rank, rank.data(), rank.size()));
        BILD_TRY(bufs.put(&d_xv, xv.data(), xv.size()));
        int nmax_shared = 0;
        for (int v : shared_n) nmax_shared = std::max(nmax_shared, v);
        std::vector<int32_t> iota(std::max(nmax_shared + 1, 1));
        for (size_t i = 0; i < iota.size(); ++i) iota[i] = (int32_t)i;
        BILD_TRY(bufs.put(&d_iota, iota.data(), iota.size()));
        std::vector<int64_t> shared_off((size_t)S * d + 1, 0);
        for (int sk = 0; sk < S * d; ++sk) shared_off[sk + 1] = shared_off[sk] + (int64_t)shared_n[sk] * shared_n[sk];
        double *d_shared;
        BILD_TRY(bufs.put(&d_shared, nullptr, (size_t)shared_off[S * d]));

        std::vector<GaussKalSet> sets(set_key.size());
        for (size_t e = 0; e < set_key.size(); ++e) {
            const int64_t key = set_key[e];
            const int s = (int)(key % S), k = (int)((key / S) % d), j = (int)(key / S / d);
            const int sk = s * d + k;
            GaussKalSet &g = sets[e];
            g.vidx = d_vidx + vbase(j, k);
            g.midx = d_midx + vbase(j, k);
            g.rank = d_rank + rbase(j, k);
            g.xv = d_xv + vbase(j, k);
            g.msd = d_msd + (size_t)sk * L1;
            g.msd_inf = m.msd_inf[sk];
            g.mean = m.mean[sk];
            g.fac = d_shared + shared_off[sk];
            g.fac_ld = shared_n[sk];
            g.order = m.order[sk];
        }
        // the shared factors: gauss_sens_factor_kernel at P = 0, one workgroup per (state, dimension)
        std::vector<GaussSensSet> ssets;
        std::vector<GaussSensJob> sjobs;
        for (int sk = 0; sk < S * d; ++sk) {
            if (shared_n[sk] == 0) continue;
            GaussSensSet e{};
            e.vidx = d_iota;
            e.msd = d_msd + (size_t)sk * L1;
            e.dmsd = e.msd;
            e.dmsd_ld = L1;
            e.msd_inf = m.msd_inf[sk];
            e.mean = m.mean[sk];
            e.order = m.order[sk];
            sjobs.push_back(GaussSensJob{(int)ssets.size(), 0, shared_n[sk], 0, 0, -1, shared_off[sk]});
            ssets.push_back(e);
        }
        GaussSensSet *d_ssets;
        GaussSensJob *d_sjobs;
        BILD_TRY(bufs.put(&d_ssets, ssets.data(), ssets.size()));
        BILD_TRY(bufs.put(&d_sjobs, sjobs.data(), sjobs.size()));
        BILD_TRY(bufs.put(&d_sets, sets.data(), sets.size()));
        BILD_TRY(bufs.put(&d_refs, refs.data(), refs.size()));
        BILD_TRY(bufs.put(&d_rec, nullptr, (size_t)rec_off[njobs]));
        // longest first, so that the long factorisations start early
        std::stable_sort(fact.begin(), fact.end(), [](const GaussKalJob &a, const GaussKalJob &b) { return a.n > b.n; });
        std::vector<GaussKalJob> all(solve);
        all.insert(all.end(), fact.begin(), fact.end());
        GaussKalJob *d_jobs;
        BILD_TRY(bufs.put(&d_jobs, all.data(), all.size()));
        const int nso = (int)solve.size(), nfa = (int)fact.size();
        if (launch_gauss_sens_factor(d_ssets, d_sjobs, (int)sjobs.size(), 0, d_shared, nullptr, bufs.stream))
            return fail(BILD_ERR_HIP, "launch of the shared-factor kernel failed");
        if (launch_gauss_kal_solve(d_sets, d_jobs, nso, nmax_shared, d_rec, bufs.stream))
            return fail(BILD_ERR_HIP, "launch of the gap-free solve kernel failed");
        // the factorisations: chunks of jobs whose scratch slots ((n + nmiss + 1) n doubles) fit the budget
        if (nfa > 0) {
            std::vector<int64_t> slot_off(nfa + 1, 0);
            for (int q = 0; q < nfa; ++q) slot_off[q + 1] = slot_off[q] + (int64_t)(fact[q].n + fact[q].nmiss + 1) * fact[q].n;
            const int64_t budget = budget_doubles(scratch_bytes);
            int64_t widest = 0;
            for (int c0 = 0; c0 < nfa;) {
                const int c1 = sim_chunk_end(slot_off, c0, nfa, budget);
                widest = std::max(widest, slot_off[c1] - slot_off[c0]);
                c0 = c1;
            }
            double *d_scratch;
            BILD_TRY(bufs.put(&d_scratch, nullptr, (size_t)widest));
            for (int c0 = 0; c0 < nfa;) {
                const int c1 = sim_chunk_end(slot_off, c0, nfa, budget);
                for (int q = c0; q < c1; ++q) all[nso + q].fac = slot_off[q] - slot_off[c0];
                HIP_TRY(hipMemcpyAsync(d_jobs + nso + c0, &all[nso + c0], (size_t)(c1 - c0) * sizeof(GaussKalJob), hipMemcpyHostToDevice,
                                       bufs.stream));
                if (launch_gauss_kal_factor(d_sets, d_jobs + nso + c0, c1 - c0, d_scratch, d_rec, bufs.stream))
                    return fail(BILD_ERR_HIP, "launch of the window factorisation kernel failed");
                c0 = c1;
            }
        }
        // (the staging vectors go out of scope: the copies must have finished)
        HIP_TRY(hipStreamSynchronize(bufs.stream));
        return BILD_OK;
    }

    // the outputs of candidates [c0, c1) into out (device, row c0 first; null entries not wanted)
    int scatter(int64_t c0, int64_t c1, double *const out[kKalOutputs])
    {
        GaussKalScatter p{};
        p.sets = d_sets;
        p.refs = d_refs + ref_off[c0];
        p.rec = d_rec;
        for (int w = 0; w < kKalOutputs; ++w) p.out[w] = out[w];
        p.c0 = c0;
        p.nrefs = (int)(ref_off[c1] - ref_off[c0]);
        p.Tout = Tout;
        p.d = m.d;
        if (launch_gauss_kal_scatter(p, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the scatter kernel failed");
        return BILD_OK;
    }
};

} // namespace

extern "C" int bild_gauss_kalman_segments(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, int64_t n, int K1,
                                          const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id,
                                          const bild_kalman_out *out, int64_t scratch_bytes)
{
    int rc = gauss_check_args(m, n_traj, T, x, n, K1, seg_start, seg_state, traj_id, 0, nullptr);
    if (rc) return rc;
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (out->filt_mean || out->filt_var)
        return fail(BILD_ERR_INVALID, "GenericGaussianModel has no filtered moments: filt_mean and filt_var must be NULL");
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    for (int64_t r = 0; r < n; ++r)
        if (out->T_max < T[traj_id ? traj_id[r] : 0])
            return fail(BILD_ERR_INVALID, "T_max = %d is shorter than trajectory %d (%d frames)", out->T_max, traj_id ? traj_id[r] : 0,
                        T[traj_id ? traj_id[r] : 0]);
    double *const host_out[kKalOutputs] = {out->terms, out->pred_mean, out->pred_var, nullptr, nullptr, out->smooth_mean, out->smooth_var, out->innov};
    int nout = 0;
    for (double *o : host_out) nout += o != nullptr;
    if (n == 0 || nout == 0) return BILD_OK;

    GaussKalCall call(*m);
    BILD_TRY(call.plan(n_traj, T, x, n, K1, seg_start, seg_state, traj_id, out->T_max, scratch_bytes));
    // chunks of whole candidates whose outputs fit the budget, at least one candidate
    const int64_t row = (int64_t)out->T_max * m->d;
    const int64_t per = std::max<int64_t>(1, budget_doubles(scratch_bytes) / std::max<int64_t>(1, nout * row));
    const int64_t cmax = std::min<int64_t>(n, per);
    double *d_out[kKalOutputs] = {};
    for (int w = 0; w < kKalOutputs; ++w)
        if (host_out[w]) BILD_TRY(call.bufs.put(&d_out[w], nullptr, (size_t)(cmax * row)));
    for (int64_t c0 = 0; c0 < n; c0 += cmax) {
        const int64_t c1 = std::min(n, c0 + cmax);
        BILD_TRY(call.scatter(c0, c1, d_out));
        for (int w = 0; w < kKalOutputs; ++w)
            if (host_out[w])
                HIP_TRY(hipMemcpyAsync(host_out[w] + c0 * row, d_out[w], (size_t)((c1 - c0) * row) * 8, hipMemcpyDeviceToHost, call.bufs.stream));
        HIP_TRY(hipStreamSynchronize(call.bufs.stream));
    }
    return BILD_OK;
}

extern "C" int bild_gauss_kalman_mixture(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, int64_t n, int K1,
                                         const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id,
                                         const double *log_weights, double *mean, double *var, int64_t scratch_bytes)
{
    int rc = gauss_check_args(m, n_traj, T, x, n, K1, seg_start, seg_state, traj_id, 0, nullptr);
    if (rc) return rc;
    if (!mean || !var || (n > 0 && !log_weights)) return fail(BILD_ERR_INVALID, "NULL buffer");
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    for (int64_t r = 0; r < n; ++r)
        if (std::isnan(log_weights[r]) || log_weights[r] == INFINITY)
            return fail(BILD_ERR_INVALID, "log_weights[%lld] = %g: log-weights must be finite or -inf", (long long)r, log_weights[r]);
    const int nt = n_traj, d = m->d;
    int Tout = 0;
    for (int j = 0; j < nt; ++j) Tout = std::max(Tout, T[j]);
    const int64_t row = (int64_t)Tout * d;
    // per trajectory: the largest log-weight and the first candidate that has it (the reference track)
    std::vector<double> lmax((size_t)nt, -INFINITY);
    std::vector<int64_t> best((size_t)nt, -1);
    for (int64_t r = 0; r < n; ++r) {
        const int j = traj_id ? traj_id[r] : 0;
        if (log_weights[r] > lmax[j]) {
            lmax[j] = log_weights[r];
            best[j] = r;
        }
    }
    // the candidates that carry weight, trajectory by trajectory in index order, cut into blocks of kKalBlock
    std::vector<std::vector<int64_t>> per((size_t)nt);
    for (int64_t r = 0; r < n; ++r) {
        const int j = traj_id ? traj_id[r] : 0;
        if (best[j] >= 0 && std::exp(log_weights[r] - lmax[j]) > 0.0) per[j].push_back(r);
    }
    std::vector<int64_t> order;
    std::vector<double> wts, W((size_t)nt, 0.0);
    std::vector<int32_t> blk_start{0}, blk_traj, blk_T, ref_row((size_t)nt, 0), ref_tid;
    std::vector<int64_t> ref_cand;
    for (int j = 0; j < nt; ++j) {
        if (per[j].empty()) continue;
        ref_row[j] = (int32_t)ref_cand.size();
        ref_cand.push_back(best[j]);
        ref_tid.push_back(j);
        for (size_t q = 0; q < per[j].size(); ++q) {
            const int64_t r = per[j][q];
            order.push_back(r);
            const double w = std::exp(log_weights[r] - lmax[j]);
            wts.push_back(w);
            W[j] += w;
            if ((q + 1) % kKalBlock == 0 || q + 1 == per[j].size()) {
                blk_start.push_back((int32_t)order.size());
                blk_traj.push_back(j);
                blk_T.push_back(T[j]);
            }
        }
    }
    for (int64_t i = 0; i < (int64_t)nt * row; ++i) mean[i] = var[i] = std::nan("");
    if (order.empty()) return BILD_OK;
    const int64_t nsel = (int64_t)order.size(), nref = (int64_t)ref_cand.size();
    const int nblk = (int)blk_traj.size();
    // gathered segment lists: the reference candidates, then the weighted candidates in block order
    std::vector<int32_t> g_start((size_t)(nref + nsel) * K1), g_state(g_start.size()), g_tid((size_t)(nref + nsel));
    auto gather = [&](int64_t dst, int64_t r, int j) {
        std::memcpy(&g_start[(size_t)dst * K1], seg_start + r * K1, (size_t)K1 * 4);
        std::memcpy(&g_state[(size_t)dst * K1], seg_state + r * K1, (size_t)K1 * 4);
        g_tid[(size_t)dst] = j;
    };
    for (int64_t q = 0; q < nref; ++q) gather(q, ref_cand[q], ref_tid[q]);
    for (int64_t q = 0; q < nsel; ++q) gather(nref + q, order[q], traj_id ? traj_id[order[q]] : 0);

    GaussKalCall call(*m);
    BILD_TRY(call.plan(n_traj, T, x, nref + nsel, K1, g_start.data(), g_state.data(), g_tid.data(), Tout, scratch_bytes));
    // chunks of whole blocks (smoothed mean and variance of their candidates, the blocks' partial sums), at least one block
    const int64_t budget = budget_doubles(scratch_bytes);
    std::vector<int> bcut{0};
    int64_t cand_max = 0, blk_max = 0;
    {
        int64_t acc = 0;
        for (int b = 0; b < nblk; ++b) {
            const int64_t need = (int64_t)(blk_start[b + 1] - blk_start[b]) * 2 * row + 3 * row;
            if (b > bcut.back() && acc + need > budget) {
                bcut.push_back(b);
                acc = 0;
            }
            acc += need;
            cand_max = std::max<int64_t>(cand_max, blk_start[b + 1] - blk_start[bcut.back()]);
            blk_max = std::max<int64_t>(blk_max, b + 1 - bcut.back());
        }
        bcut.push_back(nblk);
    }
    int32_t *d_ref_row, *d_blk_traj, *d_blk_T, *d_run_b0, *d_lstart;
    double *d_ref, *d_w, *d_mean, *d_var, *d_part, *d_acc;
    BILD_TRY(call.bufs.put(&d_ref_row, ref_row.data(), ref_row.size()));
    BILD_TRY(call.bufs.put(&d_w, wts.data(), wts.size()));
    BILD_TRY(call.bufs.put(&d_blk_traj, blk_traj.data(), blk_traj.size()));
    BILD_TRY(call.bufs.put(&d_blk_T, blk_T.data(), blk_T.size()));
    BILD_TRY(call.bufs.put(&d_run_b0, nullptr, (size_t)blk_max + 1));
    BILD_TRY(call.bufs.put(&d_lstart, nullptr, (size_t)blk_max + 1));
    BILD_TRY(call.bufs.put(&d_ref, nullptr, (size_t)(nref * row)));
    BILD_TRY(call.bufs.put(&d_mean, nullptr, (size_t)(cand_max * row)));
    BILD_TRY(call.bufs.put(&d_var, nullptr, (size_t)(cand_max * row)));
    BILD_TRY(call.bufs.put(&d_part, nullptr, (size_t)(blk_max * row * 3)));
    BILD_TRY(call.bufs.put(&d_acc, nullptr, (size_t)(nt * row * 3)));
    HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)(nt * row * 3) * 8, call.bufs.stream));
    {
        double *o[kKalOutputs] = {};
        o[5] = d_ref;
        BILD_TRY(call.scatter(0, nref, o));
    }
    std::vector<int32_t> run_b0, lstart;
    for (size_t c = 0; c + 1 < bcut.size(); ++c) {
        const int b0 = bcut[c], b1 = bcut[c + 1];
        double *o[kKalOutputs] = {};
        o[5] = d_mean;
        o[6] = d_var;
        BILD_TRY(call.scatter(nref + blk_start[b0], nref + blk_start[b1], o));
        run_b0.clear();
        for (int b = b0; b < b1; ++b)
            if (b == b0 || blk_traj[b] != blk_traj[b - 1]) run_b0.push_back(b - b0);
        run_b0.push_back(b1 - b0);
        // chunk-local block offsets
        lstart.assign(blk_start.begin() + b0, blk_start.begin() + b1 + 1);
        for (int32_t &v : lstart) v -= blk_start[b0];
        HIP_TRY(hipMemcpyAsync(d_lstart, lstart.data(), lstart.size() * 4, hipMemcpyHostToDevice, call.bufs.stream));
        HIP_TRY(hipMemcpyAsync(d_run_b0, run_b0.data(), run_b0.size() * 4, hipMemcpyHostToDevice, call.bufs.stream));
        MixParams mp{};
        mp.mean = d_mean;
        mp.var = d_var;
        mp.ref = d_ref;
        mp.ref_row = d_ref_row;
        mp.w = d_w + blk_start[b0];
        mp.blk_start = d_lstart;
        mp.blk_traj = d_blk_traj + b0;
        mp.blk_T = d_blk_T + b0;
        mp.nblk = b1 - b0;
        mp.Tout = Tout;
        mp.d = d;
        mp.part = d_part;
        mp.run_b0 = d_run_b0;
        mp.nrun = (int)run_b0.size() - 1;
        mp.acc = d_acc;
        if (launch_kalman_mix(mp, call.bufs.stream)) return fail(BILD_ERR_HIP, "launch of the mixture kernels failed");
        HIP_TRY(hipStreamSynchronize(call.bufs.stream));
    }
    std::vector<double> acc((size_t)(nt * row * 3)), ref((size_t)(nref * row));
    HIP_TRY(hipMemcpyAsync(acc.data(), d_acc, acc.size() * 8, hipMemcpyDeviceToHost, call.bufs.stream));
    HIP_TRY(hipMemcpyAsync(ref.data(), d_ref, ref.size() * 8, hipMemcpyDeviceToHost, call.bufs.stream));
    HIP_TRY(hipStreamSynchronize(call.bufs.stream));
    // law of total variance around the reference track: mean = ref + s1 / W, var = s2 / W + s3 / W - (s1 / W)^2
    for (int j = 0; j < nt; ++j) {
        if (per[j].empty()) continue;
        for (int64_t tk = 0; tk < (int64_t)T[j] * d; ++tk) {
            const double *a = &acc[(size_t)((j * row + tk) * 3)];
            const double s1 = a[0] / W[j];
            mean[j * row + tk] = ref[(size_t)(ref_row[j] * row + tk)] + s1;
            var[j * row + tk] = a[1] / W[j] + (a[2] / W[j] - s1 * s1);
        }
    }
    return BILD_OK;
}
