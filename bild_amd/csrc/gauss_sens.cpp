// Forward sensitivities of GenericGaussianModel's log-likelihood: the C ABI bild_gauss_logl_sensitivities
// (include/bild_amd.h), its checks, the windows of a call as de-duplicated jobs, and the sums per candidate.  Kernels:
// gauss_sens.hip; DESIGN.md section 15.
//
// A candidate's profile is cleaned into intervals as gauss_walk_kernel cleans it; interval i of state s covers the window
// [a, b) (a = 0 for the first interval, else its first frame - 1) and, per dimension, uses the valid frames from a on
// that lie before b.  That window is a job (trajectory, dimension, state, rank of its first valid frame, entries, centred).
// A job whose frames are consecutive (no missing frame between its first and its last) is a leading block of the
// Toeplitz covariance of its (state, dimension), so it runs against the one shared factor; the others factor their own
// covariance.  Both run only up to the window's last counted entry.
#include <algorithm>
#include <limits>
#include <unordered_map>

#include "gauss.h"
#include "gauss_windows.h"
#include "likelihood.h"
#include "sim_host.h"

namespace {

using namespace bild;

constexpr int kRefZero = -1;    // a window without counted entries
constexpr int kRefNaN = -2;     // a later ss_order-0 window without a valid frame (bild_gauss_logl_segments: NaN)

struct JobKey {
    int traj, dim, state, rank, n, centred;
    bool operator==(const JobKey &o) const
    {
        return traj == o.traj && dim == o.dim && state == o.state && rank == o.rank && n == o.n && centred == o.centred;
    }
};

struct JobKeyHash {
    size_t operator()(const JobKey &k) const
    {
        uint64_t h = 1469598103934665603ull;
        for (int v : {k.traj, k.dim, k.state, k.rank, k.n, k.centred}) h = (h ^ (uint32_t)v) * 1099511628211ull;
        return (size_t)h;
    }
};

} // namespace

extern "C" int bild_gauss_logl_sensitivities(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, int64_t n, int K1,
                                             const int32_t *seg_start, const int32_t *seg_state, const int32_t *traj_id, int P,
                                             const bild_gauss_derivs *dm, double *logl, double *grad, double *fisher,
                                             int64_t scratch_bytes)
{
    int rc = gauss_check_args(m, n_traj, T, x, n, K1, seg_start, seg_state, traj_id, P, dm);
    if (rc) return rc;
    if (n == 0 || (!logl && !grad && !fisher)) return BILD_OK;
    const int S = m->S, d = m->d, L1 = m->L + 1;

    // per (trajectory, dimension): valid frames, their values, and the rank of every frame (T + 1 entries)
    std::vector<int64_t> toff(n_traj + 1, 0);
    for (int j = 0; j < n_traj; ++j) toff[j + 1] = toff[j] + T[j];
    std::vector<int32_t> vidx((size_t)toff[n_traj] * d), rank((size_t)(toff[n_traj] + n_traj) * d);
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
                }
            }
            rank[rb + T[j]] = v;
        }

    // the windows of every candidate -> jobs (de-duplicated); refs: per candidate, interval and dimension
    std::unordered_map<JobKey, int, JobKeyHash> job_of;
    std::vector<JobKey> keys;
    std::vector<int> ref;
    std::vector<int64_t> ref_off(n + 1, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int j = traj_id ? traj_id[r] : 0;
        for_each_interval(seg_start + r * K1, seg_state + r * K1, K1, T[j], [&](int a, int b, int s, bool first) {
            for (int k = 0; k < d; ++k) {
                const int o = m->order[(size_t)s * d + k];
                const int32_t *rk = &rank[rbase(j, k)];
                const int r0 = first ? 0 : rk[a], cnt = rk[b] - r0;
                int len = o == 0 ? cnt : cnt - 1, skip = (o == 0 && !first) ? 1 : 0;
                if (o == 0 && !first && cnt == 0) {
                    ref.push_back(kRefNaN);
                    continue;
                }
                if (len <= skip) {
                    ref.push_back(kRefZero);
                    continue;
                }
                const JobKey key{j, k, s, r0, len, (o == 0 && first) ? 1 : 0};
                auto it = job_of.find(key);
                if (it == job_of.end()) {
                    it = job_of.emplace(key, (int)keys.size()).first;
                    keys.push_back(key);
                }
                ref.push_back(it->second);
            }
        });
        ref_off[r + 1] = (int64_t)ref.size();
    }
    const int njobs = (int)keys.size();

    // sets: one per (trajectory, dimension, state) that a job uses, one per (state, dimension, parameter) of a shared factor
    const int Pf = std::max(P, 1);      // shared-factor workgroups per (state, dimension)
    std::vector<GaussSensSet> sets;
    std::unordered_map<int64_t, int> set_of;
    std::vector<int> shared_n((size_t)S * d, 0);
    std::vector<GaussSensJob> solve, fact;
    for (int q = 0; q < njobs; ++q) {
        const JobKey &kk = keys[q];
        const int o = m->order[(size_t)kk.state * d + kk.dim];
        const int32_t *u = &vidx[vbase(kk.traj, kk.dim)] + kk.rank;
        const int last = o == 0 ? kk.n - 1 : kk.n;     // index of the job's last frame among u
        const bool gap_free = u[last] - u[0] == last;
        const int64_t skey = ((int64_t)kk.traj * d + kk.dim) * S + kk.state;
        auto it = set_of.find(skey);
        if (it == set_of.end()) {
            it = set_of.emplace(skey, (int)sets.size()).first;
            sets.push_back(GaussSensSet{});
        }
        GaussSensJob job{it->second, kk.rank, kk.n, (o == 0 && !kk.centred) ? 1 : 0, kk.centred, q, 0};
        if (gap_free) {
            int &sn = shared_n[(size_t)kk.state * d + kk.dim];
            sn = std::max(sn, kk.n);
            solve.push_back(job);
        } else {
            fact.push_back(job);
        }
    }

    SimBufs bufs;
    HIP_TRY(hipStreamCreateWithFlags(&bufs.stream, hipStreamNonBlocking));
    // the model and the derivative tables: msd (S d x L1), dmsd (S d x P x L1)
    std::vector<double> dmsd((size_t)S * d * Pf * L1, 0.0);
    for (int q = 0; q < P; ++q)
        for (int sk = 0; sk < S * d; ++sk)
            if (dm && dm->dmsd)
                std::copy_n(dm->dmsd + ((size_t)q * S * d + sk) * L1, L1, &dmsd[((size_t)sk * Pf + q) * L1]);
    auto dval = [&](const double *a, int q, int sk) { return (dm && a && q < P) ? a[(size_t)q * S * d + sk] : 0.0; };
    int nmax_shared = 0;
    for (int v : shared_n) nmax_shared = std::max(nmax_shared, v);
    std::vector<int32_t> iota(std::max(nmax_shared + 1, 1));
    for (size_t i = 0; i < iota.size(); ++i) iota[i] = (int32_t)i;
    double *d_msd, *d_dmsd, *d_xv;
    int32_t *d_vidx, *d_iota;
    BILD_TRY(bufs.put(&d_msd, m->msd.data(), m->msd.size()));
    BILD_TRY(bufs.put(&d_dmsd, dmsd.data(), dmsd.size()));
    BILD_TRY(bufs.put(&d_vidx, vidx.data(), vidx.size()));
    BILD_TRY(bufs.put(&d_xv, xv.data(), xv.size()));
    BILD_TRY(bufs.put(&d_iota, iota.data(), iota.size()));

    // shared factors: per (state, dimension) with gap-free jobs, P = 0: L (n^2); else Pf pairs (L, dL_q) interleaved (2 n^2)
    std::vector<int64_t> shared_off((size_t)S * d + 1, 0);
    const int W = P > 0 ? 2 : 1;
    for (int sk = 0; sk < S * d; ++sk) shared_off[sk + 1] = shared_off[sk] + (int64_t)Pf * W * shared_n[sk] * shared_n[sk];
    double *d_shared;
    BILD_TRY(bufs.put(&d_shared, nullptr, (size_t)shared_off[S * d]));
    auto fill_set = [&](GaussSensSet &e, int s, int k) {
        const int sk = s * d + k;
        e.msd = d_msd + (size_t)sk * L1;
        e.dmsd = d_dmsd + (size_t)sk * Pf * L1;
        e.dmsd_ld = L1;
        e.msd_inf = m->msd_inf[sk];
        e.mean = m->mean[sk];
        for (int q = 0; q < kGaussSensMaxP; ++q) {
            e.dmsd_inf[q] = dval(dm ? dm->dmsd_inf : nullptr, q, sk);
            e.dmean[q] = dval(dm ? dm->dmean : nullptr, q, sk);
        }
        e.order = m->order[sk];
        e.fac = d_shared + shared_off[sk];
        e.fac_ld = shared_n[sk];
    };
    for (const auto &kv : set_of) {
        const int64_t key = kv.first;
        const int s = (int)(key % S), k = (int)((key / S) % d), j = (int)(key / S / d);
        GaussSensSet &e = sets[kv.second];
        fill_set(e, s, k);
        e.vidx = d_vidx + vbase(j, k);
        e.xv = d_xv + vbase(j, k);
    }
    // the shared-factor jobs: set (state, dimension, parameter q) carries parameter q's derivatives as its only one
    std::vector<GaussSensJob> shared_jobs;
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < d; ++k) {
            const int sk = s * d + k, nn = shared_n[sk];
            if (nn == 0) continue;
            for (int q = 0; q < Pf; ++q) {
                GaussSensSet e{};
                fill_set(e, s, k);
                e.vidx = d_iota;
                e.dmsd += (size_t)q * L1;
                e.dmsd_inf[0] = e.dmsd_inf[q];
                shared_jobs.push_back(GaussSensJob{(int)sets.size(), 0, nn, 0, 0, -1, shared_off[sk] + (int64_t)q * W * nn * nn});
                sets.push_back(e);
            }
        }
    GaussSensSet *d_sets;
    GaussSensJob *d_jobs;
    double *d_out;
    BILD_TRY(bufs.put(&d_sets, sets.data(), sets.size()));
    // longest first, so that the long factorisations start early
    std::stable_sort(fact.begin(), fact.end(), [](const GaussSensJob &a, const GaussSensJob &b) { return a.n > b.n; });
    std::vector<GaussSensJob> all(shared_jobs);
    all.insert(all.end(), solve.begin(), solve.end());
    all.insert(all.end(), fact.begin(), fact.end());
    BILD_TRY(bufs.put(&d_jobs, all.data(), all.size()));
    BILD_TRY(bufs.put(&d_out, nullptr, (size_t)njobs * kGaussSensStride));
    const int nsh = (int)shared_jobs.size(), nso = (int)solve.size(), nfa = (int)fact.size();

    if (launch_gauss_sens_factor(d_sets, d_jobs, nsh, P > 0 ? 1 : 0, d_shared, d_out, bufs.stream))
        return fail(BILD_ERR_HIP, "launch of the shared-factor kernel failed");
    if (launch_gauss_sens_solve(d_sets, d_jobs + nsh, nso, P, nmax_shared, d_out, bufs.stream))
        return fail(BILD_ERR_HIP, "launch of the sensitivity solve kernel failed");
    // the factorisations with a missing frame: chunks of jobs whose scratch slots ((n + 1) n (1 + P) doubles) fit the budget
    if (nfa > 0) {
        std::vector<int64_t> slot_off(nfa + 1, 0);
        for (int q = 0; q < nfa; ++q) slot_off[q + 1] = slot_off[q] + (int64_t)(fact[q].n + 1) * fact[q].n * (1 + P);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        const int64_t budget = sim_scratch_bytes(scratch_bytes, free_b) / 8;
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
            for (int q = c0; q < c1; ++q) all[nsh + nso + q].fac = slot_off[q] - slot_off[c0];
            HIP_TRY(hipMemcpyAsync(d_jobs + nsh + nso + c0, &all[nsh + nso + c0], (size_t)(c1 - c0) * sizeof(GaussSensJob),
                                   hipMemcpyHostToDevice, bufs.stream));
            if (launch_gauss_sens_factor(d_sets, d_jobs + nsh + nso + c0, c1 - c0, P, d_scratch, d_out, bufs.stream))
                return fail(BILD_ERR_HIP, "launch of the sensitivity factorisation kernel failed");
            c0 = c1;
        }
    }
    std::vector<double> h_out((size_t)njobs * kGaussSensStride);
    if (njobs) HIP_TRY(hipMemcpyAsync(h_out.data(), d_out, h_out.size() * 8, hipMemcpyDeviceToHost, bufs.stream));
    HIP_TRY(hipStreamSynchronize(bufs.stream));

    // per candidate: intervals in order, dimensions in index order
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t r = 0; r < n; ++r) {
        double ll = 0.0, g[kGaussSensMaxP] = {}, F[kGaussSensMaxP][kGaussSensMaxP] = {};
        bool is_nan = false;
        for (int64_t e = ref_off[r]; e < ref_off[r + 1]; ++e) {
            if (ref[e] == kRefNaN) is_nan = true;
            if (ref[e] < 0) continue;
            const double *o = &h_out[(size_t)ref[e] * kGaussSensStride];
            ll -= o[0];
            for (int a = 0; a < P; ++a) g[a] -= o[1 + a];
            for (int a = 0, f = 0; a < P; ++a)
                for (int b = a; b < P; ++b, ++f) F[a][b] += o[1 + P + f];
        }
        if (logl) logl[r] = is_nan ? nan : ll;
        for (int a = 0; a < P; ++a) {
            if (grad) grad[r * P + a] = is_nan ? nan : g[a];
            if (fisher)
                for (int b = 0; b < P; ++b) fisher[(r * P + a) * P + b] = is_nan ? nan : (a <= b ? F[a][b] : F[b][a]);
        }
    }
    return BILD_OK;
}
