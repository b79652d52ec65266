// Gradient of the exact evidence of GenericGaussianModel (include/bild_amd.h, "evidence sensitivities"; DESIGN.md section
// 20): the refusals, the chunks of whole trajectories, the segment recursion's launches and its formulas on the last column
// of the forward table (gauss_segdp.h: the functions gauss_segdp.cpp calls, so that logev is the same number), the weight
// table and the weighted tangent jobs.  Kernels: gauss_segsens.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_call.h"
#include "gauss_segsens.h"
#include "gauss_windows.h"
#include "sim_host.h"

extern "C" int bild_gauss_segment_sensitivities(const bild_gauss_model *m, const bild_gauss_trajset *ts, const double *x, int k_max,
                                                const uint8_t *transitions, unsigned flags, const double *log_k_prior, int P,
                                                const bild_gauss_derivs *dm, int64_t scratch_bytes, bild_segsens_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    const int S = m->S, d = m->d, L1 = m->L + 1;
    // (nothing here is padded to a T_max, so no trajectory is too long for it)
    BILD_TRY(segdp_check_call(S, k_max, flags, transitions, scratch_bytes, n_traj, T, std::numeric_limits<int>::max()));
    if (n_traj == 0) return BILD_OK;
    BILD_TRY(gauss_check_args(m, n_traj, T, x, 0, 1, nullptr, nullptr, nullptr, P, dm));
    const int K = k_max + 1;
    if (log_k_prior)
        for (int j = 0; j < n_traj; ++j) {
            bool any = false;
            for (int k = 0; k < K; ++k) {
                const double v = log_k_prior[(size_t)j * K + k];
                if (std::isnan(v) || v == std::numeric_limits<double>::infinity())
                    return fail(BILD_ERR_INVALID, "log_k_prior[%d][%d] is NaN or +inf", j, k);
                any = any || v > -std::numeric_limits<double>::infinity();
            }
            if (!any) return fail(BILD_ERR_INVALID, "log_k_prior of trajectory %d is -inf everywhere", j);
        }
    int Tm = 1;
    for (int j = 0; j < n_traj; ++j) Tm = std::max(Tm, T[j]);
    const bool omit = (flags & BILD_SEGDP_NAN_OMIT) != 0;
    const int ld = Tm + 1;
    const int64_t slot = (int64_t)K * S * ld, om_tri = gauss_w_per_state(Tm), om_slot = (int64_t)S * (om_tri + ld);

    // per (trajectory, dimension): valid frames and their values (gauss_sens.cpp)
    std::vector<int64_t> toff(n_traj + 1, 0);
    for (int j = 0; j < n_traj; ++j) toff[j + 1] = toff[j] + T[j];
    std::vector<int32_t> vidx((size_t)toff[n_traj] * d), nvalid((size_t)n_traj * d);
    std::vector<double> xv(vidx.size());
    auto vbase = [&](int j, int k) { return (size_t)(toff[j] * d + (int64_t)k * T[j]); };
    for (int j = 0; j < n_traj; ++j)
        for (int k = 0; k < d; ++k) {
            int v = 0;
            const size_t vb = vbase(j, k);
            for (int t = 0; t < T[j]; ++t) {
                const double val = x[(size_t)(toff[j] + t) * d + k];
                if (!std::isnan(val)) {
                    vidx[vb + v] = t;
                    xv[vb + v] = val;
                    ++v;
                }
            }
            nvalid[(size_t)j * d + k] = v;
        }

    // the jobs of every trajectory in the order their sums are added: state, dimension, the first interval, starts ascending.
    // Set (trajectory, dimension, state) = (j d + k) S + s; the shared-factor sets follow.
    struct HostJob {
        SegsensJob job;
        int state;
        bool gap_free;
    };
    std::vector<std::vector<HostJob>> jobs_of(n_traj);
    std::vector<int> shared_n((size_t)S * d, 0);
    for (int j = 0; j < n_traj; ++j)
        for (int s = 0; s < S; ++s)
            for (int k = 0; k < d; ++k) {
                const int o = m->order[(size_t)s * d + k], V = nvalid[(size_t)j * d + k];
                const int32_t *u = &vidx[vbase(j, k)];
                auto add = [&](int r, bool first) {
                    const int cnt = V - r, n = o == 0 ? cnt : cnt - 1, skip = (o == 0 && !first) ? 1 : 0;
                    if (n <= skip) return;
                    int a_lo = 0, a_hi = 0;
                    if (!first) {
                        a_lo = (r > 0 ? u[r - 1] + 1 : 0) + 1;
                        a_hi = std::min(u[r] + 1, T[j] - 1);
                        if (a_lo > a_hi) return;
                    }
                    const int last = o == 0 ? n - 1 : n;    // index of the job's last frame among u + r
                    HostJob h{};
                    h.job.j = GaussSensJob{(j * d + k) * S + s, r, n, skip, (o == 0 && first) ? 1 : 0, 0, 0};
                    h.job.T = T[j];
                    h.job.a_lo = a_lo;
                    h.job.a_hi = a_hi;
                    h.job.first = first ? 1 : 0;
                    h.state = s;
                    h.gap_free = u[r + last] - u[r] == last;
                    if (h.gap_free) shared_n[(size_t)s * d + k] = std::max(shared_n[(size_t)s * d + k], n);
                    jobs_of[j].push_back(h);
                };
                add(0, true);
                for (int r = 0; r < V; ++r) add(r, false);
            }

    CallFrame call;
    BILD_TRY(call.open(m, ts));
    hipStream_t st = call.st;

    // a trajectory's share of the chunk: the recursion's tables and the weight table
    const int64_t per_traj = slot * (2 * (5 * 8 + 4) + 4 * 8) + om_slot * 8 + (int64_t)K * K * 8 + (int64_t)K * S * 40 + (int64_t)K * 16;
    int chunk = 0;
    BILD_TRY(call.chunk_of(per_traj, scratch_bytes, n_traj, &chunk));

    SegdpParams p{};
    SegsensWeights w{};
    uint8_t *d_tr = nullptr;
    double *d_coef = nullptr, *d_top = nullptr;
    BILD_TRY(call.alloc(&d_tr, (size_t)S * S));
    BILD_TRY(alloc_fwd(call, &p.A, (size_t)chunk * slot));
    BILD_TRY(alloc_fwd(call, &p.alpha, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.map_seg_start, (size_t)chunk * K * K));
    BILD_TRY(call.alloc(&p.map_seg_state, (size_t)chunk * K * K));
    BILD_TRY(call.alloc(&p.fin, (size_t)chunk * K * S * 5));
    BILD_TRY(call.alloc(&p.beta.M, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.beta.Z, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.gamma.M, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&p.gamma.Z, (size_t)chunk * slot));
    BILD_TRY(call.alloc(&w.omega, (size_t)chunk * om_slot));
    BILD_TRY(call.alloc(&d_coef, (size_t)chunk * K));
    BILD_TRY(call.alloc(&d_top, (size_t)chunk * K));
    HIP_TRY(hipMemcpyAsync(d_tr, transitions, (size_t)S * S, hipMemcpyHostToDevice, st));
    p.tr = d_tr;
    p.slot = slot;
    p.S = S;
    p.K = K;
    p.Tm = Tm;
    p.ld = ld;
    p.ntile = (Tm + kSegdpTile - 1) / kSegdpTile;
    w.coef = d_coef;
    w.top = d_top;
    w.om_slot = om_slot;
    w.om_tri = om_tri;

    // the model and the derivative tables, the data, the sets and the shared Toeplitz tangent factors (gauss_sens.cpp)
    const int Pf = std::max(P, 1), Wf = P > 0 ? 2 : 1;
    std::vector<double> dmsd((size_t)S * d * Pf * L1, 0.0);
    for (int q = 0; q < P; ++q)
        for (int sk = 0; sk < S * d; ++sk)
            if (dm && dm->dmsd) std::copy_n(dm->dmsd + ((size_t)q * S * d + sk) * L1, L1, &dmsd[((size_t)sk * Pf + q) * L1]);
    auto dval = [&](const double *a, int q, int sk) { return (dm && a && q < P) ? a[(size_t)q * S * d + sk] : 0.0; };
    int nmax_shared = 0;
    for (int v : shared_n) nmax_shared = std::max(nmax_shared, v);
    std::vector<int32_t> iota(std::max(nmax_shared + 1, 1));
    for (size_t i = 0; i < iota.size(); ++i) iota[i] = (int32_t)i;
    std::vector<int64_t> shared_off((size_t)S * d + 1, 0);
    for (int sk = 0; sk < S * d; ++sk) shared_off[sk + 1] = shared_off[sk] + (int64_t)Pf * Wf * shared_n[sk] * shared_n[sk];
    double *d_msd, *d_dmsd, *d_xv, *d_shared;
    int32_t *d_vidx, *d_iota;
    BILD_TRY(call.alloc(&d_msd, m->msd.size()));
    BILD_TRY(call.alloc(&d_dmsd, dmsd.size()));
    BILD_TRY(call.alloc(&d_vidx, vidx.size()));
    BILD_TRY(call.alloc(&d_xv, xv.size()));
    BILD_TRY(call.alloc(&d_iota, iota.size()));
    BILD_TRY(call.alloc(&d_shared, (size_t)shared_off[S * d]));
    HIP_TRY(hipMemcpyAsync(d_msd, m->msd.data(), m->msd.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_dmsd, dmsd.data(), dmsd.size() * 8, hipMemcpyHostToDevice, st));
    if (!vidx.empty()) {
        HIP_TRY(hipMemcpyAsync(d_vidx, vidx.data(), vidx.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_xv, xv.data(), xv.size() * 8, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_iota, iota.data(), iota.size() * 4, hipMemcpyHostToDevice, st));
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
    std::vector<GaussSensSet> sets((size_t)n_traj * d * S);
    for (int j = 0; j < n_traj; ++j)
        for (int k = 0; k < d; ++k)
            for (int s = 0; s < S; ++s) {
                GaussSensSet &e = sets[((size_t)j * d + k) * S + s];
                fill_set(e, s, k);
                e.vidx = d_vidx + vbase(j, k);
                e.xv = d_xv + vbase(j, k);
            }
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
                shared_jobs.push_back(GaussSensJob{(int)sets.size(), 0, nn, 0, 0, -1, shared_off[sk] + (int64_t)q * Wf * nn * nn});
                sets.push_back(e);
            }
        }
    GaussSensSet *d_sets;
    GaussSensJob *d_shared_jobs;
    BILD_TRY(call.alloc(&d_sets, sets.size()));
    BILD_TRY(call.alloc(&d_shared_jobs, shared_jobs.size()));
    HIP_TRY(hipMemcpyAsync(d_sets, sets.data(), sets.size() * sizeof(GaussSensSet), hipMemcpyHostToDevice, st));
    if (!shared_jobs.empty())
        HIP_TRY(hipMemcpyAsync(d_shared_jobs, shared_jobs.data(), shared_jobs.size() * sizeof(GaussSensJob), hipMemcpyHostToDevice, st));
    if (launch_gauss_sens_factor(d_sets, d_shared_jobs, (int)shared_jobs.size(), P > 0 ? 1 : 0, d_shared, nullptr, st))
        return fail(BILD_ERR_HIP, "launch of the shared-factor kernel failed");
    HIP_TRY(hipStreamSynchronize(st));      // the host vectors above are staged from pageable memory

    // the widest chunk's jobs and factorisation scratch
    size_t max_jobs = 0;
    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        size_t nj = 0;
        for (int j = j0; j < std::min(n_traj, j0 + chunk); ++j) nj += jobs_of[j].size();
        max_jobs = std::max(max_jobs, nj);
    }
    SegsensJob *d_jobs;
    double *d_out, *d_scratch = nullptr;
    BILD_TRY(call.alloc(&d_jobs, max_jobs));
    BILD_TRY(call.alloc(&d_out, max_jobs * kGaussSensStride));
    int64_t scratch_cap = 0;
    const int64_t fact_budget = call.budget / 8;

    const std::vector<long double> ntraces = trace_counts(S, transitions, K);
    std::vector<double> fin((size_t)chunk * K * S * 5), coef((size_t)chunk * K), top((size_t)chunk * K), h_out(max_jobs * kGaussSensStride);
    std::vector<char> is_nan(chunk);
    std::vector<SegsensJob> all;
    std::vector<int> solve_ix, fact_ix;
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();

    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        const int nc = std::min(chunk, n_traj - j0);
        p.trajs = call.d_trajs + j0;
        p.n_traj = nc;
        BILD_TRY(segdp_run_forward(p, k_max, st));
        BILD_TRY(segdp_run_backward(p, k_max, st));
        HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * K * S * 5 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        // logev of every k (segdp_evidence), the posterior over k, and the scale of every k's weights
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = T[jt];
            std::vector<double> logev(K), zk(K), lw(K);
            bool bad_traj = false;
            double lmax = ninf;
            for (int k = 0; k < K; ++k) {
                const SegdpEvidence e =
                    segdp_evidence(fin.data() + ((size_t)i * K + k) * S * 5, S, binom_ld(Tj - 1, k) * ntraces[k], omit);
                const double le = e.logev;
                logev[k] = le;
                zk[k] = e.z;
                top[(size_t)i * K + k] = e.top;
                const double lp = log_k_prior ? log_k_prior[(size_t)jt * K + k] : 0.0;
                lw[k] = lp > ninf ? lp + le : ninf;     // a k of prior weight 0 does not count, NaN or not
                if (std::isnan(lw[k])) bad_traj = true;
                else lmax = std::max(lmax, lw[k]);
                if (out->logev) out->logev[(size_t)jt * K + k] = le;
            }
            // pi normalised over k: log sum_k pi_k ev_k = lmax + log sum exp(lw - lmax) - log sum exp(log_k_prior)
            double tot = 0.0, lpmax = ninf, ptot = 0.0;
            for (int k = 0; k < K; ++k) lpmax = std::max(lpmax, log_k_prior ? log_k_prior[(size_t)jt * K + k] : 0.0);
            for (int k = 0; k < K; ++k) ptot += std::exp((log_k_prior ? log_k_prior[(size_t)jt * K + k] : 0.0) - lpmax);
            const bool dead = !bad_traj && lmax == ninf;    // no k of positive prior weight has a profile of positive weight
            if (!bad_traj && !dead)
                for (int k = 0; k < K; ++k) tot += lw[k] > ninf ? std::exp(lw[k] - lmax) : 0.0;
            is_nan[i] = bad_traj || dead;
            for (int k = 0; k < K; ++k) {
                const double kp = bad_traj || dead ? nan : (lw[k] > ninf ? std::exp(lw[k] - lmax) / tot : 0.0);
                if (out->k_post) out->k_post[(size_t)jt * K + k] = kp;
                coef[(size_t)i * K + k] = (kp > 0.0 && zk[k] > 0.0) ? kp / zk[k] : 0.0;
            }
            if (out->log_marginal)
                out->log_marginal[jt] = bad_traj ? nan : dead ? ninf : lmax + std::log(tot) - (lpmax + std::log(ptot));
        }
        HIP_TRY(hipMemcpyAsync(d_coef, coef.data(), (size_t)nc * K * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_top, top.data(), (size_t)nc * K * 8, hipMemcpyHostToDevice, st));
        if (launch_segsens_weight(p, w, st)) return fail(BILD_ERR_HIP, "launch of the weight kernel failed");

        // the chunk's jobs: output rows in the order of jobs_of; solves first, then the factorisations, longest first
        all.clear();
        solve_ix.clear();
        fact_ix.clear();
        std::vector<SegsensJob> flat;
        for (int i = 0; i < nc; ++i) {
            if (is_nan[i]) continue;
            for (const HostJob &h : jobs_of[j0 + i]) {
                SegsensJob job = h.job;
                job.j.out = (int)flat.size();
                job.om = (int64_t)i * om_slot + (job.first ? (int64_t)S * om_tri + (int64_t)h.state * ld : (int64_t)h.state * om_tri);
                (h.gap_free ? solve_ix : fact_ix).push_back((int)flat.size());
                flat.push_back(job);
            }
        }
        std::stable_sort(fact_ix.begin(), fact_ix.end(), [&](int a, int b) { return flat[a].j.n > flat[b].j.n; });
        for (int q : solve_ix) all.push_back(flat[q]);
        const int nso = (int)solve_ix.size(), nfa = (int)fact_ix.size();
        std::vector<int64_t> slot_off(nfa + 1, 0);
        for (int q = 0; q < nfa; ++q) {
            const SegsensJob &job = flat[fact_ix[q]];
            slot_off[q + 1] = slot_off[q] + (int64_t)(job.j.n + 1) * job.j.n * (1 + P);
        }
        int64_t widest = 0;
        for (int c0 = 0; c0 < nfa;) {
            const int c1 = sim_chunk_end(slot_off, c0, nfa, fact_budget);
            for (int q = c0; q < c1; ++q) {
                SegsensJob job = flat[fact_ix[q]];
                job.j.fac = slot_off[q] - slot_off[c0];
                all.push_back(job);
            }
            widest = std::max(widest, slot_off[c1] - slot_off[c0]);
            c0 = c1;
        }
        if (widest > scratch_cap) {
            BILD_TRY(call.alloc(&d_scratch, (size_t)widest));
            scratch_cap = widest;
        }
        if (!all.empty()) HIP_TRY(hipMemcpyAsync(d_jobs, all.data(), all.size() * sizeof(SegsensJob), hipMemcpyHostToDevice, st));
        if (launch_segsens_solve(d_sets, d_jobs, nso, P, nmax_shared, w.omega, d_out, st))
            return fail(BILD_ERR_HIP, "launch of the weighted solve kernel failed");
        for (int c0 = 0; c0 < nfa;) {
            const int c1 = sim_chunk_end(slot_off, c0, nfa, fact_budget);
            if (launch_segsens_factor(d_sets, d_jobs + nso + c0, c1 - c0, P, w.omega, d_scratch, d_out, st))
                return fail(BILD_ERR_HIP, "launch of the weighted factorisation kernel failed");
            c0 = c1;
        }
        if (!flat.empty()) HIP_TRY(hipMemcpyAsync(h_out.data(), d_out, flat.size() * kGaussSensStride * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        // per trajectory: its jobs in order
        size_t row = 0;
        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i;
            double el = 0.0, g[kGaussSensMaxP] = {}, F[kGaussSensMaxP][kGaussSensMaxP] = {};
            if (!is_nan[i])
                for (size_t e = 0; e < jobs_of[jt].size(); ++e, ++row) {
                    const double *o = &h_out[row * kGaussSensStride];
                    el -= o[0];
                    for (int a = 0; a < P; ++a) g[a] -= o[1 + a];
                    for (int a = 0, f = 0; a < P; ++a)
                        for (int b = a; b < P; ++b, ++f) F[a][b] += o[1 + P + f];
                }
            if (out->exp_logl) out->exp_logl[jt] = is_nan[i] ? nan : el;
            for (int a = 0; a < P; ++a) {
                if (out->grad) out->grad[(size_t)jt * P + a] = is_nan[i] ? nan : g[a];
                if (out->fisher)
                    for (int b = 0; b < P; ++b) out->fisher[((size_t)jt * P + a) * P + b] = is_nan[i] ? nan : (a <= b ? F[a][b] : F[b][a]);
            }
        }
    }
    return BILD_OK;
}
