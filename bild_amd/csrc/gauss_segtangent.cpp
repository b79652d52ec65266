// The weighted tangent jobs of an evidence gradient (gauss_segtangent.h).  Kernels: gauss_segsens.hip
// (the weighted jobs) and gauss_sens.hip (the shared factors).
#include <algorithm>
#include <cmath>
#include <limits>

#include "gauss_segtangent.h"
#include "sim_host.h"

namespace bild {

void SegTangent::stage(const bild_gauss_model *m_, int n_traj_, const int *T_, const double *x, int P_, const bild_gauss_derivs *dm_)
{
    m = m_, dm = dm_, T = T_, n_traj = n_traj_, P = P_;
    S = m->S, d = m->d, L1 = m->L + 1;

    // per (trajectory, dimension): valid frames and their values (gauss_sens.cpp)
    toff.assign(n_traj + 1, 0);
    for (int j = 0; j < n_traj; ++j) toff[j + 1] = toff[j] + T[j];
    vidx.assign((size_t)toff[n_traj] * d, 0);
    nvalid.assign((size_t)n_traj * d, 0);
    xv.assign(vidx.size(), 0.0);
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
    jobs_of.assign(n_traj, {});
    shared_n.assign((size_t)S * d, 0);
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
}

int SegTangent::upload(CallFrame &call)
{
    hipStream_t st = call.st;
    // the model and the derivative tables, the data, the sets and the shared Toeplitz tangent factors (gauss_sens.cpp)
    const int Pf = std::max(P, 1), Wf = P > 0 ? 2 : 1;
    dmsd.assign((size_t)S * d * Pf * L1, 0.0);
    for (int q = 0; q < P; ++q)
        for (int sk = 0; sk < S * d; ++sk)
            if (dm && dm->dmsd) std::copy_n(dm->dmsd + ((size_t)q * S * d + sk) * L1, L1, &dmsd[((size_t)sk * Pf + q) * L1]);
    auto dval = [&](const double *a, int q, int sk) { return (dm && a && q < P) ? a[(size_t)q * S * d + sk] : 0.0; };
    nmax_shared = 0;
    for (int v : shared_n) nmax_shared = std::max(nmax_shared, v);
    iota.resize(std::max(nmax_shared + 1, 1));
    for (size_t i = 0; i < iota.size(); ++i) iota[i] = (int32_t)i;
    shared_off.assign((size_t)S * d + 1, 0);
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
    sets.assign((size_t)n_traj * d * S, GaussSensSet{});
    for (int j = 0; j < n_traj; ++j)
        for (int k = 0; k < d; ++k)
            for (int s = 0; s < S; ++s) {
                GaussSensSet &e = sets[((size_t)j * d + k) * S + s];
                fill_set(e, s, k);
                e.vidx = d_vidx + vbase(j, k);
                e.xv = d_xv + vbase(j, k);
            }
    shared_jobs.clear();
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
    GaussSensJob *d_shared_jobs;
    BILD_TRY(call.alloc(&d_sets, sets.size()));
    BILD_TRY(call.alloc(&d_shared_jobs, shared_jobs.size()));
    HIP_TRY(hipMemcpyAsync(d_sets, sets.data(), sets.size() * sizeof(GaussSensSet), hipMemcpyHostToDevice, st));
    if (!shared_jobs.empty())
        HIP_TRY(hipMemcpyAsync(d_shared_jobs, shared_jobs.data(), shared_jobs.size() * sizeof(GaussSensJob), hipMemcpyHostToDevice, st));
    if (launch_gauss_sens_factor(d_sets, d_shared_jobs, (int)shared_jobs.size(), P > 0 ? 1 : 0, d_shared, nullptr, st))
        return fail(BILD_ERR_HIP, "launch of the shared-factor kernel failed");
    HIP_TRY(hipStreamSynchronize(st));      // the host vectors above are staged from pageable memory
    return BILD_OK;
}

int SegTangent::reserve(CallFrame &call, int chunk)
{
    // the widest chunk's jobs and factorisation scratch
    max_jobs = 0;
    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        size_t nj = 0;
        for (int j = j0; j < std::min(n_traj, j0 + chunk); ++j) nj += jobs_of[j].size();
        max_jobs = std::max(max_jobs, nj);
    }
    BILD_TRY(call.alloc(&d_jobs, max_jobs));
    BILD_TRY(call.alloc(&d_out, max_jobs * kGaussSensStride));
    h_out.assign(max_jobs * kGaussSensStride, 0.0);
    scratch_cap = 0;
    return BILD_OK;
}

int SegTangent::run(CallFrame &call, int j0, int nc, const char *skip, const double *omega, int64_t om_slot, int64_t om_tri, int ld,
                    double *exp_logl, double *grad, double *fisher)
{
    hipStream_t st = call.st;
    const int64_t fact_budget = call.budget / 8;
    const double nan = std::numeric_limits<double>::quiet_NaN();

    // the chunk's jobs: output rows in the order of jobs_of; solves first, then the factorisations, longest first
    all.clear();
    solve_ix.clear();
    fact_ix.clear();
    flat.clear();
    for (int i = 0; i < nc; ++i) {
        if (skip[i]) continue;
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
    if (launch_segsens_solve(d_sets, d_jobs, nso, P, nmax_shared, omega, d_out, st))
        return fail(BILD_ERR_HIP, "launch of the weighted solve kernel failed");
    for (int c0 = 0; c0 < nfa;) {
        const int c1 = sim_chunk_end(slot_off, c0, nfa, fact_budget);
        if (launch_segsens_factor(d_sets, d_jobs + nso + c0, c1 - c0, P, omega, d_scratch, d_out, st))
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
        if (!skip[i])
            for (size_t e = 0; e < jobs_of[jt].size(); ++e, ++row) {
                const double *o = &h_out[row * kGaussSensStride];
                el -= o[0];
                for (int a = 0; a < P; ++a) g[a] -= o[1 + a];
                for (int a = 0, f = 0; a < P; ++a)
                    for (int b = a; b < P; ++b, ++f) F[a][b] += o[1 + P + f];
            }
        if (exp_logl) exp_logl[jt] = skip[i] ? nan : el;
        for (int a = 0; a < P; ++a) {
            if (grad) grad[(size_t)jt * P + a] = skip[i] ? nan : g[a];
            if (fisher)
                for (int b = 0; b < P; ++b) fisher[((size_t)jt * P + a) * P + b] = skip[i] ? nan : (a <= b ? F[a][b] : F[b][a]);
        }
    }
    return BILD_OK;
}

} // namespace bild
