// The model behind a bild_model handle: invariant-subspace reduction, modal analysis and packing for the kernels (host
// side, once per model), its device residency, and what a launch takes from it.
#include <new>

#include "likelihood.h"

namespace {

bool all_finite(const double *p, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// Smallest subspace that contains w (and the mean sources M0, G) and is invariant under every
// B_s, Sig_s, C0_s.  All of these are symmetric, so the orthogonal complement is invariant as
// well and decouples exactly from the observable w.x: the filter restricted to the subspace
// gives the same likelihood.  (For the reference's default model -- free chain vs. chain with
// an end-to-end bond, end-to-end measurement -- this is the reflection-antisymmetric half of
// the modes, N/2 instead of N.)
//
// A Krylov construction is ill-conditioned here (the remainders decay smoothly, there is no
// gap to threshold on).  Instead: eigen-decompose ONE generic combination Z of all matrices;
// every common invariant subspace is spanned by eigenvectors of Z (generic Z has simple
// eigenvalues within each symmetry sector), so select the eigenvectors that overlap w and
// close the selection under the couplings  e_i^T X e_j  of every matrix X.  Overlaps and
// couplings are either O(1e-16) or macroscopic, which makes the threshold robust.
// Returns the basis as ROWS (n x N).
void invariant_subspace(const bild_model &m, Mat &rows, int &n)
{
    const int N = m.N, S = m.S;
    const double tol = 1e-11;
    std::vector<const double *> mats;
    for (int s = 0; s < S; ++s)
        for (const Mat *src : {&m.B, &m.Sig, &m.C0}) mats.push_back(src->data() + (size_t)s * N * N);
    Mat Z((size_t)N * N, 0.0);
    std::vector<double> scale(mats.size());
    for (size_t a = 0; a < mats.size(); ++a) {
        double mx = 0.0;
        for (int i = 0; i < N * N; ++i) mx = std::max(mx, std::fabs(mats[a][i]));
        scale[a] = std::max(mx, 1e-300);
        // fixed irrational-ish weights: reproducible, generic
        const double c = 0.5 + std::fmod(0.7548776662466927 * (double)(a + 1), 1.0);
        for (int i = 0; i < N * N; ++i) Z[i] += c * mats[a][i] / scale[a];
    }
    std::vector<double> ev;
    Mat E;
    la::jacobi_eigh(Z, N, ev, E); // columns
    Mat Et = la::transpose(E, N, N); // rows = eigenvectors

    std::vector<char> sel(N, 0);
    auto seed = [&](const double *v, int stride) {
        double nv = 0.0;
        for (int i = 0; i < N; ++i) nv += v[(size_t)i * stride] * v[(size_t)i * stride];
        nv = std::sqrt(nv);
        if (nv == 0.0) return;
        for (int e = 0; e < N; ++e) {
            double dot = 0.0;
            for (int i = 0; i < N; ++i) dot += Et[(size_t)e * N + i] * v[(size_t)i * stride];
            if (std::fabs(dot) > tol * nv) sel[e] = 1;
        }
    };
    seed(m.w.data(), 1);
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < m.d; ++k) {
            seed(m.M0.data() + (size_t)s * N * m.d + k, m.d);
            seed(m.G.data() + (size_t)s * N * m.d + k, m.d);
        }
    // coupling matrices in the eigenbasis of Z
    std::vector<Mat> coup(mats.size());
    for (size_t a = 0; a < mats.size(); ++a) {
        Mat X(mats[a], mats[a] + (size_t)N * N);
        coup[a] = la::matmul(la::matmul(Et, X, N, N, N), E, N, N, N);
    }
    bool grew = true;
    while (grew) {
        grew = false;
        for (size_t a = 0; a < mats.size(); ++a)
            for (int i = 0; i < N; ++i) {
                if (sel[i]) continue;
                for (int j = 0; j < N; ++j)
                    if (sel[j] && std::fabs(coup[a][(size_t)i * N + j]) > tol * scale[a]) {
                        sel[i] = 1;
                        grew = true;
                        break;
                    }
            }
    }
    rows.clear();
    n = 0;
    for (int e = 0; e < N; ++e)
        if (sel[e]) {
            rows.insert(rows.end(), Et.begin() + (size_t)e * N, Et.begin() + (size_t)(e + 1) * N);
            ++n;
        }
}

int analyse(bild_model &m)
{
    const int N = m.N, d = m.d, S = m.S;
    m.has_G = la::max_abs(m.G) != 0.0;

    // ---- reduction ------------------------------------------------------------------
    bool symmetric = true;
    for (int s = 0; s < S && symmetric; ++s)
        for (const Mat *src : {&m.B, &m.Sig, &m.C0}) {
            const double *X = src->data() + (size_t)s * N * N;
            double scale = 0.0, asym = 0.0;
            for (int i = 0; i < N; ++i)
                for (int j = 0; j < N; ++j) {
                    scale = std::max(scale, std::fabs(X[(size_t)i * N + j]));
                    asym = std::max(asym, std::fabs(X[(size_t)i * N + j] - X[(size_t)j * N + i]));
                }
            if (asym > 1e-12 * std::max(scale, 1e-300)) symmetric = false;
        }

    Mat rows;
    int n = N;
    bool reduced = false;
    if (symmetric && !(m.flags & BILD_MODEL_NO_REDUCE)) {
        invariant_subspace(m, rows, n);
        reduced = n < N && n >= 1;
    }
    if (!reduced) {
        n = N;
        rows.assign((size_t)N * N, 0.0);
        for (int i = 0; i < N; ++i) rows[(size_t)i * N + i] = 1.0;
    }
    m.n = n;
    m.V = la::transpose(rows, n, N); // N x n
    const Mat &Vt = rows;            // n x N

    auto project_sym = [&](const Mat &X3) {
        Mat out((size_t)S * n * n);
        for (int s = 0; s < S; ++s) {
            Mat X(X3.begin() + (size_t)s * N * N, X3.begin() + (size_t)(s + 1) * N * N);
            Mat t = la::matmul(Vt, X, n, N, N);
            Mat r = la::matmul(t, m.V, n, N, n);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) out[((size_t)s * n + i) * n + j] = reduced ? 0.5 * (r[(size_t)i * n + j] + r[(size_t)j * n + i]) : X[(size_t)i * N + j];
        }
        return out;
    };
    auto project_vecs = [&](const Mat &X3) {
        Mat out((size_t)S * n * d);
        for (int s = 0; s < S; ++s) {
            Mat X(X3.begin() + (size_t)s * N * d, X3.begin() + (size_t)(s + 1) * N * d);
            Mat r = la::matmul(Vt, X, n, N, d);
            std::copy(r.begin(), r.end(), out.begin() + (size_t)s * n * d);
        }
        return out;
    };
    m.rB = project_sym(m.B);
    m.rSig = project_sym(m.Sig);
    m.rC0 = project_sym(m.C0);
    m.rG = project_vecs(m.G);
    m.rM0 = project_vecs(m.M0);
    m.rw = la::matmul(Vt, m.w, n, N, 1);

    if (reduced) {
        // verify invariance: || X V - V (V^T X V) || small for every matrix; otherwise undo
        double worst = 0.0;
        for (int s = 0; s < S; ++s) {
            const Mat *full[3] = {&m.B, &m.Sig, &m.C0};
            const Mat *red[3] = {&m.rB, &m.rSig, &m.rC0};
            for (int a = 0; a < 3; ++a) {
                Mat X(full[a]->begin() + (size_t)s * N * N, full[a]->begin() + (size_t)(s + 1) * N * N);
                Mat Xr(red[a]->begin() + (size_t)s * n * n, red[a]->begin() + (size_t)(s + 1) * n * n);
                Mat XV = la::matmul(X, m.V, N, N, n);
                Mat VXr = la::matmul(m.V, Xr, N, n, n);
                double dev = 0.0;
                for (size_t i = 0; i < XV.size(); ++i) dev = std::max(dev, std::fabs(XV[i] - VXr[i]));
                worst = std::max(worst, dev / std::max(la::max_abs(X), 1e-300));
            }
        }
        if (worst > 1e-9) {
            // numerically not invariant enough: keep the full chain
            m.flags |= BILD_MODEL_NO_REDUCE;
            return analyse(m);
        }
    }

    // ---- modal analysis ---------------------------------------------------------------
    m.modal_ok = symmetric;
    m.symmetric = symmetric;
    m.modal_why = symmetric ? "" : "B, Sig or C0 is not symmetric";
    m.lam.assign((size_t)S * n, 0.0);
    m.sigd.assign((size_t)S * n, 0.0);
    m.Q.assign((size_t)S * n * n, 0.0);
    m.wq.assign((size_t)S * n, 0.0);
    m.R.assign((size_t)S * S * n * n, 0.0);
    m.C0q.assign((size_t)S * n * n, 0.0);
    m.M0q.assign((size_t)S * n * d, 0.0);
    m.Gq.assign((size_t)S * n * d, 0.0);
    if (m.modal_ok) {
        for (int s = 0; s < S; ++s) {
            Mat Bs(m.rB.begin() + (size_t)s * n * n, m.rB.begin() + (size_t)(s + 1) * n * n);
            Mat Ss(m.rSig.begin() + (size_t)s * n * n, m.rSig.begin() + (size_t)(s + 1) * n * n);
            // B and Sig of a Rouse model are functions of the same connectivity matrix and share
            // an eigenbasis.  Diagonalise a generic combination so that (near-)degenerate
            // eigenvalues of B alone (fast modes, exp(-ka) ~ 0) are still resolved.
            const double nb = std::max(la::fro(Bs), 1e-300), ns = std::max(la::fro(Ss), 1e-300);
            Mat mix((size_t)n * n);
            for (size_t i = 0; i < mix.size(); ++i) mix[i] = Bs[i] / nb + 0.61803398874989485 * Ss[i] / ns;
            std::vector<double> ev;
            Mat Q;
            la::jacobi_eigh(mix, n, ev, Q);
            Mat Qt = la::transpose(Q, n, n);
            Mat Bq = la::matmul(la::matmul(Qt, Bs, n, n, n), Q, n, n, n);
            Mat Sq = la::matmul(la::matmul(Qt, Ss, n, n, n), Q, n, n, n);
            double offB = 0.0, offS = 0.0;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    if (i != j) {
                        offB = std::max(offB, std::fabs(Bq[(size_t)i * n + j]));
                        offS = std::max(offS, std::fabs(Sq[(size_t)i * n + j]));
                    }
            if (offB > 1e-13 * std::max(la::max_abs(Bs), 1e-300) || offS > 1e-13 * std::max(la::max_abs(Ss), 1e-300)) {
                m.modal_ok = false;
                char buf[160];
                snprintf(buf, sizeof buf, "state %d: B and Sig do not share an eigenbasis (off-diagonal %.2e / %.2e)", s,
                         offB, offS);
                m.modal_why = buf;
                break;
            }
            for (int i = 0; i < n; ++i) {
                m.lam[(size_t)s * n + i] = Bq[(size_t)i * n + i];
                m.sigd[(size_t)s * n + i] = Sq[(size_t)i * n + i];
            }
            std::copy(Q.begin(), Q.end(), m.Q.begin() + (size_t)s * n * n);
            Mat ws(m.rw);
            Mat wqs = la::matmul(Qt, ws, n, n, 1);
            std::copy(wqs.begin(), wqs.end(), m.wq.begin() + (size_t)s * n);
            Mat C0s(m.rC0.begin() + (size_t)s * n * n, m.rC0.begin() + (size_t)(s + 1) * n * n);
            Mat C0qs = la::matmul(la::matmul(Qt, C0s, n, n, n), Q, n, n, n);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    m.C0q[((size_t)s * n + i) * n + j] = 0.5 * (C0qs[(size_t)i * n + j] + C0qs[(size_t)j * n + i]);
            Mat M0s(m.rM0.begin() + (size_t)s * n * d, m.rM0.begin() + (size_t)(s + 1) * n * d);
            Mat Gs(m.rG.begin() + (size_t)s * n * d, m.rG.begin() + (size_t)(s + 1) * n * d);
            Mat M0qs = la::matmul(Qt, M0s, n, n, d), Gqs = la::matmul(Qt, Gs, n, n, d);
            std::copy(M0qs.begin(), M0qs.end(), m.M0q.begin() + (size_t)s * n * d);
            std::copy(Gqs.begin(), Gqs.end(), m.Gq.begin() + (size_t)s * n * d);
        }
    }
    if (m.modal_ok) {
        for (int s2 = 0; s2 < S; ++s2)
            for (int s = 0; s < S; ++s) {
                Mat Q2(m.Q.begin() + (size_t)s2 * n * n, m.Q.begin() + (size_t)(s2 + 1) * n * n);
                Mat Q1(m.Q.begin() + (size_t)s * n * n, m.Q.begin() + (size_t)(s + 1) * n * n);
                Mat Rm = la::matmul(la::transpose(Q2, n, n), Q1, n, n, n);
                std::copy(Rm.begin(), Rm.end(), m.R.begin() + ((size_t)s2 * S + s) * n * n);
            }
    }

    // ---- pack --------------------------------------------------------------------------
    m.NP = padded_rows(n);
    if (!m.NP) {
        if (n > kWideMaxNP)
            return fail(BILD_ERR_UNSUPPORTED, "chain of %d effective modes exceeds the kernels (max %d)", n, kWideMaxNP);
        if (n <= kMidMaxNP) {
            m.NP = (n + 3) & ~3;
            m.mid = true;
        } else {
            m.NP = (n + 1) & ~1;
            m.wide = true;
        }
    }
    m.NPm[kModal] = m.NP;
    // register-resident kernels keep the basis-change matrices in LDS: all S*S pairs while that stays small
    // (two workgroups' worth of product images must still fit beside them), else the 2 S factors Q[s], Q[s]^T
    m.tab_factored = !m.wide && !m.mid && m.modal_ok && (size_t)S * S * table_stride(m.NP) * sizeof(double) > (size_t)32 * 1024;
    // the matrix-pipe kernel reads tiles transposed and relies on B, Sig, C0 being symmetric
    m.NPm[kDense] = (!m.wide && !m.mid && m.symmetric && dense_mfma_supported((n + 3) & ~3)) ? ((n + 3) & ~3) : m.NP;
    for (int mode = 0; mode < 2; ++mode) {
        const int NP = m.NPm[mode];
        const int SB = StateBlock::size(NP);
        const int MS = table_stride(NP);
        Mat &sb = m.blob_states[mode];
        Mat &tb = m.blob_tab[mode];
        sb.assign((size_t)S * SB, 0.0);
        const int ntab = mode == kDense ? 2 * S : S * S;
        tb.assign((size_t)ntab * MS, 0.0);
        if (mode == kModal && !m.modal_ok) continue;
        for (int s = 0; s < S; ++s) {
            double *b = sb.data() + (size_t)s * SB;
            const double *C0src = mode == kDense ? m.rC0.data() + (size_t)s * n * n : m.C0q.data() + (size_t)s * n * n;
            const double *M0src = mode == kDense ? m.rM0.data() + (size_t)s * n * d : m.M0q.data() + (size_t)s * n * d;
            const double *Gsrc = mode == kDense ? m.rG.data() + (size_t)s * n * d : m.Gq.data() + (size_t)s * n * d;
            for (int i = 0; i < n; ++i) {
                b[StateBlock::wq(NP) + i] = mode == kDense ? m.rw[i] : m.wq[(size_t)s * n + i];
                if (mode == kModal) {
                    b[StateBlock::lam(NP) + i] = m.lam[(size_t)s * n + i];
                    b[StateBlock::sig(NP) + i] = m.sigd[(size_t)s * n + i];
                }
                for (int k = 0; k < d; ++k) {
                    b[StateBlock::G(NP) + k * NP + i] = Gsrc[(size_t)i * d + k];
                    b[StateBlock::M0(NP) + k * NP + i] = M0src[(size_t)i * d + k];
                }
                for (int j = 0; j < n; ++j) b[StateBlock::C0(NP) + i * NP + j] = C0src[(size_t)i * n + j];
            }
        }
        auto put = [&](int slot, const double *X) {
            double *t = tb.data() + (size_t)slot * MS;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) t[i * NP + j] = X[(size_t)i * n + j];
        };
        if (mode == kDense) {
            for (int s = 0; s < S; ++s) {
                put(s, m.rB.data() + (size_t)s * n * n);
                put(S + s, m.rSig.data() + (size_t)s * n * n);
            }
        } else if (m.tab_factored) {
            // many states: S*S basis changes R[s2][s] = Q[s2]^T Q[s] would not fit LDS; keep the 2 S factors instead
            // (slot s: Q[s], modal -> common coordinates; slot S + s: Q[s]^T, back) and change basis in two steps
            tb.assign((size_t)2 * S * MS, 0.0);
            for (int s = 0; s < S; ++s) {
                Mat Q(m.Q.begin() + (size_t)s * n * n, m.Q.begin() + (size_t)(s + 1) * n * n);
                Mat Qt = la::transpose(Q, n, n);
                put(s, Q.data());
                put(S + s, Qt.data());
            }
        } else {
            for (int s2 = 0; s2 < S; ++s2)
                for (int s = 0; s < S; ++s) put(s2 * S + s, m.R.data() + ((size_t)s2 * S + s) * n * n);
        }
    }
    return BILD_OK;
}

} // namespace

namespace bild {

size_t lds_bytes(const bild_model &m, const Geometry &geom, int mode)
{
    // matrix tables (dense: B_s, Sig_s; modal: basis changes R), state headers, per-group product images and segment lists
    return LdsLayout(geom.NP, geom.W * (64 / geom.G), (int)m.blob_tab[mode].size(), m.S).frame_bytes();
}

int ensure_device(const bild_model &m)
{
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(m.mu);
    if (m.device == dev) return BILD_OK;
    if (m.device != -1)
        return fail(BILD_ERR_INVALID, "model is resident on device %d but device %d is current (one process per GPU)", m.device, dev);
    for (int mode = 0; mode < 2; ++mode) {
        HIP_TRY(hipMalloc((void **)&m.d_states[mode], m.blob_states[mode].size() * sizeof(double)));
        HIP_TRY(hipMemcpy(m.d_states[mode], m.blob_states[mode].data(), m.blob_states[mode].size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc((void **)&m.d_tab[mode], m.blob_tab[mode].size() * sizeof(double)));
        HIP_TRY(hipMemcpy(m.d_tab[mode], m.blob_tab[mode].data(), m.blob_tab[mode].size() * sizeof(double), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&m.h_in_event, hipEventDisableTiming));
    HIP_TRY(hipMalloc((void **)&m.d_frames, kFrameCounters * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(m.d_frames, 0, kFrameCounters * sizeof(unsigned long long)));
    HIP_TRY(hipDeviceSynchronize()); // (a memset is not ordered against the non-blocking stream just created)
    m.device = dev;
    return BILD_OK;
}

int pick_mode(const bild_model &m, unsigned flags, int *mode)
{
    switch (flags & 0xFu) {
    case BILD_PATH_AUTO: *mode = m.modal_ok ? kModal : kDense; return BILD_OK;
    case BILD_PATH_DENSE: *mode = kDense; return BILD_OK;
    case BILD_PATH_MODAL:
        if (!m.modal_ok) return fail(BILD_ERR_UNSUPPORTED, "modal path unavailable: %s", m.modal_why.c_str());
        *mode = kModal;
        return BILD_OK;
    default: return fail(BILD_ERR_INVALID, "unknown path selector %u", flags & 0xFu);
    }
}

int fill_params(const bild_model &m, const bild_trajset &ts, int mode, KParams &p)
{
    p.states = m.d_states[mode];
    p.tab = m.d_tab[mode];
    p.tab_doubles = (int32_t)m.blob_tab[mode].size();
    p.S = m.S;
    p.d = m.d;
    p.has_G = m.has_G ? 1 : 0;
    p.all_valid = ts.all_valid ? 1 : 0;
    p.trajs = ts.d_descs;
    p.dstar_max = ts.dstar_max;
    p.zeros = ts.d_zeros;
    p.tab_factored = (mode == kModal && m.tab_factored) ? 1 : 0;
    return BILD_OK;
}

} // namespace bild

extern "C" {

int bild_model_create(int N, int d, int S, const double *B, const double *G, const double *Sig, const double *M0,
                      const double *C0, const double *w, unsigned flags, bild_model **out)
{
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!B || !G || !Sig || !M0 || !C0 || !w) return fail(BILD_ERR_INVALID, "NULL model array");
    if (N < 1 || S < 1) return fail(BILD_ERR_INVALID, "need N >= 1 and S >= 1 (got N=%d, S=%d)", N, S);
    if (d < 1 || d > kDStore) return fail(BILD_ERR_UNSUPPORTED, "spatial dimension d=%d outside 1..%d", d, kDStore);
    if (S > 255) return fail(BILD_ERR_UNSUPPORTED, "S=%d states exceed 255", S);
    const size_t nn = (size_t)S * N * N, nd = (size_t)S * N * d;
    if (!all_finite(B, nn) || !all_finite(Sig, nn) || !all_finite(C0, nn) || !all_finite(G, nd) || !all_finite(M0, nd) ||
        !all_finite(w, (size_t)N))
        return fail(BILD_ERR_INVALID, "model arrays contain NaN or Inf");
    bild_model *m = new (std::nothrow) bild_model;
    if (!m) return fail(BILD_ERR_NOMEM, "out of memory");
    m->N = N;
    m->d = d;
    m->S = S;
    m->flags = flags;
    m->B.assign(B, B + nn);
    m->Sig.assign(Sig, Sig + nn);
    m->C0.assign(C0, C0 + nn);
    m->G.assign(G, G + nd);
    m->M0.assign(M0, M0 + nd);
    m->w.assign(w, w + N);
    int rc = analyse(*m);
    if (rc) {
        delete m;
        return rc;
    }
    *out = m;
    return BILD_OK;
}

int bild_model_destroy(bild_model *m)
{
    if (!m) return BILD_OK;
    for (int mode = 0; mode < 2; ++mode) {
        if (m->d_states[mode]) (void)hipFree(m->d_states[mode]);
        if (m->d_tab[mode]) (void)hipFree(m->d_tab[mode]);
    }
    if (m->h_in_busy) (void)hipEventSynchronize(m->h_in_event); // (a call nobody waited for still reads these blocks)
    if (m->h_in_event) (void)hipEventDestroy(m->h_in_event);
    m->ws_in.release();
    m->ws_out.release();
    m->ws_sched.release();
    for (bild_model::WorkSlot &sl : m->slots) {
        sl.ws_work.release();
        sl.ws_lists.release();
    }
    m->h_in.release();
    m->h_out.release();
    m->h_status.release();
    if (m->d_frames) (void)hipFree(m->d_frames);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
    return BILD_OK;
}

int bild_model_query(const bild_model *m, int what, int64_t *value)
{
    if (!m || !value) return fail(BILD_ERR_INVALID, "NULL argument");
    switch (what) {
    case BILD_Q_N: *value = m->N; break;
    case BILD_Q_D: *value = m->d; break;
    case BILD_Q_S: *value = m->S; break;
    case BILD_Q_MODAL_OK: *value = m->modal_ok; break;
    case BILD_Q_NP: *value = m->NP; break;
    case BILD_Q_NEFF: *value = m->n; break;
    case BILD_Q_HAS_G: *value = m->has_G; break;
    case BILD_Q_LAST_GEOMETRY: *value = m->last_geom; break;
    default: return fail(BILD_ERR_INVALID, "unknown query %d", what);
    }
    return BILD_OK;
}

int bild_model_export(const bild_model *m, int what, int s, int s2, double *buf, int64_t buf_len)
{
    if (!m || !buf) return fail(BILD_ERR_INVALID, "NULL argument");
    const int n = m->n, S = m->S;
    if (s < 0 || s >= S || s2 < 0 || s2 >= S) return fail(BILD_ERR_INVALID, "state index out of range");
    const double *src = nullptr;
    int64_t len = 0;
    switch (what) {
    case BILD_X_LAMBDA: src = m->lam.data() + (size_t)s * n; len = n; break;
    case BILD_X_SIGMA: src = m->sigd.data() + (size_t)s * n; len = n; break;
    case BILD_X_Q: src = m->Q.data() + (size_t)s * n * n; len = (int64_t)n * n; break;
    case BILD_X_WQ: src = m->wq.data() + (size_t)s * n; len = n; break;
    case BILD_X_R: src = m->R.data() + ((size_t)s2 * S + s) * n * n; len = (int64_t)n * n; break;
    case BILD_X_C0Q: src = m->C0q.data() + (size_t)s * n * n; len = (int64_t)n * n; break;
    case BILD_X_V: src = m->V.data(); len = (int64_t)m->N * n; break;
    default: return fail(BILD_ERR_INVALID, "unknown export %d", what);
    }
    if (what != BILD_X_V && !m->modal_ok) return fail(BILD_ERR_UNSUPPORTED, "modal analysis unavailable: %s", m->modal_why.c_str());
    if (buf_len < len) return fail(BILD_ERR_INVALID, "buffer too small: need %lld doubles", (long long)len);
    std::memcpy(buf, src, (size_t)len * sizeof(double));
    return BILD_OK;
}

} // extern "C"
