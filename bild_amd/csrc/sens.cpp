// Forward sensitivities of the Kalman-filter log-likelihood: the C ABI bild_logl_sensitivities (include/bild_amd.h), the
// projection of the caller's derivative arrays into each state's modal basis, its checks, and the chunking of a call
// under its workspace budget.  Kernel: sens.hip.  The likelihood tables of the trajectory set are neither built nor read.
#include "kalman.h"
#include "sens.h"
#include "sim_host.h"

namespace {

using namespace bild;

// relative residual above which a derivative is refused: outside the model's reduced subspace, or (dB, dSig) not
// diagonal in a state's modal basis
constexpr double kSensTol = 1e-9;

// the derivatives of one parameter in the padded modal layout of the kernel (SensParams)
struct ModalDerivs {
    std::vector<double> dlam, dsig, dC0, dM0, dG;
};

// X (N x N) of state s -> Q_s^T V^T X V Q_s (n x n); refuses a derivative that does not leave the reduced subspace
// invariant, and with `diag` one whose projection has off-diagonal entries.  name, p: for the message
int project_matrix(const bild_model &m, const double *X3, int s, bool diag, const char *name, int p, Mat &out)
{
    const int N = m.N, n = m.n;
    out.assign((size_t)n * n, 0.0);
    if (!X3) return BILD_OK;
    Mat X(X3 + (size_t)s * N * N, X3 + (size_t)(s + 1) * N * N);
    const double scale = la::max_abs(X);
    if (!std::isfinite(scale)) return fail(BILD_ERR_INVALID, "%s[%d] of state %d contains NaN or Inf", name, p, s);
    if (scale == 0.0) return BILD_OK;
    const Mat Vt = la::transpose(m.V, N, n);
    Mat XV = la::matmul(X, m.V, N, N, n), Xr = la::matmul(Vt, XV, n, N, n), VXr = la::matmul(m.V, Xr, N, n, n);
    double res = 0.0;
    for (size_t i = 0; i < XV.size(); ++i) res = std::max(res, std::fabs(XV[i] - VXr[i]));
    if (res > kSensTol * scale)
        return fail(BILD_ERR_UNSUPPORTED, "%s[%d] of state %d leaves the model's reduced subspace (relative residual %.3g > %.0e)",
                    name, p, s, res / scale, kSensTol);
    const Mat Q(m.Q.begin() + (size_t)s * n * n, m.Q.begin() + (size_t)(s + 1) * n * n);
    Mat Xq = la::matmul(la::matmul(la::transpose(Q, n, n), Xr, n, n, n), Q, n, n, n);
    double off = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            out[(size_t)i * n + j] = 0.5 * (Xq[(size_t)i * n + j] + Xq[(size_t)j * n + i]);
            if (i != j) off = std::max(off, std::fabs(Xq[(size_t)i * n + j]));
        }
    if (diag && off > kSensTol * scale)
        return fail(BILD_ERR_UNSUPPORTED,
                    "%s[%d] of state %d is not diagonal in the state's modal basis (relative off-diagonal %.3g > %.0e): the "
                    "parameter moves the eigenvectors", name, p, s, off / scale, kSensTol);
    return BILD_OK;
}

// X (N x d) of state s -> Q_s^T V^T X (n x d); refuses a derivative outside the reduced subspace
int project_vectors(const bild_model &m, const double *X3, int s, const char *name, int p, Mat &out)
{
    const int N = m.N, n = m.n, d = m.d;
    out.assign((size_t)n * d, 0.0);
    if (!X3) return BILD_OK;
    Mat X(X3 + (size_t)s * N * d, X3 + (size_t)(s + 1) * N * d);
    const double scale = la::max_abs(X);
    if (!std::isfinite(scale)) return fail(BILD_ERR_INVALID, "%s[%d] of state %d contains NaN or Inf", name, p, s);
    if (scale == 0.0) return BILD_OK;
    Mat Xr = la::matmul(la::transpose(m.V, N, n), X, n, N, d), VXr = la::matmul(m.V, Xr, N, n, d);
    double res = 0.0;
    for (size_t i = 0; i < X.size(); ++i) res = std::max(res, std::fabs(X[i] - VXr[i]));
    if (res > kSensTol * scale)
        return fail(BILD_ERR_UNSUPPORTED, "%s[%d] of state %d leaves the model's reduced subspace (relative residual %.3g > %.0e)",
                    name, p, s, res / scale, kSensTol);
    const Mat Q(m.Q.begin() + (size_t)s * n * n, m.Q.begin() + (size_t)(s + 1) * n * n);
    out = la::matmul(la::transpose(Q, n, n), Xr, n, n, d);
    return BILD_OK;
}

// all P parameters into the padded layout of the kernel (P x S x L, P x S x L x L, P x S x L x d)
int project_all(const bild_model &m, int P, const bild_model_derivs *dm, int L, ModalDerivs &md, bool &has_dG)
{
    const int N = m.N, n = m.n, d = m.d, S = m.S;
    md.dlam.assign((size_t)P * S * L, 0.0);
    md.dsig.assign(md.dlam.size(), 0.0);
    md.dC0.assign((size_t)P * S * L * L, 0.0);
    md.dM0.assign((size_t)P * S * L * d, 0.0);
    md.dG.assign(md.dM0.size(), 0.0);
    has_dG = false;
    if (!dm) return BILD_OK;
    const size_t nn = (size_t)S * N * N, nd = (size_t)S * N * d;
    Mat X;
    for (int p = 0; p < P; ++p) {
        auto at = [&](const double *a, size_t per) { return a ? a + (size_t)p * per : nullptr; };
        for (int s = 0; s < S; ++s) {
            const size_t o1 = ((size_t)p * S + s) * L;
            BILD_TRY(project_matrix(m, at(dm->dB, nn), s, true, "dB", p, X));
            for (int i = 0; i < n; ++i) md.dlam[o1 + i] = X[(size_t)i * n + i];
            BILD_TRY(project_matrix(m, at(dm->dSig, nn), s, true, "dSig", p, X));
            for (int i = 0; i < n; ++i) md.dsig[o1 + i] = X[(size_t)i * n + i];
            BILD_TRY(project_matrix(m, at(dm->dC0, nn), s, false, "dC0", p, X));
            for (int i = 0; i < n; ++i)
                for (int c = 0; c < n; ++c) md.dC0[(o1 + i) * L + c] = X[(size_t)i * n + c];
            BILD_TRY(project_vectors(m, at(dm->dM0, nd), s, "dM0", p, X));
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < d; ++k) md.dM0[(o1 + i) * d + k] = X[(size_t)i * d + k];
            BILD_TRY(project_vectors(m, at(dm->dG, nd), s, "dG", p, X));
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < d; ++k) {
                    md.dG[(o1 + i) * d + k] = X[(size_t)i * d + k];
                    has_dG = has_dG || X[(size_t)i * d + k] != 0.0;
                }
        }
    }
    return BILD_OK;
}

} // namespace

extern "C" int bild_logl_sensitivities(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                                       const int32_t *seg_state, const int32_t *traj_id, int P, const bild_model_derivs *dm,
                                       const double *ds2, double *logl, double *grad, double *fisher, int64_t scratch_bytes)
{
    int rc = kalman_check_args(m, ts, n, K1, seg_start, seg_state, traj_id, scratch_bytes);
    if (rc) return rc;
    if (P < 0) return fail(BILD_ERR_INVALID, "P = %d is negative", P);
    if (P > kSensMaxP) return fail(BILD_ERR_UNSUPPORTED, "at most %d parameters per call; P = %d", kSensMaxP, P);
    const int L = kalman_lanes(m->n);
    if (L == 32 && P > kSensMaxP32)
        return fail(BILD_ERR_UNSUPPORTED, "models of 17 to 32 effective modes (this one has %d) support at most %d parameters; P = %d",
                    m->n, kSensMaxP32, P);
    const int S = m->S, d = m->d, nt = ts->n_traj, D = ts->dstar_max;
    ModalDerivs md;
    bool has_dG = false;
    rc = project_all(*m, P, dm, L, md, has_dG);
    if (rc) return rc;
    // per (trajectory, chain): the derivatives of the chain's variance, equal for all dimensions of the chain
    std::vector<double> ds2c((size_t)nt * kChains * kSensMaxP, 0.0);
    if (ds2)
        for (int j = 0; j < nt; ++j) {
            const TrajDesc &td = ts->descs[j];
            for (int e = 0; e < td.dstar; ++e)
                for (int p = 0; p < P; ++p) {
                    const double v = ds2[((size_t)p * nt + j) * d + td.dims[e][0]];
                    if (!std::isfinite(v)) return fail(BILD_ERR_INVALID, "ds2[%d][%d] contains NaN or Inf", p, j);
                    for (int k = 1; k < td.ndims[e]; ++k) {
                        const double u = ds2[((size_t)p * nt + j) * d + td.dims[e][k]];
                        if (u != v)
                            return fail(BILD_ERR_UNSUPPORTED,
                                        "ds2[%d] of trajectory %d differs between dimensions %d and %d (%g vs %g), which share a "
                                        "covariance chain (equal localization errors)", p, j, td.dims[e][0], td.dims[e][k], v, u);
                    }
                    ds2c[((size_t)j * kChains + e) * kSensMaxP + p] = v;
                }
        }
    if (n == 0 || (!logl && !grad && !fisher)) return BILD_OK;

    SimBufs bufs;
    HIP_TRY(hipStreamCreateWithFlags(&bufs.stream, hipStreamNonBlocking));
    SensParams sp{};
    {
        const int nm = m->n;
        std::vector<double> lam((size_t)S * L, 0.0), sig(lam), wq(lam), C0((size_t)S * L * L, 0.0), Q(C0),
            M0((size_t)S * L * d, 0.0), G(M0);
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < nm; ++i) {
                lam[(size_t)s * L + i] = m->lam[(size_t)s * nm + i];
                sig[(size_t)s * L + i] = m->sigd[(size_t)s * nm + i];
                wq[(size_t)s * L + i] = m->wq[(size_t)s * nm + i];
                for (int c = 0; c < nm; ++c) {
                    C0[((size_t)s * L + i) * L + c] = m->C0q[((size_t)s * nm + i) * nm + c];
                    Q[((size_t)s * L + i) * L + c] = m->Q[((size_t)s * nm + i) * nm + c];
                }
                for (int k = 0; k < d; ++k) {
                    M0[((size_t)s * L + i) * d + k] = m->M0q[((size_t)s * nm + i) * d + k];
                    G[((size_t)s * L + i) * d + k] = m->Gq[((size_t)s * nm + i) * d + k];
                }
            }
        BILD_TRY(bufs.put(&sp.lam, lam.data(), lam.size()));
        BILD_TRY(bufs.put(&sp.sig, sig.data(), sig.size()));
        BILD_TRY(bufs.put(&sp.wq, wq.data(), wq.size()));
        BILD_TRY(bufs.put(&sp.C0, C0.data(), C0.size()));
        BILD_TRY(bufs.put(&sp.Q, Q.data(), Q.size()));
        BILD_TRY(bufs.put(&sp.M0, M0.data(), M0.size()));
        BILD_TRY(bufs.put(&sp.G, G.data(), G.size()));
        BILD_TRY(bufs.put(&sp.dlam, md.dlam.data(), md.dlam.size()));
        BILD_TRY(bufs.put(&sp.dsig, md.dsig.data(), md.dsig.size()));
        BILD_TRY(bufs.put(&sp.dC0, md.dC0.data(), md.dC0.size()));
        BILD_TRY(bufs.put(&sp.dM0, md.dM0.data(), md.dM0.size()));
        BILD_TRY(bufs.put(&sp.dG, md.dG.data(), md.dG.size()));
        BILD_TRY(bufs.put(&sp.ds2, ds2c.data(), ds2c.size()));
        // (the staging vectors go out of scope: the copies must have finished)
        HIP_TRY(hipStreamSynchronize(bufs.stream));
    }
    sp.trajs = ts->d_descs;
    sp.dstar_max = D;
    sp.S = S;
    sp.d = d;
    sp.K1 = K1;
    sp.has_dG = has_dG ? 1 : 0;
    // chunks of whole candidates: their segment lists and sums within the budget (the sim_host.h rule), at least one
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    const int64_t per = (int64_t)D * kSensStride + 2 * K1 + 1; // doubles (and int32 pairs, rounded up) per candidate
    const int64_t cmax = std::max<int64_t>(1, std::min<int64_t>(n, sim_scratch_bytes(scratch_bytes, free_b) / 8 / per));
    int32_t *d_start, *d_state, *d_tid = nullptr;
    BILD_TRY(bufs.put(&d_start, nullptr, (size_t)(cmax * K1)));
    BILD_TRY(bufs.put(&d_state, nullptr, (size_t)(cmax * K1)));
    if (traj_id) BILD_TRY(bufs.put(&d_tid, nullptr, (size_t)cmax));
    BILD_TRY(bufs.put(&sp.out, nullptr, (size_t)(cmax * D * kSensStride)));
    std::vector<double> h_out((size_t)(cmax * D * kSensStride));
    for (int64_t c0 = 0; c0 < n; c0 += cmax) {
        const int64_t cn = std::min(cmax, n - c0);
        HIP_TRY(hipMemcpyAsync(d_start, seg_start + c0 * K1, (size_t)(cn * K1) * 4, hipMemcpyHostToDevice, bufs.stream));
        HIP_TRY(hipMemcpyAsync(d_state, seg_state + c0 * K1, (size_t)(cn * K1) * 4, hipMemcpyHostToDevice, bufs.stream));
        if (traj_id) HIP_TRY(hipMemcpyAsync(d_tid, traj_id + c0, (size_t)cn * 4, hipMemcpyHostToDevice, bufs.stream));
        SensParams q = sp;
        q.seg_start = d_start;
        q.seg_state = d_state;
        q.traj_id = d_tid;
        q.n = cn;
        if (launch_sens(q, L, P, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the sensitivity kernel failed");
        HIP_TRY(hipMemcpyAsync(h_out.data(), sp.out, (size_t)(cn * D * kSensStride) * 8, hipMemcpyDeviceToHost, bufs.stream));
        HIP_TRY(hipStreamSynchronize(bufs.stream));
        // the chains of a candidate, added in chain order
        for (int64_t r = 0; r < cn; ++r) {
            const int64_t row = c0 + r;
            const TrajDesc &td = ts->descs[traj_id ? traj_id[row] : 0];
            double ll = 0.0, g[kSensMaxP] = {}, F[kSensMaxP][kSensMaxP] = {};
            for (int e = 0; e < td.dstar; ++e) {
                const double *o = &h_out[(size_t)((r * D + e) * kSensStride)];
                ll += o[0];
                for (int a = 0; a < P; ++a) g[a] += o[1 + a];
                for (int a = 0, f = 0; a < P; ++a)
                    for (int b = a; b < P; ++b, ++f) F[a][b] += o[1 + P + f];
            }
            if (logl) logl[row] = ll;
            for (int a = 0; a < P; ++a) {
                if (grad) grad[row * P + a] = g[a];
                if (fisher)
                    for (int b = 0; b < P; ++b) fisher[(row * P + a) * P + b] = a <= b ? F[a][b] : F[b][a];
            }
        }
    }
    return BILD_OK;
}
