// Kalman filter and smoother of candidate profiles: the C ABI bild_kalman_segments and bild_kalman_mixture
// (include/bild_amd.h), their checks, the staging of the model's modal arrays, and the chunking of a call under its
// workspace budget.  Kernels: kalman.hip.  Neither entry builds or reads the likelihood tables of the trajectory set.
#include "kalman.h"
#include "sim_host.h"

namespace bild {

// the envelope of the kernel, checked before any device work
static int check_model(const bild_model *m)
{
    if (!m->modal_ok) return fail(BILD_ERR_UNSUPPORTED, "the smoother needs the modal path, which this model lacks: %s", m->modal_why.c_str());
    if (m->n > kKalMaxModes)
        return fail(BILD_ERR_UNSUPPORTED, "the smoother supports at most %d effective modes; this model has %d", kKalMaxModes, m->n);
    if (m->d > kDStore) return fail(BILD_ERR_UNSUPPORTED, "the smoother supports at most %d dimensions; d = %d", kDStore, m->d);
    if (m->S > kKalMaxStates) return fail(BILD_ERR_UNSUPPORTED, "the smoother supports at most %d states; S = %d", kKalMaxStates, m->S);
    return BILD_OK;
}

int kalman_check_args(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start, const int32_t *seg_state,
                      const int32_t *traj_id, int64_t scratch_bytes)
{
    if (!m || !ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (ts->model != m) return fail(BILD_ERR_INVALID, "trajectory set belongs to a different model");
    if (n < 0) return fail(BILD_ERR_INVALID, "negative batch size");
    if (K1 < 1) return fail(BILD_ERR_INVALID, "need at least one segment per sample");
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    int rc = check_model(m);
    if (rc) return rc;
    if (n > 0 && (!seg_start || !seg_state)) return fail(BILD_ERR_INVALID, "NULL segment array");
    for (int64_t r = 0; r < n; ++r) {
        if (traj_id && (traj_id[r] < 0 || traj_id[r] >= ts->n_traj))
            return fail(BILD_ERR_INVALID, "traj_id[%lld]=%d out of range", (long long)r, traj_id[r]);
        const int32_t *a = seg_start + r * K1, *b = seg_state + r * K1;
        if (a[0] != 0) return fail(BILD_ERR_INVALID, "seg_start[%lld][0] must be 0", (long long)r);
        for (int i = 0; i < K1; ++i) {
            if (b[i] < 0 || b[i] >= m->S) return fail(BILD_ERR_INVALID, "state %d out of range at sample %lld", b[i], (long long)r);
            if (i > 0 && (a[i] < a[i - 1] || a[i] < 1))
                return fail(BILD_ERR_INVALID, "segment starts of sample %lld are decreasing (or a later segment starts at frame 0)", (long long)r);
        }
    }
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != ts->device) return fail(BILD_ERR_INVALID, "trajectory set lives on device %d, current device is %d", ts->device, dev);
    return BILD_OK;
}

} // namespace bild

namespace {

using namespace bild;

// One call's device state: the model's modal arrays padded to L lanes, the workspace of the records, the segment lists
struct KalCall {
    const bild_model &m;
    const bild_trajset &ts;
    SimBufs bufs;
    int L = 0, REC = 0, Tout = 0;
    KalParams p{};
    int64_t rec_cap = 0, task_cap = 0; // doubles of the record workspace, tasks of the offset array
    std::vector<int64_t> h_rec_off;
    int64_t *d_rec_off = nullptr;

    KalCall(const bild_model &m_, const bild_trajset &ts_) : m(m_), ts(ts_) {}

    int init(int Tout_)
    {
        HIP_TRY(hipStreamCreateWithFlags(&bufs.stream, hipStreamNonBlocking));
        const int n = m.n, S = m.S, d = m.d;
        L = kalman_lanes(n);
        REC = kalman_rec(L);
        Tout = Tout_;
        std::vector<double> lam((size_t)S * L, 0.0), sig(lam), wq(lam), C0((size_t)S * L * L, 0.0), Q(C0),
            M0((size_t)S * L * d, 0.0), G(M0);
        for (int s = 0; s < S; ++s)
            for (int i = 0; i < n; ++i) {
                lam[(size_t)s * L + i] = m.lam[(size_t)s * n + i];
                sig[(size_t)s * L + i] = m.sigd[(size_t)s * n + i];
                wq[(size_t)s * L + i] = m.wq[(size_t)s * n + i];
                for (int c = 0; c < n; ++c) {
                    C0[((size_t)s * L + i) * L + c] = m.C0q[((size_t)s * n + i) * n + c];
                    Q[((size_t)s * L + i) * L + c] = m.Q[((size_t)s * n + i) * n + c];
                }
                for (int k = 0; k < d; ++k) {
                    M0[((size_t)s * L + i) * d + k] = m.M0q[((size_t)s * n + i) * d + k];
                    G[((size_t)s * L + i) * d + k] = m.Gq[((size_t)s * n + i) * d + k];
                }
            }
        BILD_TRY(bufs.put(&p.lam, lam.data(), lam.size()));
        BILD_TRY(bufs.put(&p.sig, sig.data(), sig.size()));
        BILD_TRY(bufs.put(&p.wq, wq.data(), wq.size()));
        BILD_TRY(bufs.put(&p.C0, C0.data(), C0.size()));
        BILD_TRY(bufs.put(&p.Q, Q.data(), Q.size()));
        BILD_TRY(bufs.put(&p.M0, M0.data(), M0.size()));
        BILD_TRY(bufs.put(&p.G, G.data(), G.size()));
        // (the staging vectors go out of scope: the copies must have finished)
        HIP_TRY(hipStreamSynchronize(bufs.stream));
        p.trajs = ts.d_descs;
        p.dstar_max = ts.dstar_max;
        p.S = S;
        p.d = d;
        p.Tout = Tout;
        return BILD_OK;
    }
    // record doubles of candidate r on trajectory j
    int64_t rec_doubles(int j) const { return (int64_t)ts.descs[j].dstar * ts.descs[j].T * REC; }
    int reserve(int64_t rec_doubles_max, int64_t cand_max)
    {
        BILD_TRY(bufs.put(&p.rec, nullptr, (size_t)std::max<int64_t>(rec_doubles_max, 1)));
        BILD_TRY(bufs.put(&d_rec_off, nullptr, (size_t)std::max<int64_t>(cand_max * ts.dstar_max, 1)));
        task_cap = cand_max * ts.dstar_max;
        rec_cap = rec_doubles_max;
        return BILD_OK;
    }
    // candidates [c0, c1) of the device lists (seg_start, seg_state, traj_id; h_tid: host copy of traj_id or null);
    // outputs to `out` (device, row c0 first), null entries not wanted.  Waits for the kernel.
    int run(const int32_t *d_start, const int32_t *d_state, const int32_t *d_tid, const int32_t *h_tid, int K1, int64_t c0,
            int64_t c1, double *const out[kKalOutputs])
    {
        const int64_t cn = c1 - c0, D = ts.dstar_max;
        h_rec_off.assign((size_t)(cn * D), 0);
        int64_t off = 0;
        for (int64_t r = 0; r < cn; ++r) {
            const TrajDesc &td = ts.descs[h_tid ? h_tid[c0 + r] : 0];
            for (int e = 0; e < D; ++e) {
                h_rec_off[(size_t)(r * D + e)] = off;
                if (e < td.dstar) off += (int64_t)td.T * REC;
            }
        }
        if (off > rec_cap || cn * D > task_cap) return fail(BILD_ERR_INVALID, "internal: chunk exceeds its workspace");
        HIP_TRY(hipMemcpyAsync(d_rec_off, h_rec_off.data(), (size_t)(cn * D) * sizeof(int64_t), hipMemcpyHostToDevice, bufs.stream));
        KalParams q = p;
        q.seg_start = d_start + c0 * K1;
        q.seg_state = d_state + c0 * K1;
        q.traj_id = d_tid ? d_tid + c0 : nullptr;
        q.K1 = K1;
        q.n = cn;
        q.rec_off = d_rec_off;
        for (int w = 0; w < kKalOutputs; ++w) q.out[w] = out[w];
        if (launch_kalman(q, L, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the Kalman kernel failed");
        HIP_TRY(hipStreamSynchronize(bufs.stream));
        return BILD_OK;
    }
};

int64_t budget_bytes(int64_t scratch_bytes)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    return sim_scratch_bytes(scratch_bytes, free_b);
}

} // namespace

extern "C" int bild_kalman_segments(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                                    const int32_t *seg_state, const int32_t *traj_id, const bild_kalman_out *out,
                                    int64_t scratch_bytes)
{
    int rc = kalman_check_args(m, ts, n, K1, seg_start, seg_state, traj_id, scratch_bytes);
    if (rc) return rc;
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    double *const host_out[kKalOutputs] = {out->terms, out->pred_mean, out->pred_var, out->filt_mean,
                                           out->filt_var, out->smooth_mean, out->smooth_var, out->innov};
    int nout = 0;
    for (double *o : host_out) nout += o != nullptr;
    for (int64_t r = 0; r < n; ++r)
        if (out->T_max < ts->descs[traj_id ? traj_id[r] : 0].T)
            return fail(BILD_ERR_INVALID, "T_max = %d is shorter than trajectory %d (%d frames)", out->T_max, traj_id ? traj_id[r] : 0,
                        ts->descs[traj_id ? traj_id[r] : 0].T);
    if (n == 0 || nout == 0) return BILD_OK;

    KalCall kc(*m, *ts);
    BILD_TRY(kc.init(out->T_max));
    const int d = m->d;
    const int64_t row = (int64_t)out->T_max * d;
    // chunks of whole candidates: records + the wanted outputs within the budget, at least one candidate
    const int64_t budget = budget_bytes(scratch_bytes) / 8;
    std::vector<int64_t> cut{0};
    int64_t rec_max = 0, cand_max = 0;
    for (int64_t r = 0, acc = 0, racc = 0; r < n; ++r) {
        const int64_t rec = kc.rec_doubles(traj_id ? traj_id[r] : 0), need = rec + nout * row;
        if (r > cut.back() && acc + need > budget) {
            cut.push_back(r);
            acc = racc = 0;
        }
        acc += need;
        racc += rec;
        rec_max = std::max(rec_max, racc);
        cand_max = std::max(cand_max, r + 1 - cut.back());
    }
    cut.push_back(n);
    BILD_TRY(kc.reserve(rec_max, cand_max));
    int32_t *d_start, *d_state, *d_tid = nullptr;
    BILD_TRY(kc.bufs.put(&d_start, seg_start, (size_t)n * K1));
    BILD_TRY(kc.bufs.put(&d_state, seg_state, (size_t)n * K1));
    if (traj_id) BILD_TRY(kc.bufs.put(&d_tid, traj_id, (size_t)n));
    double *d_out[kKalOutputs] = {};
    for (int w = 0; w < kKalOutputs; ++w)
        if (host_out[w]) BILD_TRY(kc.bufs.put(&d_out[w], nullptr, (size_t)(cand_max * row)));
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int64_t c0 = cut[c], c1 = cut[c + 1];
        BILD_TRY(kc.run(d_start, d_state, d_tid, traj_id, K1, c0, c1, d_out));
        for (int w = 0; w < kKalOutputs; ++w)
            if (host_out[w])
                HIP_TRY(hipMemcpyAsync(host_out[w] + c0 * row, d_out[w], (size_t)((c1 - c0) * row) * 8, hipMemcpyDeviceToHost, kc.bufs.stream));
        HIP_TRY(hipStreamSynchronize(kc.bufs.stream));
    }
    return BILD_OK;
}

extern "C" int bild_kalman_mixture(const bild_model *m, const bild_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                                   const int32_t *seg_state, const int32_t *traj_id, const double *log_weights, double *mean,
                                   double *var, int64_t scratch_bytes)
{
    int rc = kalman_check_args(m, ts, n, K1, seg_start, seg_state, traj_id, scratch_bytes);
    if (rc) return rc;
    if (!mean || !var || (n > 0 && !log_weights)) return fail(BILD_ERR_INVALID, "NULL buffer");
    for (int64_t r = 0; r < n; ++r)
        if (std::isnan(log_weights[r]) || log_weights[r] == INFINITY)
            return fail(BILD_ERR_INVALID, "log_weights[%lld] = %g: log-weights must be finite or -inf", (long long)r, log_weights[r]);
    const int nt = ts->n_traj, d = m->d, Tout = ts->Tmax;
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
                blk_T.push_back(ts->descs[j].T);
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

    KalCall kc(*m, *ts);
    BILD_TRY(kc.init(Tout));
    // chunks: whole blocks (records, smoothed mean and variance, the block's partial sums), at least one block; the
    // reference tracks run in chunks of whole candidates under the same budget
    const int64_t budget = budget_bytes(scratch_bytes) / 8;
    std::vector<int> bcut{0};
    int64_t rec_max = 0, cand_max = 0, blk_max = 0;
    {
        int64_t acc = 0, racc = 0;
        for (int b = 0; b < nblk; ++b) {
            int64_t rec = 0;
            for (int32_t q = blk_start[b]; q < blk_start[b + 1]; ++q) rec += kc.rec_doubles(g_tid[(size_t)(nref + q)]);
            const int64_t cands = blk_start[b + 1] - blk_start[b];
            const int64_t need = rec + cands * 2 * row + 3 * row;
            if (b > bcut.back() && acc + need > budget) {
                bcut.push_back(b);
                acc = racc = 0;
            }
            acc += need;
            racc += rec;
            rec_max = std::max(rec_max, racc);
            cand_max = std::max<int64_t>(cand_max, blk_start[b + 1] - blk_start[bcut.back()]);
            blk_max = std::max<int64_t>(blk_max, b + 1 - bcut.back());
        }
        bcut.push_back(nblk);
    }
    std::vector<int64_t> rcut{0};
    {
        int64_t acc = 0;
        for (int64_t q = 0; q < nref; ++q) {
            const int64_t need = kc.rec_doubles(ref_tid[q]);
            if (q > rcut.back() && acc + need > std::max(budget, rec_max)) {
                rcut.push_back(q);
                acc = 0;
            }
            acc += need;
            rec_max = std::max(rec_max, acc);
            cand_max = std::max(cand_max, q + 1 - rcut.back());
        }
        rcut.push_back(nref);
    }
    BILD_TRY(kc.reserve(rec_max, cand_max));
    int32_t *d_start, *d_state, *d_tid, *d_ref_row, *d_blk_start, *d_blk_traj, *d_blk_T, *d_run_b0;
    double *d_ref, *d_w, *d_mean, *d_var, *d_part, *d_acc;
    BILD_TRY(kc.bufs.put(&d_start, g_start.data(), g_start.size()));
    BILD_TRY(kc.bufs.put(&d_state, g_state.data(), g_state.size()));
    BILD_TRY(kc.bufs.put(&d_tid, g_tid.data(), g_tid.size()));
    BILD_TRY(kc.bufs.put(&d_ref_row, ref_row.data(), ref_row.size()));
    BILD_TRY(kc.bufs.put(&d_w, wts.data(), wts.size()));
    BILD_TRY(kc.bufs.put(&d_blk_start, blk_start.data(), blk_start.size()));
    BILD_TRY(kc.bufs.put(&d_blk_traj, blk_traj.data(), blk_traj.size()));
    BILD_TRY(kc.bufs.put(&d_blk_T, blk_T.data(), blk_T.size()));
    BILD_TRY(kc.bufs.put(&d_run_b0, nullptr, (size_t)blk_max + 1));
    BILD_TRY(kc.bufs.put(&d_ref, nullptr, (size_t)(nref * row)));
    BILD_TRY(kc.bufs.put(&d_mean, nullptr, (size_t)(cand_max * row)));
    BILD_TRY(kc.bufs.put(&d_var, nullptr, (size_t)(cand_max * row)));
    BILD_TRY(kc.bufs.put(&d_part, nullptr, (size_t)(blk_max * row * 3)));
    BILD_TRY(kc.bufs.put(&d_acc, nullptr, (size_t)(nt * row * 3)));
    HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)(nt * row * 3) * 8, kc.bufs.stream));
    for (size_t c = 0; c + 1 < rcut.size(); ++c) {
        double *o[kKalOutputs] = {};
        o[5] = d_ref + rcut[c] * row;
        BILD_TRY(kc.run(d_start, d_state, d_tid, g_tid.data(), K1, rcut[c], rcut[c + 1], o));
    }
    std::vector<int32_t> run_b0;
    for (size_t c = 0; c + 1 < bcut.size(); ++c) {
        const int b0 = bcut[c], b1 = bcut[c + 1];
        const int64_t c0 = nref + blk_start[b0], c1 = nref + blk_start[b1];
        double *o[kKalOutputs] = {};
        o[5] = d_mean;
        o[6] = d_var;
        BILD_TRY(kc.run(d_start, d_state, d_tid, g_tid.data(), K1, c0, c1, o));
        run_b0.clear();
        for (int b = b0; b < b1; ++b)
            if (b == b0 || blk_traj[b] != blk_traj[b - 1]) run_b0.push_back(b - b0);
        run_b0.push_back(b1 - b0);
        // chunk-local block offsets
        std::vector<int32_t> lstart(blk_start.begin() + b0, blk_start.begin() + b1 + 1);
        for (int32_t &v : lstart) v -= blk_start[b0];
        int32_t *d_lstart;
        BILD_TRY(kc.bufs.put(&d_lstart, lstart.data(), lstart.size()));
        HIP_TRY(hipMemcpyAsync(d_run_b0, run_b0.data(), run_b0.size() * 4, hipMemcpyHostToDevice, kc.bufs.stream));
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
        if (launch_kalman_mix(mp, kc.bufs.stream)) return fail(BILD_ERR_HIP, "launch of the mixture kernels failed");
        HIP_TRY(hipStreamSynchronize(kc.bufs.stream));
    }
    std::vector<double> acc((size_t)(nt * row * 3)), ref((size_t)(nref * row));
    HIP_TRY(hipMemcpyAsync(acc.data(), d_acc, acc.size() * 8, hipMemcpyDeviceToHost, kc.bufs.stream));
    HIP_TRY(hipMemcpyAsync(ref.data(), d_ref, ref.size() * 8, hipMemcpyDeviceToHost, kc.bufs.stream));
    HIP_TRY(hipStreamSynchronize(kc.bufs.stream));
    // law of total variance around the reference track: mean = ref + s1 / W, var = s2 / W + s3 / W - (s1 / W)^2
    for (int j = 0; j < nt; ++j) {
        if (per[j].empty()) continue;
        const int64_t T = ts->descs[j].T;
        for (int64_t tk = 0; tk < T * d; ++tk) {
            const double *a = &acc[(size_t)((j * row + tk) * 3)];
            const double s1 = a[0] / W[j];
            mean[j * row + tk] = ref[(size_t)(ref_row[j] * row + tk)] + s1;
            var[j * row + tk] = a[1] / W[j] + (a[2] / W[j] - s1 * s1);
        }
    }
    return BILD_OK;
}
