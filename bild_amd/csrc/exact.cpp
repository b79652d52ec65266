// Exact evidence by enumeration (include/bild_amd.h, "exact evidence"): the count, the refusals, the
// plan of blocks and chunks, and the per-chunk sequence enumerate -> likelihood -> reduce -> fold.  Kernels: exact.hip.
#include <functional>
#include <limits>

#include "exact.h"
#include "gauss.h"
#include "gauss_call.h"
#include "gauss_segdp.h"

namespace {

using namespace bild;

constexpr double kTwo53 = 9007199254740992.0;

// C(n, k) as a double: exact while the value is below 2^53 (products of integers kept exact in 128 bits while they fit)
double binom_double(int64_t n, int k)
{
    if (n < k || n < 0) return 0.0;
    unsigned __int128 c = 1;
    for (int i = 0; i < k; ++i) {
        const unsigned __int128 next = c * (unsigned __int128)(n - i);
        if (next / (unsigned __int128)(n - i) != c || next >> 120) {     // too large to carry exactly: the rest in double
            double d = (double)c;
            for (int i2 = i; i2 < k; ++i2) d = d * (double)(n - i2) / (double)(i2 + 1);
            return d;
        }
        c = next / (unsigned __int128)(i + 1);
    }
    return (double)c;
}

// valid traces of k switches: sum of the entries of transitions^k (as a double: exact below 2^53)
double trace_count(int S, const uint8_t *tr, int k)
{
    std::vector<double> v(S, 1.0), w(S);
    for (int step = 0; step < k; ++step) {
        for (int a = 0; a < S; ++a) {
            double acc = 0.0;
            for (int b = 0; b < S; ++b)
                if (tr[a * S + b]) acc += v[b];
            w[a] = acc;
        }
        v.swap(w);
    }
    double n = 0.0;
    for (double x : v) n += x;
    return n;
}

// the traces in CFC.full_sample order: extended slot by slot, each trace by its allowed successors in ascending order
std::vector<int32_t> full_sample(int S, const uint8_t *tr, int k)
{
    std::vector<int32_t> cur(S);
    for (int s = 0; s < S; ++s) cur[s] = s;
    for (int len = 1; len <= k; ++len) {
        std::vector<int32_t> nxt;
        const size_t n = cur.size() / len;
        for (size_t i = 0; i < n; ++i) {
            const int32_t *t = cur.data() + i * len;
            for (int b = 0; b < S; ++b)
                if (tr[t[len - 1] * S + b]) {
                    nxt.insert(nxt.end(), t, t + len);
                    nxt.push_back(b);
                }
        }
        cur.swap(nxt);
    }
    return cur;
}

// C(a, m) at a * (k + 1) + m for a < A, saturated at 2^64 - 1
std::vector<uint64_t> binom_table(int A, int k)
{
    const int K1 = k + 1;
    std::vector<uint64_t> t((size_t)A * K1, 0);
    for (int a = 0; a < A; ++a) {
        t[(size_t)a * K1] = 1;
        for (int m = 1; m <= k; ++m) {
            if (a == 0) continue;
            const uint64_t x = t[(size_t)(a - 1) * K1 + m - 1], y = t[(size_t)(a - 1) * K1 + m];
            t[(size_t)a * K1 + m] = x + y < x ? UINT64_MAX : x + y;
        }
    }
    return t;
}

// profile L of a trajectory of T frames as segment rows: the host twin of exact_enumerate_kernel
void unrank(int64_t L, int T, int k, int64_t C, const std::vector<int32_t> &traces, const std::vector<uint64_t> &binom, int32_t *ss,
            int32_t *sv)
{
    const int K1 = k + 1, n = T - 1;
    const int64_t tr = L / C;
    uint64_t r = (uint64_t)(C - 1 - (L - tr * C));
    ss[0] = 0;
    sv[0] = traces[(size_t)tr * K1];
    int hi = n - 1;
    for (int j = 1; j <= k; ++j) {
        const int m = k - j + 1;
        int lo = m - 1, top = hi;
        while (lo < top) {
            const int mid = (lo + top + 1) >> 1;
            if (binom[(size_t)mid * K1 + m] <= r) lo = mid;
            else top = mid - 1;
        }
        r -= binom[(size_t)lo * K1 + m];
        ss[j] = n - lo;
        sv[j] = traces[(size_t)tr * K1 + j];
        hi = lo - 1;
    }
}

// What the refusals leave for the device part
struct Plan {
    int n_traj = 0, S = 0, k = 0, Tm = 1;
    std::vector<int32_t> T;
    std::vector<int64_t> count;     // profiles per trajectory
    std::vector<int64_t> ncomb;     // C(T - 1, k) per trajectory
    std::vector<int32_t> traces;
    bool marginals = false;
};

// every refusal, before any device work
int plan_call(int n_traj, const int *T, int S, int k, const uint8_t *transitions, double max_profiles, int64_t scratch_bytes, int T_max,
              const bild_exact_out *out, Plan *p)
{
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (k < 0 || k > kExactMaxK) return fail(BILD_ERR_UNSUPPORTED, "k = %d: exact enumeration supports 0 <= k <= %d", k, kExactMaxK);
    BILD_TRY(segdp_check_transitions(S, transitions));
    if (!(max_profiles >= 0)) return fail(BILD_ERR_INVALID, "max_profiles must be a non-negative number");
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    p->n_traj = n_traj;
    p->S = S;
    p->k = k;
    p->T.assign(T, T + n_traj);
    p->marginals = out->log_post != nullptr;
    const double ntr = trace_count(S, transitions, k);
    double total = 0.0;
    for (int j = 0; j < n_traj; ++j) {
        if (T[j] > T_max) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames, more than T_max = %d", j, T[j], T_max);
        p->Tm = std::max(p->Tm, T[j]);
        const double c = binom_double(T[j] - 1, k);
        total += c * ntr;
        if (c * ntr >= kTwo53)
            return fail(BILD_ERR_UNSUPPORTED, "trajectory %d: %.6g profiles at k = %d; exact enumeration indexes fewer than 2^53", j,
                        c * ntr, k);
        p->ncomb.push_back((int64_t)c);
        p->count.push_back((int64_t)(c * ntr));
        if (p->marginals && c > 0 && (int64_t)S * T[j] > kExactMargMax)
            return fail(BILD_ERR_UNSUPPORTED, "trajectory %d: marginals of S x T = %d x %d exceed the %d values of a block's LDS accumulators",
                        j, S, T[j], kExactMargMax);
    }
    if (total > max_profiles)
        return fail(BILD_ERR_UNSUPPORTED, "%.17g profiles in all (k = %d, %d trajectories) exceed max_profiles = %.17g", total, k, n_traj,
                    max_profiles);
    if (total > 0) {
        if (ntr > (double)(1 << 26)) return fail(BILD_ERR_UNSUPPORTED, "%.6g valid traces at k = %d: the trace table is limited to 2^26", ntr, k);
        p->traces = full_sample(S, transitions, k);
    }
    return BILD_OK;
}

using Eval = std::function<int(int64_t rows, const int32_t *d_ss, const int32_t *d_sv, const int32_t *d_tid, double *d_out)>;

// the device part: plan of blocks and chunks, one pass per chunk, results to `out`.  On `st`, under `held` where the stream
// is shared.
int run_exact(const Plan &p, int64_t scratch_bytes, int T_max, hipStream_t st, std::unique_lock<std::mutex> held, const Eval &eval,
              bild_exact_out *out)
{
    CallFrame call;
    call.open(st, std::move(held));
    const int k = p.k, K1 = k + 1, S = p.S, n_traj = p.n_traj, Tm = p.Tm;
    const bool marg = p.marginals;

    // blocks in trajectory order, then chunks of whole blocks
    std::vector<ExactBlock> blocks;
    for (int j = 0; j < n_traj; ++j)
        for (int64_t l0 = 0; l0 < p.count[j]; l0 += kExactBlock)
            blocks.push_back(ExactBlock{l0, 0, j, (int32_t)std::min<int64_t>(kExactBlock, p.count[j] - l0)});
    const int64_t nblocks = (int64_t)blocks.size();
    const int64_t per_block = (int64_t)kExactBlock * (8 * K1 + 4 + 8) + (int64_t)sizeof(ExactPart) + (marg ? (int64_t)S * Tm * 8 : 0);
    int chunk = 0;
    BILD_TRY(call.chunk_of(per_block, scratch_bytes, 1 << 20, &chunk));
    const int64_t chunk_blocks = chunk;
    struct Chunk {
        int64_t b0, nb, rows, r0, nr;   // blocks [b0, b0 + nb), rows, runs [r0, r0 + nr)
    };
    std::vector<Chunk> chunks;
    std::vector<ExactRun> runs;
    for (int64_t b0 = 0; b0 < nblocks; b0 += chunk_blocks) {
        Chunk c{b0, std::min(chunk_blocks, nblocks - b0), 0, (int64_t)runs.size(), 0};
        for (int64_t b = b0; b < b0 + c.nb; ++b) {
            blocks[b].row0 = c.rows;
            c.rows += blocks[b].n;
            if (b == b0 || blocks[b].traj != blocks[b - 1].traj) runs.push_back(ExactRun{blocks[b].traj, (int32_t)(b - b0), 0, 0});
            ++runs.back().nb;
        }
        c.nr = (int64_t)runs.size() - c.r0;
        chunks.push_back(c);
    }
    int64_t max_rows = 0, max_nb = 0;
    for (const Chunk &c : chunks) {
        max_rows = std::max(max_rows, c.rows);
        max_nb = std::max(max_nb, c.nb);
    }

    const int A = std::max(1, Tm - 1);
    const std::vector<uint64_t> binom = binom_table(A, k);
    ExactBlock *d_blocks;
    ExactRun *d_runs;
    uint64_t *d_binom;
    int32_t *d_traces, *d_T, *d_ss, *d_sv, *d_tid;
    int64_t *d_ncomb;
    ExactAcc *d_acc;
    ExactPart *d_part;
    double *d_logl, *d_marg = nullptr, *d_acc_marg = nullptr;
    BILD_TRY(call.alloc(&d_blocks, blocks.size()));
    BILD_TRY(call.alloc(&d_runs, runs.size()));
    BILD_TRY(call.alloc(&d_binom, binom.size()));
    BILD_TRY(call.alloc(&d_traces, p.traces.size()));
    BILD_TRY(call.alloc(&d_T, n_traj));
    BILD_TRY(call.alloc(&d_ncomb, n_traj));
    BILD_TRY(call.alloc(&d_acc, n_traj));
    BILD_TRY(call.alloc(&d_ss, (size_t)max_rows * K1));
    BILD_TRY(call.alloc(&d_sv, (size_t)max_rows * K1));
    BILD_TRY(call.alloc(&d_tid, (size_t)max_rows));
    BILD_TRY(call.alloc(&d_logl, (size_t)max_rows));
    BILD_TRY(call.alloc(&d_part, (size_t)max_nb));
    if (marg) {
        BILD_TRY(call.alloc(&d_marg, (size_t)max_nb * S * Tm));
        BILD_TRY(call.alloc(&d_acc_marg, (size_t)n_traj * S * Tm));
        HIP_TRY(hipMemsetAsync(d_acc_marg, 0, (size_t)n_traj * S * Tm * 8, st));
    }
    std::vector<ExactAcc> acc(n_traj, ExactAcc{-std::numeric_limits<double>::infinity(), 0.0, 0.0,
                                               std::numeric_limits<double>::quiet_NaN(), -1, 0});
    // (synchronous copies: the host vectors are gone when the stream gets to them otherwise)
    HIP_TRY(hipMemcpy(d_blocks, blocks.data(), blocks.size() * sizeof(ExactBlock), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_runs, runs.data(), runs.size() * sizeof(ExactRun), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_binom, binom.data(), binom.size() * 8, hipMemcpyHostToDevice));
    if (!p.traces.empty()) HIP_TRY(hipMemcpy(d_traces, p.traces.data(), p.traces.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_T, p.T.data(), (size_t)n_traj * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ncomb, p.ncomb.data(), (size_t)n_traj * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_acc, acc.data(), (size_t)n_traj * sizeof(ExactAcc), hipMemcpyHostToDevice));

    for (const Chunk &c : chunks) {
        ExactEnum e{};
        e.blocks = d_blocks + c.b0;
        e.binom = d_binom;
        e.traces = d_traces;
        e.ncomb = d_ncomb;
        e.T = d_T;
        e.seg_start = d_ss;
        e.seg_state = d_sv;
        e.traj_id = d_tid;
        e.nblocks = (int)c.nb;
        e.k = k;
        e.A = A;
        if (launch_exact_enumerate(e, st)) return fail(BILD_ERR_HIP, "launch of the enumeration kernel failed");
        BILD_TRY(eval(c.rows, d_ss, d_sv, d_tid, d_logl));
        ExactReduce r{};
        r.blocks = d_blocks + c.b0;
        r.logl = d_logl;
        r.seg_start = d_ss;
        r.seg_state = d_sv;
        r.T = d_T;
        r.part = d_part;
        r.marg = d_marg;
        r.nblocks = (int)c.nb;
        r.K1 = K1;
        r.S = S;
        r.Tm = Tm;
        if (launch_exact_reduce(r, st)) return fail(BILD_ERR_HIP, "launch of the reduction kernel failed");
        ExactFold f{};
        f.runs = d_runs + c.r0;
        f.part = d_part;
        f.marg = d_marg;
        f.T = d_T;
        f.acc = d_acc;
        f.acc_marg = d_acc_marg;
        f.nruns = (int)c.nr;
        f.S = S;
        f.Tm = Tm;
        if (launch_exact_fold(f, st)) return fail(BILD_ERR_HIP, "launch of the fold kernel failed");
    }
    std::vector<double> post(marg ? (size_t)n_traj * S * Tm : 0);
    HIP_TRY(hipMemcpyAsync(acc.data(), d_acc, (size_t)n_traj * sizeof(ExactAcc), hipMemcpyDeviceToHost, st));
    if (marg) HIP_TRY(hipMemcpyAsync(post.data(), d_acc_marg, post.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // per trajectory: the host's formulas (FixedkSampler.fix_exhaustive, log_marginal_posterior)
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();
    for (int j = 0; j < n_traj; ++j) {
        const ExactAcc &a = acc[j];
        const int64_t N = p.count[j];
        double logev = ninf, kl = nan;
        if (N > 0 && a.n_nan > 0) logev = nan;
        else if (N > 0 && a.M != ninf) {
            const double ev = a.s / (double)N;
            logev = std::log(ev) + a.M;
            kl = (a.sl / (double)N) / ev - logev;
        }
        if (out->logev) out->logev[j] = logev;
        if (out->kl) out->kl[j] = kl;
        if (out->n_nan) out->n_nan[j] = N > 0 ? a.n_nan : 0;
        if (out->map_logl) out->map_logl[j] = N > 0 && a.map_idx >= 0 ? a.map_l : nan;
        int32_t *ms = out->map_seg_start ? out->map_seg_start + (size_t)j * K1 : nullptr;
        int32_t *mv = out->map_seg_state ? out->map_seg_state + (size_t)j * K1 : nullptr;
        std::vector<int32_t> tmp_s(K1, -1), tmp_v(K1, -1);
        if (N > 0 && a.map_idx >= 0) unrank(a.map_idx, p.T[j], k, p.ncomb[j], p.traces, binom, tmp_s.data(), tmp_v.data());
        if (ms) std::copy(tmp_s.begin(), tmp_s.end(), ms);
        if (mv) std::copy(tmp_v.begin(), tmp_v.end(), mv);
        if (!marg) continue;
        double *lp = out->log_post + (size_t)j * S * T_max;
        const bool usable = N > 0 && a.n_nan == 0 && a.M != ninf;
        for (int t = 0; t < T_max; ++t) {
            double tot = 0.0;
            if (usable && t < p.T[j])
                for (int s = 0; s < S; ++s) tot += post[((size_t)j * S + s) * Tm + t];
            for (int s = 0; s < S; ++s)
                lp[(size_t)s * T_max + t] = usable && t < p.T[j] ? std::log(post[((size_t)j * S + s) * Tm + t]) - std::log(tot) : nan;
        }
    }
    return BILD_OK;
}

} // namespace

extern "C" {

int bild_exact_count(int T, int k, int S, const uint8_t *transitions, double *n_profiles)
{
    if (!n_profiles) return fail(BILD_ERR_INVALID, "n_profiles is NULL");
    if (T < 1) return fail(BILD_ERR_INVALID, "T = %d must be positive", T);
    if (S < 1) return fail(BILD_ERR_INVALID, "S = %d must be positive", S);
    if (k < 0 || k > kExactMaxK) return fail(BILD_ERR_UNSUPPORTED, "k = %d: exact enumeration supports 0 <= k <= %d", k, kExactMaxK);
    BILD_TRY(segdp_check_transitions(S, transitions));
    *n_profiles = binom_double(T - 1, k) * trace_count(S, transitions, k);
    return BILD_OK;
}

int bild_exact_evidence(const bild_model *m, const bild_trajset *ts, int k, const uint8_t *transitions, double max_profiles,
                        int64_t scratch_bytes, int T_max, unsigned flags, bild_exact_out *out)
{
    if (!m || !ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (ts->model != m) return fail(BILD_ERR_INVALID, "trajectory set belongs to a different model");
    std::vector<int> T(ts->n_traj);
    for (int j = 0; j < ts->n_traj; ++j) T[j] = ts->descs[j].T;
    Plan p;
    BILD_TRY(plan_call(ts->n_traj, T.data(), m->S, k, transitions, max_profiles, scratch_bytes, T_max, out, &p));
    int64_t total = 0;
    for (int64_t c : p.count) total += c;
    // a set that has not been evaluated yet and sees 1e8 evaluations here: the state table may take its larger budget
    if (ts->prefix_state == 0 && ts->expected_evals < total && (ts->expected_evals >= 0 || total >= (int64_t)100000000))
        ts->expected_evals = total;
    hipStream_t st = (hipStream_t)internal_model_stream(m);
    if (!st) return BILD_ERR_NO_DEVICE;
    const int K1 = k + 1;
    auto eval = [&](int64_t rows, const int32_t *d_ss, const int32_t *d_sv, const int32_t *d_tid, double *d_out) {
        return bild_logl_segments_device(m, ts, rows, K1, d_ss, d_sv, d_tid, flags & 0xfu, (void *)st, d_out);
    };
    // the model's stream: one call at a time, as for the host-buffer calls
    return run_exact(p, scratch_bytes, T_max, st, std::unique_lock<std::mutex>(m->call_mu), eval, out);
}

int bild_gauss_exact_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k, const uint8_t *transitions,
                              double max_profiles, int64_t scratch_bytes, int T_max, bild_exact_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    BILD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    Plan p;
    BILD_TRY(plan_call(n_traj, T, m->S, k, transitions, max_profiles, scratch_bytes, T_max, out, &p));
    hipStream_t st = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } guard{st};
    const int K1 = k + 1;
    auto eval = [&](int64_t rows, const int32_t *d_ss, const int32_t *d_sv, const int32_t *d_tid, double *d_out) {
        return internal_gauss_walk_resident(m, ts, rows, K1, d_ss, d_sv, d_tid, d_out, (void *)st);
    };
    return run_exact(p, scratch_bytes, T_max, st, std::unique_lock<std::mutex>(), eval, out);     // a stream of the call's own
}

} // extern "C"
