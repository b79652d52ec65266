// GenericGaussianModel: the C ABI (include/bild_amd.h, "GenericGaussianModel"), the host side of the table build and the
// evaluation calls.  The kernels and the decomposition they compute are described in gauss.hip.
#include <chrono>
#include <initializer_list>

#include "likelihood.h"
#include "gauss.h"
#include "internal.h"

struct bild_gauss_trajset {
    const bild_gauss_model *model = nullptr;
    int n_traj = 0;
    std::vector<int> T;
    double *tables = nullptr;           // per trajectory: W (S x T(T+1)/2), then F (S x (T+1))
    bild::GaussTraj *d_trajs = nullptr;
    int64_t table_bytes = 0;
    double build_ms = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;                      // evaluation staging below
    DeviceBuf d_in, d_out;
    PinnedBuf h_out;
};

namespace {

using namespace bild;

// Device memory of one build, freed on every path
struct BuildBufs {
    std::vector<void *> ptrs;
    ~BuildBufs()
    {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class X> int alloc(X **out, size_t count)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(X));
        if (e != hipSuccess) return fail(BILD_ERR_NOMEM, "hipMalloc(%zu) failed: %s", count * sizeof(X), hipGetErrorString(e));
        ptrs.push_back(p);
        *out = static_cast<X *>(p);
        return BILD_OK;
    }
};

// The tables of one trajectory (x: T x d, NaN = missing) into W / F.  Dimensions in index order; per dimension and state:
// the shared factor of the valid tail, the starts inside it (solve), the others (per-start factorisation, in chunks of
// `slots` scratch slots).
int build_one(const bild_gauss_model *m, int T, const double *x, const double *d_msd, double *W, double *F, double *d_tau,
              double *d_factor, double *d_scratch, int64_t scratch_doubles, BuildBufs &bufs, hipStream_t stream)
{
    const int S = m->S, d = m->d;
    // per dimension: valid frames, their values, ranks; staged once
    std::vector<int32_t> vidx((size_t)d * T), rank((size_t)d * T), order_d((size_t)d * S);
    std::vector<double> xv((size_t)d * T);
    std::vector<int> V(d), tail(d);
    for (int k = 0; k < d; ++k) {
        int v = 0;
        for (int t = 0; t < T; ++t) {
            rank[(size_t)k * T + t] = v;
            const double val = x[(size_t)t * d + k];
            if (!std::isnan(val)) {
                vidx[(size_t)k * T + v] = t;
                xv[(size_t)k * T + v] = val;
                ++v;
            }
        }
        V[k] = v;
        int c = 0;
        while (c < v && vidx[(size_t)k * T + v - 1 - c] == T - 1 - c) ++c;
        tail[k] = c;
        for (int s = 0; s < S; ++s) order_d[(size_t)k * S + s] = m->order[(size_t)s * d + k];
    }
    // the jobs of every (dimension, state): [shared factor][solves][factorisations]
    struct Group {
        int dim, s, shared, solve0, nsolve, fact0, nfact, nT, nmax;
    };
    std::vector<GaussJob> jobs;
    std::vector<Group> groups;
    for (int k = 0; k < d; ++k)
        for (int s = 0; s < S; ++s) {
            const int o = m->order[(size_t)s * d + k], v = V[k], c = tail[k];
            auto len = [&](int r) { return std::max(0, o == 0 ? v - r : v - r - 1); };
            Group g{k, s, -1, 0, 0, 0, 0, std::max(0, o == 0 ? c : c - 1), 0};
            const int row0 = s * (v + 1);
            std::vector<GaussJob> solve, fact;
            auto add = [&](int r, int row, int centred) {
                const int n = len(r);
                if (n <= 0) return;
                GaussJob j{r, n, row, centred, 0};
                if (r >= v - c) solve.push_back(j);
                else {
                    fact.push_back(j);
                    g.nmax = std::max(g.nmax, n);
                }
            };
            for (int r = 0; r < v; ++r) add(r, row0 + r, 0);
            if (o == 0) add(0, row0 + v, 1);     // the first interval: centred first value
            if (g.nT > 0 && !solve.empty()) {
                g.shared = (int)jobs.size();
                jobs.push_back(GaussJob{v - c, g.nT, -1, 0, 1});
            }
            g.solve0 = (int)jobs.size();
            g.nsolve = (int)solve.size();
            jobs.insert(jobs.end(), solve.begin(), solve.end());
            g.fact0 = (int)jobs.size();
            g.nfact = (int)fact.size();
            jobs.insert(jobs.end(), fact.begin(), fact.end());
            groups.push_back(g);
        }

    int32_t *d_vidx, *d_rank, *d_order;
    double *d_xv;
    GaussJob *d_jobs;
    BILD_TRY(bufs.alloc(&d_vidx, vidx.size()));
    BILD_TRY(bufs.alloc(&d_rank, rank.size()));
    BILD_TRY(bufs.alloc(&d_order, order_d.size()));
    BILD_TRY(bufs.alloc(&d_xv, xv.size()));
    BILD_TRY(bufs.alloc(&d_jobs, jobs.size()));
    HIP_TRY(hipMemcpyAsync(d_vidx, vidx.data(), vidx.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_rank, rank.data(), rank.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_order, order_d.data(), order_d.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(d_xv, xv.data(), xv.size() * 8, hipMemcpyHostToDevice, stream));
    if (!jobs.empty()) HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), jobs.size() * sizeof(GaussJob), hipMemcpyHostToDevice, stream));

    size_t gi = 0;
    for (int k = 0; k < d; ++k) {
        const int v = V[k];
        for (int s = 0; s < S; ++s, ++gi) {
            const Group &g = groups[gi];
            GaussJobSet p{};
            p.vidx = d_vidx + (size_t)k * T;
            p.xv = d_xv + (size_t)k * T;
            p.msd = d_msd + ((size_t)s * d + k) * (m->L + 1);
            p.msd_inf = m->msd_inf[(size_t)s * d + k];
            p.mean = m->mean[(size_t)s * d + k];
            p.order = m->order[(size_t)s * d + k];
            p.tau = d_tau;
            p.tau_ld = std::max(v, 1);
            p.factor = d_factor;
            if (g.shared >= 0 && launch_gauss_factor(p, d_jobs + g.shared, 1, nullptr, 0, stream))
                return fail(BILD_ERR_HIP, "launch of the shared-factor kernel failed");
            if (launch_gauss_solve(p, d_jobs + g.solve0, g.nsolve, g.nT, stream))
                return fail(BILD_ERR_HIP, "launch of the solve kernel failed");
            if (g.nfact > 0) {
                const int64_t slot = (int64_t)(g.nmax + 1) * g.nmax;
                const int64_t slots = std::min<int64_t>(scratch_doubles / slot, g.nfact);
                if (slots < 1) return fail(BILD_ERR_NOMEM, "factorisation scratch of %lld bytes does not fit the budget", (long long)slot * 8);
                for (int j0 = 0; j0 < g.nfact; j0 += (int)slots) {
                    const int cnt = (int)std::min<int64_t>(slots, g.nfact - j0);
                    if (launch_gauss_factor(p, d_jobs + g.fact0 + j0, cnt, d_scratch, slot, stream))
                        return fail(BILD_ERR_HIP, "launch of the factorisation kernel failed");
                }
            }
        }
        GaussAccum a{};
        a.vidx = d_vidx + (size_t)k * T;
        a.rank_of = d_rank + (size_t)k * T;
        a.tau = d_tau;
        a.tau_ld = std::max(v, 1);
        a.order = d_order + (size_t)k * S;
        a.W = W;
        a.F = F;
        a.w_per_state = gauss_w_per_state(T);
        a.S = S;
        a.T = T;
        a.V = v;
        a.dim = k;
        if (launch_gauss_accumulate(a, stream)) return fail(BILD_ERR_HIP, "launch of the accumulate kernel failed");
    }
    HIP_TRY(hipStreamSynchronize(stream));     // the host vectors above are staged from pageable memory
    return BILD_OK;
}

int destroy_set(bild_gauss_trajset *ts)
{
    if (!ts) return BILD_OK;
    if (ts->stream) (void)hipStreamSynchronize(ts->stream);
    if (ts->tables) (void)hipFree(ts->tables);
    if (ts->d_trajs) (void)hipFree(ts->d_trajs);
    ts->d_in.release();
    ts->d_out.release();
    ts->h_out.release();
    if (ts->stream) (void)hipStreamDestroy(ts->stream);
    delete ts;
    return BILD_OK;
}

int check_eval(const bild_gauss_model *m, const bild_gauss_trajset *ts, int64_t n, int K1, const int32_t *traj_id, const double *out)
{
    if (!m || !ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (ts->model != m) return fail(BILD_ERR_INVALID, "trajectory set belongs to a different model");
    if (n < 0 || K1 < 1) return fail(BILD_ERR_INVALID, "n = %lld, K1 = %d", (long long)n, K1);
    if (n > 0 && !out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (traj_id)
        for (int64_t r = 0; r < n; ++r)
            if (traj_id[r] < 0 || traj_id[r] >= ts->n_traj)
                return fail(BILD_ERR_INVALID, "traj_id[%lld] = %d out of range (%d trajectories)", (long long)r, traj_id[r], ts->n_traj);
    return BILD_OK;
}

struct Part {
    const void *host;
    size_t bytes;
    const void **field;     // the walk's pointer to set to the staged copy (stays null without data)
};

// stage the parts into one device buffer, run the walk, copy the results to `out`
int run_walk(bild_gauss_trajset *ts, GaussWalk &w, bool st, std::initializer_list<Part> parts, int32_t *status_out, double *out)
{
    std::lock_guard<std::mutex> lock(ts->mu);
    size_t total = 256;     // status
    for (const Part &pp : parts) total += (pp.bytes + 255) & ~size_t(255);
    BILD_TRY(ts->d_in.reserve(total));
    BILD_TRY(ts->d_out.reserve((size_t)w.n * 8));
    BILD_TRY(ts->h_out.reserve((size_t)w.n * 8 + 8));
    char *base = static_cast<char *>(ts->d_in.ptr);
    size_t off = 0;
    for (const Part &pp : parts) {
        if (!pp.host || !pp.bytes) continue;
        *pp.field = base + off;
        HIP_TRY(hipMemcpyAsync(base + off, pp.host, pp.bytes, hipMemcpyHostToDevice, ts->stream));
        off += (pp.bytes + 255) & ~size_t(255);
    }
    int32_t *d_status = reinterpret_cast<int32_t *>(base + off);
    HIP_TRY(hipMemsetAsync(d_status, 0, 8, ts->stream));
    w.status = d_status;
    w.out = static_cast<double *>(ts->d_out.ptr);
    w.trajs = ts->d_trajs;
    if (launch_gauss_walk(w, st, ts->stream)) return fail(BILD_ERR_HIP, "launch of the walk kernel failed");
    double *h = static_cast<double *>(ts->h_out.ptr);
    HIP_TRY(hipMemcpyAsync(h, ts->d_out.ptr, (size_t)w.n * 8, hipMemcpyDeviceToHost, ts->stream));
    HIP_TRY(hipMemcpyAsync(h + w.n, d_status, 8, hipMemcpyDeviceToHost, ts->stream));
    HIP_TRY(hipStreamSynchronize(ts->stream));
    std::memcpy(out, h, (size_t)w.n * 8);
    std::memcpy(status_out, h + w.n, 8);
    return BILD_OK;
}

} // namespace

int bild::internal_gauss_set_lengths(const bild_gauss_model *m, const bild_gauss_trajset *ts, int *n_traj, const int **T)
{
    if (!m || !ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (ts->model != m) return fail(BILD_ERR_INVALID, "trajectory set belongs to a different model");
    *n_traj = ts->n_traj;
    *T = ts->T.data();
    return BILD_OK;
}

int bild::internal_gauss_set_device(const bild_gauss_model *m, const bild_gauss_trajset *ts, const GaussTraj **d_trajs, void **stream,
                                    std::mutex **mu)
{
    if (!m || !ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (ts->model != m) return fail(BILD_ERR_INVALID, "trajectory set belongs to a different model");
    *d_trajs = ts->d_trajs;
    *stream = (void *)ts->stream;
    *mu = const_cast<std::mutex *>(&ts->mu);
    return BILD_OK;
}

int bild::internal_gauss_walk_resident(const bild_gauss_model *m, const bild_gauss_trajset *ts, int64_t n, int K1, const int32_t *d_seg_start,
                                       const int32_t *d_seg_state, const int32_t *d_traj_id, double *d_out, void *stream)
{
    if (!m || !ts || ts->model != m || n < 0 || K1 < 1 || !d_seg_start || !d_seg_state || !d_out)
        return fail(BILD_ERR_INVALID, "internal_gauss_walk_resident: bad arguments");
    GaussWalk w{};
    w.trajs = ts->d_trajs;
    w.seg_start = d_seg_start;
    w.seg_state = d_seg_state;
    w.traj_id = d_traj_id;
    w.out = d_out;
    w.n = n;
    w.K1 = K1;
    w.S = m->S;
    if (launch_gauss_walk(w, false, stream)) return fail(BILD_ERR_HIP, "launch of the walk kernel failed");
    return BILD_OK;
}

extern "C" {

int bild_gauss_model_create(int S, int d, int Tmax, const int32_t *ss_order, const double *mean, const double *msd,
                            const double *msd_inf, bild_gauss_model **out)
{
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (S < 1 || d < 1) return fail(BILD_ERR_INVALID, "S = %d and d = %d must be positive", S, d);
    if (Tmax < 0) return fail(BILD_ERR_INVALID, "Tmax = %d must be non-negative", Tmax);
    if (!ss_order || !mean || !msd || !msd_inf) return fail(BILD_ERR_INVALID, "NULL array");
    const size_t sd = (size_t)S * d, L1 = (size_t)Tmax + 1;
    for (size_t i = 0; i < sd; ++i) {
        if (ss_order[i] != 0 && ss_order[i] != 1)
            return fail(BILD_ERR_INVALID, "ss_order[%zu] = %d; must be 0 or 1", i, ss_order[i]);
        if (!std::isfinite(mean[i])) return fail(BILD_ERR_INVALID, "mean[%zu] is not finite", i);
        if (ss_order[i] == 0 && !std::isfinite(msd_inf[i]))
            return fail(BILD_ERR_INVALID, "msd_inf[%zu] is not finite (needed for ss_order 0)", i);
        for (size_t l = 0; l < L1; ++l)
            if (!std::isfinite(msd[i * L1 + l])) return fail(BILD_ERR_INVALID, "msd[%zu][%zu] is not finite", i, l);
    }
    auto *m = new bild_gauss_model;
    m->S = S;
    m->d = d;
    m->L = Tmax;
    m->order.assign(ss_order, ss_order + sd);
    m->mean.assign(mean, mean + sd);
    m->msd_inf.assign(msd_inf, msd_inf + sd);
    m->msd.assign(msd, msd + sd * L1);
    *out = m;
    return BILD_OK;
}

int bild_gauss_model_destroy(bild_gauss_model *m)
{
    if (m && m->factors) (void)hipFree(m->factors);     // only a model that simulated holds device memory
    delete m;
    return BILD_OK;
}

int bild_gauss_trajset_create(const bild_gauss_model *m, int n_traj, const int32_t *T, const double *x, bild_gauss_trajset **out)
{
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!m || !T || !x) return fail(BILD_ERR_INVALID, "NULL argument");
    if (n_traj < 1) return fail(BILD_ERR_INVALID, "n_traj = %d must be positive", n_traj);
    for (int j = 0; j < n_traj; ++j) {
        if (T[j] < 1) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames", j, T[j]);
        if (T[j] > kGaussMaxT)
            return fail(BILD_ERR_UNSUPPORTED, "trajectory %d has %d frames; GenericGaussianModel supports at most %d", j, T[j], kGaussMaxT);
        if (T[j] - 1 > m->L)
            return fail(BILD_ERR_INVALID, "trajectory %d has %d frames but the MSD tables end at lag %d", j, T[j], m->L);
    }
    int dev = 0;
    if (hipGetDeviceCount(&dev) != hipSuccess || dev < 1) return fail(BILD_ERR_NO_DEVICE, "no usable GPU");

    auto *ts = new bild_gauss_trajset;
    ts->model = m;
    ts->n_traj = n_traj;
    ts->T.assign(T, T + n_traj);
    struct Guard {
        bild_gauss_trajset *ts;
        ~Guard()
        {
            if (ts) destroy_set(ts);
        }
    } guard{ts};
    HIP_TRY(hipStreamCreateWithFlags(&ts->stream, hipStreamNonBlocking));

    const int S = m->S, d = m->d;
    int Tmax = 0;
    std::vector<int64_t> off(n_traj + 1, 0);
    for (int j = 0; j < n_traj; ++j) {
        Tmax = std::max(Tmax, T[j]);
        off[j + 1] = off[j] + (int64_t)S * (gauss_w_per_state(T[j]) + T[j] + 1);
    }
    ts->table_bytes = off[n_traj] * 8;
    HIP_TRY(hipMalloc(&ts->tables, (size_t)ts->table_bytes));
    HIP_TRY(hipMalloc(&ts->d_trajs, sizeof(GaussTraj) * n_traj));

    const auto t_start = std::chrono::steady_clock::now();
    BuildBufs bufs;
    double *d_msd, *d_tau, *d_factor, *d_scratch;
    BILD_TRY(bufs.alloc(&d_msd, m->msd.size()));
    HIP_TRY(hipMemcpyAsync(d_msd, m->msd.data(), m->msd.size() * 8, hipMemcpyHostToDevice, ts->stream));
    BILD_TRY(bufs.alloc(&d_tau, (size_t)S * (Tmax + 1) * Tmax));
    BILD_TRY(bufs.alloc(&d_factor, (size_t)Tmax * Tmax));
    // per-start factorisation scratch: at most 1 GiB and at most a third of the free memory, no more than all starts need
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int64_t slot_max = (int64_t)(Tmax + 1) * Tmax;
    int64_t scratch_doubles = std::min<int64_t>({(int64_t)(1ll << 30) / 8, (int64_t)(free_b / 3) / 8, slot_max * Tmax});
    scratch_doubles = std::max<int64_t>(scratch_doubles, slot_max);    // at least one slot, else the build cannot run
    BILD_TRY(bufs.alloc(&d_scratch, (size_t)scratch_doubles));

    std::vector<GaussTraj> desc(n_traj);
    const double *xj = x;
    for (int j = 0; j < n_traj; ++j) {
        double *W = ts->tables + off[j];
        double *F = W + (int64_t)S * gauss_w_per_state(T[j]);
        desc[j] = GaussTraj{W, F, gauss_w_per_state(T[j]), T[j]};
        BILD_TRY(build_one(m, T[j], xj, d_msd, W, F, d_tau, d_factor, d_scratch, scratch_doubles, bufs, ts->stream));
        xj += (size_t)T[j] * d;
    }
    HIP_TRY(hipMemcpyAsync(ts->d_trajs, desc.data(), sizeof(GaussTraj) * n_traj, hipMemcpyHostToDevice, ts->stream));
    HIP_TRY(hipStreamSynchronize(ts->stream));
    ts->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    guard.ts = nullptr;
    *out = ts;
    return BILD_OK;
}

int bild_gauss_trajset_destroy(bild_gauss_trajset *ts) { return destroy_set(ts); }

int bild_gauss_trajset_info(const bild_gauss_trajset *ts, int64_t *table_bytes, double *build_ms)
{
    if (!ts) return fail(BILD_ERR_INVALID, "NULL handle");
    if (table_bytes) *table_bytes = ts->table_bytes;
    if (build_ms) *build_ms = ts->build_ms;
    return BILD_OK;
}

int bild_gauss_logl_segments(const bild_gauss_model *m, const bild_gauss_trajset *ts, int64_t n, int K1, const int32_t *seg_start,
                             const int32_t *seg_state, const int32_t *traj_id, double *out)
{
    BILD_TRY(check_eval(m, ts, n, K1, traj_id, out));
    if (n == 0) return BILD_OK;
    if (!seg_start || !seg_state) return fail(BILD_ERR_INVALID, "NULL segment arrays");
    for (int64_t r = 0; r < n; ++r) {
        const int32_t *a = seg_start + r * K1, *b = seg_state + r * K1;
        if (a[0] != 0) return fail(BILD_ERR_INVALID, "sample %lld: the first segment must start at 0", (long long)r);
        for (int i = 0; i < K1; ++i) {
            if (b[i] < 0 || b[i] >= m->S) return fail(BILD_ERR_INVALID, "sample %lld: state %d out of range", (long long)r, b[i]);
            if (i > 0 && (a[i] < 1 || a[i] < a[i - 1]))
                return fail(BILD_ERR_INVALID, "sample %lld: segment starts must be >= 1 and non-decreasing", (long long)r);
        }
    }
    GaussWalk w{};
    w.n = n;
    w.K1 = K1;
    w.S = m->S;
    int32_t status[2] = {0, 0};
    BILD_TRY(run_walk(const_cast<bild_gauss_trajset *>(ts), w, false,
                       {{seg_start, (size_t)n * K1 * 4, (const void **)&w.seg_start},
                        {seg_state, (size_t)n * K1 * 4, (const void **)&w.seg_state},
                        {traj_id, traj_id ? (size_t)n * 4 : 0, (const void **)&w.traj_id}},
                       status, out));
    return BILD_OK;
}

int bild_gauss_logl_st(const bild_gauss_model *m, const bild_gauss_trajset *ts, int64_t n, int K1, const double *ss,
                       const int64_t *thetas, const int32_t *traj_id, double *out)
{
    BILD_TRY(check_eval(m, ts, n, K1, traj_id, out));
    if (n == 0) return BILD_OK;
    if (!ss || !thetas) return fail(BILD_ERR_INVALID, "NULL ss / thetas");
    GaussWalk w{};
    w.n = n;
    w.K1 = K1;
    w.S = m->S;
    int32_t status[2] = {0, 0};
    BILD_TRY(run_walk(const_cast<bild_gauss_trajset *>(ts), w, true,
                       {{ss, (size_t)n * K1 * 8, (const void **)&w.ss},
                        {thetas, (size_t)n * K1 * 8, (const void **)&w.thetas},
                        {traj_id, traj_id ? (size_t)n * 4 : 0, (const void **)&w.traj_id}},
                       status, out));
    if (status[0])
        return fail(BILD_ERR_INVALID, "sample %d: a state is out of range, or the interval lengths are not non-negative finite numbers "
                                      "(of a point on the simplex)", status[1]);
    return BILD_OK;
}

} // extern "C"
