// GenericGaussianModel's trajectory generator: the C ABI bild_gauss_simulate (include/bild_amd.h), its checks, the
// model's cache of Toeplitz factors, the columns of the product and the chunked normals.  Kernels: gauss.hip ("the
// generator"); derivation: DESIGN.md section 12.
#include "gauss.h"
#include "sim_host.h"

namespace {

using namespace bild;

// The factors of every (state, dimension) for trajectories of up to T frames, built with the likelihood's column sweep
// (one workgroup each, one launch).  The sweep is left-looking, so a factor's leading block does not depend on its size:
// growing the cache changes no result.  Called with m->sim_mu held; the temporaries live in the call's `bufs`.
int ensure_factors(const bild_gauss_model *m, int T, SimBufs &bufs)
{
    if (m->factors && m->factor_T >= T) return BILD_OK;
    const int sd = m->S * m->d;
    std::vector<int64_t> off(sd + 1, 0);
    std::vector<int> nn(sd);
    for (int i = 0; i < sd; ++i) {
        nn[i] = m->order[i] == 0 ? T : T - 1;
        off[i + 1] = off[i] + (int64_t)nn[i] * nn[i];
    }
    if (m->factors) (void)hipFree(m->factors);
    m->factors = nullptr;
    m->factor_T = 0;
    void *f = nullptr;
    hipError_t e = hipMalloc(&f, (size_t)std::max<int64_t>(off[sd], 1) * 8);
    if (e != hipSuccess) return fail(BILD_ERR_NOMEM, "hipMalloc(%lld) of the generator's factors failed: %s", (long long)off[sd] * 8,
                                     hipGetErrorString(e));
    double *factors = static_cast<double *>(f);

    std::vector<int32_t> times(T);
    for (int t = 0; t < T; ++t) times[t] = t;
    double *d_msd;
    int32_t *d_times;
    BILD_TRY(bufs.put(&d_msd, m->msd.data(), m->msd.size()));
    BILD_TRY(bufs.put(&d_times, times.data(), times.size()));
    std::vector<GaussJobSet> sets(sd);
    std::vector<GaussJob> jobs(sd);
    for (int i = 0; i < sd; ++i) {
        GaussJobSet &p = sets[i];
        p.vidx = d_times;
        p.msd = d_msd + (size_t)i * (m->L + 1);
        p.msd_inf = m->msd_inf[i];
        p.mean = m->mean[i];
        p.order = m->order[i];
        p.factor = factors + off[i];
        jobs[i] = GaussJob{0, nn[i], -1, 0, 1};
    }
    GaussJobSet *d_sets;
    GaussJob *d_jobs;
    BILD_TRY(bufs.put(&d_sets, sets.data(), sets.size()));
    BILD_TRY(bufs.put(&d_jobs, jobs.data(), jobs.size()));
    // (the cache owns the memory from here: a failure below leaves it allocated but empty, freed by the next build or destroy)
    m->factors = factors;
    if (launch_gauss_factor_sets(d_sets, d_jobs, sd, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the factor kernel failed");
    // the diagonals, for the check of each call
    std::vector<double> diag((size_t)std::max(sd * T, 1));
    for (int i = 0; i < sd; ++i)
        if (nn[i] > 0)
            HIP_TRY(hipMemcpy2DAsync(diag.data() + (size_t)i * T, 8, factors + off[i], (size_t)(nn[i] + 1) * 8, 8, nn[i],
                                     hipMemcpyDeviceToHost, bufs.stream));
    HIP_TRY(hipStreamSynchronize(bufs.stream));
    m->factor_off.assign(off.begin(), off.end() - 1);
    m->factor_n = nn;
    m->factor_ok.assign(sd, 0);
    for (int i = 0; i < sd; ++i) {
        int ok = 0;
        while (ok < nn[i] && std::isfinite(diag[(size_t)i * T + ok]) && diag[(size_t)i * T + ok] > 0) ++ok;
        m->factor_ok[i] = ok;
    }
    m->factor_T = T;
    return BILD_OK;
}

} // namespace

extern "C" int bild_gauss_simulate(const bild_gauss_model *m, int n, const int32_t *T, int K1, const int32_t *seg_start,
                                   const int32_t *seg_state, const uint8_t *missing, const double *normals, uint64_t seed,
                                   int64_t scratch_bytes, double *out)
{
    if (!m) return fail(BILD_ERR_INVALID, "NULL model");
    if (n < 0 || K1 < 1) return fail(BILD_ERR_INVALID, "n = %d, K1 = %d", n, K1);
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    if (n > 0 && (!T || !seg_start || !seg_state || !out)) return fail(BILD_ERR_INVALID, "NULL trajectory array");
    if (n == 0) return BILD_OK;
    const int S = m->S, d = m->d;

    // trajectories: lengths, intervals (runs of equal state, as the walk of the likelihood reads segments), normals
    std::vector<int64_t> frame_off(n + 1, 0), z_off(n + 1, 0), iv_off(n + 1, 0);
    std::vector<int32_t> iv;
    int Tmax = 0;
    for (int i = 0; i < n; ++i) {
        const int Ti = T[i];
        if (Ti < 1) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames", i, Ti);
        if (Ti > kGaussMaxT)
            return fail(BILD_ERR_UNSUPPORTED, "trajectory %d has %d frames; GenericGaussianModel supports at most %d", i, Ti, kGaussMaxT);
        if (Ti - 1 > m->L)
            return fail(BILD_ERR_UNSUPPORTED, "trajectory %d has %d frames but the MSD tables end at lag %d", i, Ti, m->L);
        Tmax = std::max(Tmax, Ti);
        const int32_t *a = seg_start + (size_t)i * K1, *s = seg_state + (size_t)i * K1;
        if (a[0] != 0) return fail(BILD_ERR_INVALID, "trajectory %d: the first segment must start at 0", i);
        for (int q = 0; q < K1; ++q) {
            if (s[q] < 0 || s[q] >= S) return fail(BILD_ERR_INVALID, "trajectory %d: state %d out of range (%d states)", i, s[q], S);
            if (q > 0 && (a[q] < 1 || a[q] < a[q - 1]))
                return fail(BILD_ERR_INVALID, "trajectory %d: segment starts must be >= 1 and non-decreasing", i);
        }
        int t0 = 0, cur = s[0];
        for (int q = 1; q < K1; ++q) {
            const int st = std::min(a[q], Ti), en = q + 1 < K1 ? std::min(a[q + 1], Ti) : Ti;
            if (en <= st || s[q] == cur) continue;
            iv.insert(iv.end(), {t0, st, cur});
            t0 = st;
            cur = s[q];
        }
        iv.insert(iv.end(), {t0, Ti, cur});
        iv_off[i + 1] = (int64_t)iv.size() / 3;
        frame_off[i + 1] = frame_off[i] + Ti;
        int64_t nz = 0;
        for (int k = 0; k < d; ++k) nz += Ti - m->order[(size_t)s[0] * d + k];
        z_off[i + 1] = z_off[i] + nz;
    }
    const int64_t rows = frame_off[n];

    int dev = 0;
    if (hipGetDeviceCount(&dev) != hipSuccess || dev < 1) return fail(BILD_ERR_NO_DEVICE, "no usable GPU");
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    // the normals of a chunk of whole trajectories, host-drawn (replay) or drawn on the device, within the budget
    const int64_t scratch = sim_scratch_bytes(scratch_bytes, free_b);
    const int64_t scratch_doubles = std::min<int64_t>(scratch / 8, z_off[n]);
    for (int i = 0; i < n; ++i)
        if (z_off[i + 1] - z_off[i] > scratch_doubles)
            return fail(BILD_ERR_UNSUPPORTED, "trajectory %d needs %lld bytes of normals; the budget is %lld", i,
                        (long long)(z_off[i + 1] - z_off[i]) * 8, (long long)scratch);

    std::lock_guard<std::mutex> lock(m->sim_mu);
    SimBufs bufs;
    HIP_TRY(hipStreamCreateWithFlags(&bufs.stream, hipStreamNonBlocking));
    BILD_TRY(ensure_factors(m, Tmax, bufs));

    // the columns, chunk by chunk, in the loop's order of the normals: per trajectory, interval, dimension
    std::vector<GaussSimCol> cols;
    std::vector<GaussSimBlock> blocks;
    std::vector<GaussSimTask> tasks;
    std::vector<int> chunk_end, col_off{0}, task_off{0};
    std::vector<int> need((size_t)S * d, 0);
    for (int first = 0; first < n;) {
        const int last = sim_chunk_end(z_off, first, n, scratch_doubles);
        const size_t c_begin = cols.size();
        for (int i = first; i < last; ++i) {
            int64_t zo = z_off[i] - z_off[first];
            for (int64_t v = iv_off[i]; v < iv_off[i + 1]; ++v) {
                const int t0 = iv[3 * v], t1 = iv[3 * v + 1], s = iv[3 * v + 2];
                for (int k = 0; k < d; ++k) {
                    const int o = m->order[(size_t)s * d + k];
                    GaussSimCol c{};
                    if (t0 == 0) {
                        c.frame0 = o;
                        c.len = t1 - o;
                    } else {
                        c.skip0 = 1 - o;
                        c.frame0 = t0 - c.skip0;
                        c.len = t1 - t0 + c.skip0;
                    }
                    c.z = zo - c.skip0;
                    c.row = frame_off[i] + c.frame0;
                    c.traj = i;
                    c.k = s * d + k;    // (the group key while sorting; the dimension afterwards)
                    zo += c.len - c.skip0;
                    if (c.len > c.skip0) {
                        cols.push_back(c);
                        need[c.k] = std::max(need[c.k], c.len);
                    }
                }
            }
        }
        // grouped by (state, dimension), longest first; blocks of up to kGaussSimTN, tasks of kGaussSimTM rows
        std::stable_sort(cols.begin() + c_begin, cols.end(), [](const GaussSimCol &x, const GaussSimCol &y) {
            return x.k != y.k ? x.k < y.k : x.len > y.len;
        });
        const size_t b_begin = blocks.size();
        for (size_t c = c_begin; c < cols.size();) {
            const int sk = cols[c].k;
            size_t e = c + 1;
            while (e < cols.size() && e - c < (size_t)kGaussSimTN && cols[e].k == sk) ++e;
            blocks.push_back(GaussSimBlock{m->factors + m->factor_off[sk], m->factor_n[sk], sk % d, (int)c, (int)(e - c), cols[c].len});
            c = e;
        }
        for (size_t c = c_begin; c < cols.size(); ++c) cols[c].k %= d;
        std::vector<size_t> order(blocks.size() - b_begin);
        for (size_t b = 0; b < order.size(); ++b) order[b] = b_begin + b;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return blocks[x].nmax > blocks[y].nmax; });
        for (size_t b : order)
            for (int r0 = 0; r0 < blocks[b].nmax; r0 += kGaussSimTM) tasks.push_back(GaussSimTask{(int)b, r0});
        chunk_end.push_back(last);
        col_off.push_back((int)cols.size());
        task_off.push_back((int)tasks.size());
        first = last;
    }
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < d; ++k) {
            const int sk = s * d + k;
            if (need[sk] > m->factor_ok[sk])
                return fail(BILD_ERR_INVALID, "state %d, dimension %d: the covariance of a window of %d %s is not positive definite", s, k,
                            need[sk], m->order[sk] == 0 ? "frames" : "increments");
        }

    std::vector<const double *> Ls((size_t)S * d);
    for (int sk = 0; sk < S * d; ++sk) Ls[sk] = m->factors + m->factor_off[sk];
    GaussSimProduct p{};
    GaussSimAssemble a{};
    BILD_TRY(bufs.put(&p.cols, cols.data(), cols.size()));
    BILD_TRY(bufs.put(&p.blocks, blocks.data(), blocks.size()));
    BILD_TRY(bufs.put(&p.tasks, tasks.data(), tasks.size()));
    double *d_z, *d_out;
    BILD_TRY(bufs.put(&d_z, nullptr, (size_t)scratch_doubles));
    BILD_TRY(bufs.put(&d_out, nullptr, (size_t)rows * d));
    BILD_TRY(bufs.put(&a.frame_off, frame_off.data(), n + 1));
    BILD_TRY(bufs.put(&a.iv_off, iv_off.data(), n + 1));
    BILD_TRY(bufs.put(&a.iv, iv.data(), iv.size()));
    BILD_TRY(bufs.put(&a.order, m->order.data(), m->order.size()));
    BILD_TRY(bufs.put(&a.mean, m->mean.data(), m->mean.size()));
    BILD_TRY(bufs.put(&a.L, Ls.data(), Ls.size()));
    uint8_t *d_missing;
    BILD_TRY(bufs.put(&d_missing, missing, rows));
    if (!missing) HIP_TRY(hipMemsetAsync(d_missing, 0, rows, bufs.stream));
    a.missing = d_missing;
    a.out = p.out = d_out;
    a.d = p.d = d;
    p.z = d_z;
    p.seed = seed;

    const GaussSimCol *all_cols = p.cols;
    const GaussSimTask *all_tasks = p.tasks;
    for (size_t c = 0, first = 0; c < chunk_end.size(); first = chunk_end[c++]) {
        const int last = chunk_end[c];
        if (normals) {
            // (pageable source: the copy is staged, and the next chunk's copy waits for this chunk's kernels on the stream)
            HIP_TRY(hipMemcpyAsync(d_z, normals + z_off[first], (size_t)(z_off[last] - z_off[first]) * 8, hipMemcpyHostToDevice,
                                   bufs.stream));
        } else {
            GaussSimProduct q = p;
            q.cols = all_cols + col_off[c];
            q.ncols = col_off[c + 1] - col_off[c];
            if (launch_gauss_sim_normals(q, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the normals kernel failed");
        }
        GaussSimProduct q = p;
        q.tasks = all_tasks + task_off[c];
        q.ntasks = task_off[c + 1] - task_off[c];
        if (launch_gauss_sim_product(q, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the product kernel failed");
        GaussSimAssemble r = a;
        r.frame_off += first;
        r.iv_off += first;
        r.n = last - (int)first;
        if (launch_gauss_sim_assemble(r, bufs.stream)) return fail(BILD_ERR_HIP, "launch of the assembly kernel failed");
    }
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)rows * d * 8, hipMemcpyDeviceToHost, bufs.stream));
    HIP_TRY(hipStreamSynchronize(bufs.stream));
    return BILD_OK;
}
