// Exact evidence of every k by a segment recursion (include/bild_amd.h, "exact evidence of every k"):
// the refusals, the chunks of whole trajectories, the launches level after level on the set's stream, and the host's
// formulas on the last column of the forward table.  Kernels: gauss_segdp.hip.
#include <cmath>
#include <limits>

#include "likelihood.h"
#include "gauss_segdp.h"
#include "internal.h"

namespace {

using namespace bild;

#define SD_TRY(x)                       \
    do {                                \
        int rc_ = (x);                  \
        if (rc_ != BILD_OK) return rc_; \
    } while (0)

// Device memory of one call, freed on every path
struct Bufs {
    std::vector<void *> ptrs;
    ~Bufs()
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

// C(n, k) from exact integer steps (each division is exact), carried in a 64-bit mantissa once it no longer fits 128 bits
long double binom_ld(int n, int k)
{
    if (k < 0 || n < k) return 0.0L;
    unsigned __int128 c = 1;
    for (int i = 0; i < k; ++i) {
        const unsigned __int128 f = (unsigned __int128)(n - i);
        if (c >> 100) {
            long double d = (long double)c;
            for (int i2 = i; i2 < k; ++i2) d = d * (long double)(n - i2) / (long double)(i2 + 1);
            return d;
        }
        c = c * f / (unsigned __int128)(i + 1);
    }
    return (long double)c;
}

// valid traces of k switches for every k < K: the sum of the entries of transitions^k
std::vector<long double> trace_counts(int S, const uint8_t *tr, int K)
{
    std::vector<long double> out(K), v(S, 1.0L), w(S);
    for (int k = 0; k < K; ++k) {
        long double n = 0.0L;
        for (long double x : v) n += x;
        out[k] = n;
        for (int a = 0; a < S; ++a) {
            long double acc = 0.0L;
            for (int b = 0; b < S; ++b)
                if (tr[a * S + b]) acc += v[b];
            w[a] = acc;
        }
        v.swap(w);
    }
    return out;
}

int alloc_fwd(Bufs &bufs, SegdpFwd *t, size_t n)
{
    SD_TRY(bufs.alloc(&t->M, n));
    SD_TRY(bufs.alloc(&t->Z, n));
    SD_TRY(bufs.alloc(&t->R, n));
    SD_TRY(bufs.alloc(&t->ok, n));
    SD_TRY(bufs.alloc(&t->bad, n));
    return bufs.alloc(&t->arg, n);
}

} // namespace

extern "C" int bild_gauss_segment_evidence(const bild_gauss_model *m, const bild_gauss_trajset *ts, int k_max, const uint8_t *transitions,
                                           int T_max, unsigned flags, int64_t scratch_bytes, bild_segdp_out *out)
{
    int n_traj = 0;
    const int *T = nullptr;
    SD_TRY(internal_gauss_set_lengths(m, ts, &n_traj, &T));
    if (!out) return fail(BILD_ERR_INVALID, "out is NULL");
    if (k_max < 0 || k_max > kSegdpMaxK)
        return fail(BILD_ERR_UNSUPPORTED, "k_max = %d: the segment recursion supports 0 <= k_max <= %d", k_max, kSegdpMaxK);
    if (flags & ~BILD_SEGDP_NAN_OMIT) return fail(BILD_ERR_INVALID, "flags = %u: unknown bits", flags);
    const int S = m->S;
    if (!transitions) return fail(BILD_ERR_INVALID, "transitions is NULL");
    for (int i = 0; i < S * S; ++i)
        if (transitions[i] > 1) return fail(BILD_ERR_INVALID, "transitions[%d] = %d; must be 0 or 1", i, transitions[i]);
    if (scratch_bytes < 0) return fail(BILD_ERR_INVALID, "scratch_bytes = %lld is negative", (long long)scratch_bytes);
    int Tm = 1;
    for (int j = 0; j < n_traj; ++j) {
        if (T[j] > T_max) return fail(BILD_ERR_INVALID, "trajectory %d has %d frames, more than T_max = %d", j, T[j], T_max);
        Tm = std::max(Tm, T[j]);
    }
    if (n_traj == 0) return BILD_OK;
    const bool omit = (flags & BILD_SEGDP_NAN_OMIT) != 0, marg = out->log_post != nullptr;
    const int K = k_max + 1, ld = Tm + 1, ntile = (Tm + kSegdpTile - 1) / kSegdpTile;
    const int64_t slot = (int64_t)K * S * ld, rows = (int64_t)K * S * ntile * Tm;

    const GaussTraj *d_trajs = nullptr;
    void *stream = nullptr;
    std::mutex *mu = nullptr;
    SD_TRY(internal_gauss_set_device(m, ts, &d_trajs, &stream, &mu));
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(*mu);      // the set's stream: one call at a time

    // chunks of whole trajectories within the budget (at least one)
    const int64_t per_traj = slot * (2 * (5 * 8 + 4) + (marg ? 6 * 8 : 0)) + (marg ? rows * 8 : 0) + (int64_t)K * K * 8 + (int64_t)K * S * 40;
    int64_t budget = scratch_bytes;
    if (budget == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<int64_t>((int64_t)1 << 30, (int64_t)(free_b / 3));
    }
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(budget / per_traj, n_traj));

    Bufs bufs;
    struct Drain {      // (declared after the buffers: on an error path the stream is drained before they are freed)
        hipStream_t s;
        ~Drain() { (void)hipStreamSynchronize(s); }
    } drain{st};
    SegdpParams p{};
    uint8_t *d_tr = nullptr;
    SD_TRY(bufs.alloc(&d_tr, (size_t)S * S));
    SD_TRY(alloc_fwd(bufs, &p.A, (size_t)chunk * slot));
    SD_TRY(alloc_fwd(bufs, &p.alpha, (size_t)chunk * slot));
    SD_TRY(bufs.alloc(&p.map_seg_start, (size_t)chunk * K * K));
    SD_TRY(bufs.alloc(&p.map_seg_state, (size_t)chunk * K * K));
    SD_TRY(bufs.alloc(&p.fin, (size_t)chunk * K * S * 5));
    if (marg) {
        SD_TRY(bufs.alloc(&p.beta.M, (size_t)chunk * slot));
        SD_TRY(bufs.alloc(&p.beta.Z, (size_t)chunk * slot));
        SD_TRY(bufs.alloc(&p.gamma.M, (size_t)chunk * slot));
        SD_TRY(bufs.alloc(&p.gamma.Z, (size_t)chunk * slot));
        SD_TRY(bufs.alloc(&p.cover, (size_t)chunk * slot));
        SD_TRY(bufs.alloc(&p.post, (size_t)chunk * slot));
        SD_TRY(bufs.alloc(&p.row_tot, (size_t)chunk * rows));
    }
    HIP_TRY(hipMemcpy(d_tr, transitions, (size_t)S * S, hipMemcpyHostToDevice));
    p.tr = d_tr;
    p.slot = slot;
    p.S = S;
    p.K = K;
    p.Tm = Tm;
    p.ld = ld;
    p.ntile = ntile;

    const std::vector<long double> ntraces = trace_counts(S, transitions, K);
    std::vector<double> fin((size_t)chunk * K * S * 5), post(marg ? (size_t)chunk * slot : 0);
    std::vector<int32_t> seg_a((size_t)chunk * K * K), seg_v((size_t)chunk * K * K);
    const double nan = std::numeric_limits<double>::quiet_NaN(), ninf = -std::numeric_limits<double>::infinity();

    for (int j0 = 0; j0 < n_traj; j0 += chunk) {
        const int nc = std::min(chunk, n_traj - j0);
        p.trajs = d_trajs + j0;
        p.n_traj = nc;
        if (launch_segdp_init(p, false, st)) return fail(BILD_ERR_HIP, "launch of the segment recursion's first level failed");
        for (int j = 1; j <= k_max; ++j)
            if (launch_segdp_mix(p, j, st) || launch_segdp_level(p, j, st))
                return fail(BILD_ERR_HIP, "launch of level %d of the segment recursion failed", j);
        if (launch_segdp_backtrack(p, st)) return fail(BILD_ERR_HIP, "launch of the back-pointer walk failed");
        if (marg) {
            if (launch_segdp_init(p, true, st)) return fail(BILD_ERR_HIP, "launch of the backward recursion's first level failed");
            for (int lv = 0; lv < k_max; ++lv)
                if (launch_segdp_blevel(p, lv, st) || launch_segdp_bmix(p, lv + 1, st))
                    return fail(BILD_ERR_HIP, "launch of level %d of the backward recursion failed", lv);
            if (launch_segdp_cover(p, st) || launch_segdp_carry(p, st)) return fail(BILD_ERR_HIP, "launch of the marginal kernels failed");
            HIP_TRY(hipMemcpyAsync(post.data(), p.post, (size_t)nc * slot * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(fin.data(), p.fin, (size_t)nc * K * S * 5 * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(seg_a.data(), p.map_seg_start, (size_t)nc * K * K * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(seg_v.data(), p.map_seg_state, (size_t)nc * K * K * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        for (int i = 0; i < nc; ++i) {
            const int jt = j0 + i, Tj = T[jt];
            for (int k = 0; k < K; ++k) {
                const size_t o = (size_t)jt * K + k;
                const double *f = fin.data() + ((size_t)i * K + k) * S * 5;
                const long double n_all = binom_ld(Tj - 1, k) * ntraces[k];
                double ok = 0.0, bad = 0.0, top = ninf, map_l = nan;
                bool have_map = false;
                for (int s = 0; s < S; ++s) {
                    ok += f[s * 5 + 3];
                    bad += f[s * 5 + 4];
                    if (f[s * 5 + 1] > 0.0) top = std::max(top, f[s * 5]);
                    if (f[s * 5 + 3] > 0.0 && (!have_map || f[s * 5] > map_l)) {
                        map_l = f[s * 5];
                        have_map = true;
                    }
                }
                const bool any = n_all > 0.0L;
                const double count = !any ? 0.0 : omit ? ok : (double)n_all;
                const double log_count = omit ? std::log(ok) : (double)logl(n_all);
                double logev = ninf, kl = nan;
                bool usable = false;
                if (any && !omit && bad > 0.0) logev = nan;
                else if (any && count > 0.0 && top != ninf) {
                    double z = 0.0, u = 0.0;
                    for (int s = 0; s < S; ++s) {
                        if (!(f[s * 5 + 1] > 0.0)) continue;
                        const double w = f[s * 5 + 1] * std::exp(f[s * 5] - top);
                        z += w;
                        if (w > 0.0) u += w * f[s * 5 + 2];
                    }
                    logev = top + std::log(z) - log_count;
                    kl = u / z - logev;
                    usable = true;
                }
                if (out->logev) out->logev[o] = logev;
                if (out->kl) out->kl[o] = kl;
                if (out->map_logl) out->map_logl[o] = any && have_map ? map_l : nan;
                if (out->n_profiles) out->n_profiles[o] = count;
                if (out->n_omitted) out->n_omitted[o] = any && omit ? bad : 0.0;
                if (out->map_seg_start) std::copy_n(seg_a.data() + ((size_t)i * K + k) * K, K, out->map_seg_start + o * K);
                if (out->map_seg_state) std::copy_n(seg_v.data() + ((size_t)i * K + k) * K, K, out->map_seg_state + o * K);
                if (!marg) continue;
                double *lp = out->log_post + o * S * T_max;
                const double *ps = post.data() + (size_t)i * slot + (size_t)k * S * ld;
                for (int t = 0; t < T_max; ++t) {
                    const bool in = usable && t < Tj;
                    double tot = 0.0;
                    if (in)
                        for (int s = 0; s < S; ++s) tot += ps[(size_t)s * ld + t];
                    for (int s = 0; s < S; ++s) lp[(size_t)s * T_max + t] = in ? std::log(ps[(size_t)s * ld + t]) - std::log(tot) : nan;
                }
            }
        }
    }
    return BILD_OK;
}
